#!/usr/bin/env python3
"""Mixed stream pool benchmark: 128 live stereo streams (fft 2048, phase-locked) fed 480-frame calls, all slots open
from the start, in four runs:
  a  a uniform pool (pv_pool_create) at +4 st;
  b  a mixed pool (pv_pool_create_mixed, -12 ... +12 st) with every slot at +4 st;
  c  a mixed pool with the slots spread over 25 pitches, -12 ... +12 st;
  d  the streams of c through 25 uniform pools, one per pitch, fed in turn (a "feed" = one call of all 25).
Per run: median and p99 per feed, the median host / wait split (summed over the pools in d) and the launches per feed.
Prints one JSON line.   python tools/pool_mixed_bench.py [--slots 128] [--seconds 5]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiomod_amd import engine as E, signals  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=128)
ap.add_argument("--seconds", type=float, default=5.0)
args = ap.parse_args()
S, B, SR, WARM = args.slots, 480, 48000, 20
kw = dict(semitones=4.0, coremode=1, fftsize=2048)
calls = int(args.seconds * SR) // B
PITCHES = [float(p) for p in range(-12, 13)]  # 25
src = signals.voice(SR, 2)
L = E.lib()
fp = C.POINTER(C.c_float)
out = np.zeros((2, 1 << 16), np.float32)
outp = (fp * 2)(out[0].ctypes.data_as(fp), out[1].ctypes.data_as(fp))


def block_ptrs(k, streams):
    ptrs = (fp * (2 * len(streams)))()
    for i, j in enumerate(streams):
        off = (k * B + 97 * j) % (SR - B)
        for c in range(2):
            ptrs[2 * i + c] = src[c, off:].ctypes.data_as(fp)
    return ptrs


def run(pools):
    """pools: [(pool, slots, stream ids)]; every call feeds each pool once, in turn."""
    lat, host, wait, launches = [], [], [], []
    h_us, w_us, nl = C.c_double(), C.c_double(), C.c_int32()
    prepared = []
    for pool, slots, streams in pools:
        prepared.append((pool, np.array(slots, np.int32), np.full(len(slots), B, np.int32), streams))
    for k in range(calls):
        ptrs = [block_ptrs(k, streams) for _, _, _, streams in prepared]
        t0 = time.perf_counter()
        hs = ws = ls = 0
        for (pool, slots, n, _), pt in zip(prepared, ptrs):
            if L.pv_pool_feed(pool.h, len(slots), slots.ctypes.data, pt, n.ctypes.data) != 0:
                raise SystemExit(f"pv_pool_feed: {L.pv_last_error().decode()}")
            L.pv_pool_last_timing(pool.h, C.byref(h_us), C.byref(w_us))
            L.pv_pool_last_launches(pool.h, C.byref(nl))
            hs += h_us.value
            ws += w_us.value
            ls += nl.value
        lat.append(time.perf_counter() - t0)
        host.append(hs)
        wait.append(ws)
        launches.append(ls)
        for pool, slots, _, _ in prepared:
            for s in slots:
                L.pv_pool_retrieve(pool.h, int(s), outp, L.pv_pool_available(pool.h, int(s)))
    steady = np.array(lat[WARM:]) * 1e6
    return {"feed_us_median": round(float(np.median(steady)), 1),
            "feed_us_p99": round(float(np.percentile(steady, 99)), 1),
            "host_us_median": round(float(np.median(host[WARM:])), 1),
            "wait_us_median": round(float(np.median(wait[WARM:])), 1),
            "launches_per_feed": int(np.median(launches[WARM:]))}


res = {}
pool = E.StreamPool(S, channels=2, **kw)
res["a_uniform_+4"] = run([(pool, [pool.open() for _ in range(S)], list(range(S)))])
pool.close_pool()
pool = E.StreamPool(S, channels=2, pitch_range=(-12, 12), **kw)
res["b_mixed_all_+4"] = run([(pool, [pool.open(semitones=4.0) for _ in range(S)], list(range(S)))])
pool.close_pool()
pool = E.StreamPool(S, channels=2, pitch_range=(-12, 12), **kw)
res["c_mixed_25_pitches"] = run([(pool, [pool.open(semitones=PITCHES[j % 25]) for j in range(S)], list(range(S)))])
pool.close_pool()
pools = []
for i, p in enumerate(PITCHES):
    streams = [j for j in range(S) if j % 25 == i]
    u = E.StreamPool(len(streams), channels=2, **dict(kw, semitones=p))
    pools.append((u, [u.open() for _ in streams], streams))
res["d_25_uniform_pools"] = run(pools)
for u, _, _ in pools:
    u.close_pool()
print(json.dumps({"workload": f"{S} live stereo streams, fft 2048, phase-locked, {B}-frame calls, "
                              f"{args.seconds:g} s of audio", **res}))
