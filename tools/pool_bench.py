#!/usr/bin/env python3
"""Stream pool benchmark: S live stereo streams (fft 2048, +4 st, phase-locked) fed 480-frame calls over 10 s of audio,
the slots joining staggered over the first 20 calls (with each call's host time -- planning, descriptors, staging,
enqueueing -- and its wait for the device); then, in the same process, the same S streams through S pv_engines
round-robin.  Prints one JSON line.   python tools/pool_bench.py [--slots 128] [--seconds 10]"""
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
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--engine-seconds", type=float, default=2.0, help="audio per stream for the pv_engine comparison")
args = ap.parse_args()
S, B, SR = args.slots, 480, 48000
kw = dict(semitones=4.0, coremode=1, fftsize=2048)
calls = int(args.seconds * SR) // B
src = signals.voice(SR, 2)  # one second, read by every stream from its own offset
L = E.lib()
fp = C.POINTER(C.c_float)


def block_ptrs(k, n_streams):
    """pointer table [stream][channel] of each stream's k-th block (stream j starts 97*j frames into the source)"""
    ptrs = (fp * (2 * n_streams))()
    for j in range(n_streams):
        off = (k * B + 97 * j) % (SR - B)
        for c in range(2):
            ptrs[2 * j + c] = src[c, off:].ctypes.data_as(fp)
    return ptrs


# ---- the pool
pool = E.StreamPool(S, channels=2, **kw)
out = np.zeros((2, 1 << 16), np.float32)
outp = (fp * 2)(out[0].ctypes.data_as(fp), out[1].ctypes.data_as(fp))
lat, host, wait, opened = [], [], [], 0
h_us, w_us = C.c_double(), C.c_double()
slots = np.zeros(S, np.int32)
n = np.full(S, B, np.int32)
t_all = time.perf_counter()
for k in range(calls):
    while opened < S and opened < (k + 1) * S // 20:
        slots[opened] = pool.open()
        opened += 1
    ptrs = block_ptrs(k, opened)
    t0 = time.perf_counter()
    st = L.pv_pool_feed(pool.h, opened, slots.ctypes.data, ptrs, n.ctypes.data)
    lat.append(time.perf_counter() - t0)
    if st != 0:
        raise SystemExit(f"pv_pool_feed: {L.pv_last_error().decode()}")
    L.pv_pool_last_timing(pool.h, C.byref(h_us), C.byref(w_us))
    host.append(h_us.value)
    wait.append(w_us.value)
    for j in range(opened):
        L.pv_pool_retrieve(pool.h, int(slots[j]), outp, L.pv_pool_available(pool.h, int(slots[j])))
t_pool = time.perf_counter() - t_all
steady = np.array(lat[20:]) * 1e6
pool.close_pool()
pool_xrt = S * args.seconds / t_pool  # aggregate stream-seconds per second

# ---- the same streams through S single-stream engines, round-robin
ecalls = int(args.engine_seconds * SR) // B
engines = [E.PhaseVocoder(SR, 2, 1.0, 4.0, E.NORMAL_SHIFT, E.PHASE_LOCKED, 2048) for _ in range(S)]
elat = []
t_all = time.perf_counter()
for k in range(ecalls):
    ptrs = block_ptrs(k, S)
    for j, pv in enumerate(engines):
        t0 = time.perf_counter()
        L.pv_feed(pv.h, C.cast(C.addressof(ptrs) + 2 * j * C.sizeof(fp), C.POINTER(fp)), B)
        elat.append(time.perf_counter() - t0)
        L.pv_retrieve(pv.h, outp, L.pv_available(pv.h))
t_eng = time.perf_counter() - t_all
for pv in engines:
    pv.close()
eng_xrt = S * args.engine_seconds / t_eng
elat = np.array(elat) * 1e6

print(json.dumps({
    "workload": f"{S} live stereo streams, +4 st, fft 2048, phase-locked, {B}-frame calls, {args.seconds:g} s of audio",
    "pool_feed_us_median": round(float(np.median(steady)), 1),
    "pool_feed_us_p99": round(float(np.percentile(steady, 99)), 1),
    "pool_host_us_median": round(float(np.median(host[20:])), 1),  # planning, descriptors, staging, enqueueing
    "pool_wait_us_median": round(float(np.median(wait[20:])), 1),  # waiting for the device after that
    "pool_aggregate_x_realtime": round(pool_xrt, 1),
    "pool_per_slot_x_realtime": round(pool_xrt / S, 2),
    "engines_round_us_median": round(float(np.median(elat)) * S, 1),
    "engines_feed_us_median": round(float(np.median(elat)), 1),
    "engines_aggregate_x_realtime": round(eng_xrt, 1),
    "pool_vs_engines": round(pool_xrt / eng_xrt, 2),
}))
