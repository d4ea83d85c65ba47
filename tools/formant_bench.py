#!/usr/bin/env python3
"""The formant setting: what switching it on costs, on the two workloads the README quotes (fft 2048, phase-locked).
  pool   128 stereo slots, +4 st, 480-frame pv_pool_feed calls (wall time of a call, its wait included): a pool with
         the setting off in every slot against a pool with it on at 0 (formant-preserving shift) in every slot;
  mixed  tools/mbatch_bench.py's corpus -- 128 stereo clips of 5 ... 60 s, 25 pitches -12 ... +12 st -- as one
         MixedBatch.run (device events), the setting off for every stream against on at 0 for every stream (the clips
         at pitch 0 have env_comp 1 and skip the stage, as mode formant_cepstral does).
Both legs run in one process, alternating, --repeats rounds (default five) after a warm-up round; a round of the pool is
the median of --feeds calls.  Prints median and range per leg, the launches per call / run and one JSON line; --out FILE
appends the same there.   python tools/formant_bench.py [--repeats 5] [--out profiles/r17/formant.txt]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiomod_amd import engine as E, signals  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--feeds", type=int, default=100)
ap.add_argument("--warm", type=int, default=40)
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--min-seconds", type=float, default=5.0)
ap.add_argument("--max-seconds", type=float, default=60.0)
ap.add_argument("--seed", type=int, default=20240)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if E.lib().pv_device_count() < 1:
    raise SystemExit("formant_bench: no gfx950 device visible (there is no CPU fallback: nothing is measured)")
CAP, B, SR = 128, 480, 48000
L = E.lib()
fp = C.POINTER(C.c_float)
src = signals.voice(SR, 2)


def stat(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3), max=round(float(max(v)), 3))


# ---- pool
kw = dict(semitones=4.0, coremode=1, fftsize=2048)
pools = {"off": E.StreamPool(CAP, channels=2, **kw), "on": E.StreamPool(CAP, channels=2, **kw)}
slots = {k: np.array([p.open() for _ in range(CAP)], np.int32) for k, p in pools.items()}
for s in slots["on"]:
    pools["on"].set_formant(int(s), 0.0)
n = np.full(CAP, B, np.int32)
blocks = np.ascontiguousarray(np.stack([src[:, (97 * j) % (SR - B):][:, :B] for j in range(CAP)]), np.float32)
rows = (fp * (2 * CAP))(*[blocks[j, c].ctypes.data_as(fp) for j in range(CAP) for c in range(2)])
sink = np.zeros((2, 1 << 16), np.float32)
sinkp = (fp * 2)(sink[0].ctypes.data_as(fp), sink[1].ctypes.data_as(fp))


def feed(key):
    """one 480-frame feed of every slot (everything retrieved afterwards, untimed); its wall time in us"""
    pool, sl = pools[key], slots[key]
    t0 = time.perf_counter()
    st = L.pv_pool_feed(pool.h, len(sl), sl.ctypes.data, rows, n.ctypes.data)
    dt = (time.perf_counter() - t0) * 1e6
    if st != 0:
        raise SystemExit(f"pv_pool_feed: {L.pv_last_error().decode()}")
    for s in sl:
        L.pv_pool_retrieve(pool.h, int(s), sinkp, L.pv_pool_available(pool.h, int(s)))
    return dt


for _ in range(args.warm):
    feed("off"), feed("on")
pool_us = {"off": [], "on": []}
for r in range(-1, args.repeats):  # (-1: warm-up round, not recorded)
    for key in ("off", "on") if r % 2 == 0 else ("on", "off"):
        v = [feed(key) for _ in range(args.feeds)]
        if r >= 0:
            pool_us[key].append(float(np.median(v)))
pool_launches = {k: pools[k].last_launches() for k in pools}
for p in pools.values():
    p.close_pool()

# ---- mixed batch
S = args.streams
rng = np.random.default_rng(args.seed)
frames = [int(f) for f in rng.integers(int(args.min_seconds * SR), int(args.max_seconds * SR) + 1, S)]
streams = [(f, float(-12 + i % 25), 1.0) for i, f in enumerate(frames)]
host = [np.ascontiguousarray(np.tile(np.roll(src, 977 * i, axis=1), (1, f // SR + 1))[:, :f]) for i, f in enumerate(frames)]
mb = E.MixedBatch(streams, channels=2, block=B, coremode=1, fftsize=2048)
d_in, d_out = mb.pack(host), mb.alloc_out()
del host


def run_ms():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    mb.run(d_in, d_out)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


mb_ms, mb_launches = {"off": [], "on": []}, {}
for r in range(-1, args.repeats):
    for key in ("off", "on") if r % 2 == 0 else ("on", "off"):
        mb.set_formant(None if key == "off" else [0.0] * S)  # (synchronises; outside the timed window)
        mb_launches[key] = mb.kernel_launches
        run_ms()  # (one untimed run after the switch)
        t = run_ms()
        if r >= 0:
            mb_ms[key].append(t)
mb.close()

res = dict(pool_feed_us={k: stat(v) for k, v in pool_us.items()}, pool_launches=pool_launches,
           mbatch_run_ms={k: stat(v) for k, v in mb_ms.items()}, mbatch_kernel_launches=mb_launches)
lines = [f"formant setting, speed: fft 2048, phase-locked, stereo; {args.repeats} rounds after one warm-up round, legs alternating",
         f"pool: {CAP} slots, +4 st, {B}-frame pv_pool_feed calls, wall time per call (a round: median of {args.feeds} calls)",
         f"mixed batch: {S} clips of {args.min_seconds:g} ... {args.max_seconds:g} s ({sum(frames) / SR:.0f} s), 25 pitches, "
         f"one MixedBatch.run, device events",
         f"{'what':<28} {'median':>10} {'min':>10} {'max':>10} {'launches':>9}"]
for key in ("off", "on"):
    v = res["pool_feed_us"][key]
    lines.append(f"{'pool feed, setting ' + key + ' (us)':<28} {v['median']:>10.1f} {v['min']:>10.1f} {v['max']:>10.1f} "
                 f"{pool_launches[key]:>9}")
for key in ("off", "on"):
    v = res["mbatch_run_ms"][key]
    lines.append(f"{'mixed batch, setting ' + key + ' (ms)':<28} {v['median']:>10.3f} {v['min']:>10.3f} {v['max']:>10.3f} "
                 f"{mb_launches[key]:>9}")
lines.append(json.dumps(res))
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")
