#!/usr/bin/env python3
"""The voice setting: what the WHISPER voice costs against the ROBOTIC one -- the two differ by the generator alone
(fft 2048, stereo, mode robotic).
  pool   128 slots, 480-frame pv_pool_feed calls: a pool with every slot robotic against a pool with every slot
         whisper; per call the wall time (its wait included), the host time up to the wait (pv_pool_last_timing) and the
         kernels launched;
  mixed  tools/mbatch_bench.py's corpus -- 128 stereo clips of 5 ... 60 s, 25 pitches -12 ... +12 st -- as one
         MixedBatch.run (device events), every stream robotic against every stream whisper;
  set    the wall time of MixedBatch.set_voice (all whisper: it draws the shared phase table) and of redraw on that
         corpus.
All legs run in one process, alternating, --repeats rounds (default five) after a warm-up round; a round of the pool is
the median of --feeds calls.  Prints median and range per leg and one JSON line; --out FILE appends the same there.
  python tools/voice_bench.py [--repeats 5] [--out profiles/r18/voice.txt]"""
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
    raise SystemExit("voice_bench: no gfx950 device visible (there is no CPU fallback: nothing is measured)")
CAP, B, SR = 128, 480, 48000
L = E.lib()
fp = C.POINTER(C.c_float)
src = signals.voice(SR, 2)
VOICES = ("robotic", "whisper")


def stat(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3), max=round(float(max(v)), 3))


# ---- pool
kw = dict(mode="robotic", fftsize=2048)
pools = {k: E.StreamPool(CAP, channels=2, **kw) for k in VOICES}
slots = {k: np.array([p.open(voice=k) for _ in range(CAP)], np.int32) for k, p in pools.items()}
n = np.full(CAP, B, np.int32)
blocks = np.ascontiguousarray(np.stack([src[:, (97 * j) % (SR - B):][:, :B] for j in range(CAP)]), np.float32)
rows = (fp * (2 * CAP))(*[blocks[j, c].ctypes.data_as(fp) for j in range(CAP) for c in range(2)])
sink = np.zeros((2, 1 << 16), np.float32)
sinkp = (fp * 2)(sink[0].ctypes.data_as(fp), sink[1].ctypes.data_as(fp))


def feed(key):
    """one 480-frame feed of every slot (everything retrieved afterwards, untimed): wall us, host us, launches"""
    pool, sl = pools[key], slots[key]
    t0 = time.perf_counter()
    st = L.pv_pool_feed(pool.h, len(sl), sl.ctypes.data, rows, n.ctypes.data)
    dt = (time.perf_counter() - t0) * 1e6
    if st != 0:
        raise SystemExit(f"pv_pool_feed: {L.pv_last_error().decode()}")
    host_us = pool.last_timing()[0]
    launches = pool.last_launches()
    for s in sl:
        L.pv_pool_retrieve(pool.h, int(s), sinkp, L.pv_pool_available(pool.h, int(s)))
    return dt, host_us, launches


for _ in range(args.warm):
    feed("robotic"), feed("whisper")
pool_us = {k: [] for k in VOICES}
pool_host_us = {k: [] for k in VOICES}
pool_launches = {k: 0 for k in VOICES}
for r in range(-1, args.repeats):  # (-1: warm-up round, not recorded)
    for key in VOICES if r % 2 == 0 else VOICES[::-1]:
        v = [feed(key) for _ in range(args.feeds)]
        if r >= 0:
            pool_us[key].append(float(np.median([x[0] for x in v])))
            pool_host_us[key].append(float(np.median([x[1] for x in v])))
            pool_launches[key] = max(x[2] for x in v)  # (a call that completes slices: most do at this block size)
for p in pools.values():
    p.close_pool()

# ---- mixed batch
S = args.streams
rng = np.random.default_rng(args.seed)
frames = [int(f) for f in rng.integers(int(args.min_seconds * SR), int(args.max_seconds * SR) + 1, S)]
streams = [(f, float(-12 + i % 25), 1.0) for i, f in enumerate(frames)]
host = [np.ascontiguousarray(np.tile(np.roll(src, 977 * i, axis=1), (1, f // SR + 1))[:, :f]) for i, f in enumerate(frames)]
mb = E.MixedBatch(streams, channels=2, block=B, mode="robotic", fftsize=2048)
d_in, d_out = mb.pack(host), mb.alloc_out()
del host
slices = max(E.mbatch_layout(streams, channels=2, block=B, mode="robotic", fftsize=2048)["slices"])


def run_ms():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    mb.run(d_in, d_out)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


mb_ms, mb_launches = {k: [] for k in VOICES}, {}
set_ms, redraw_ms = [], []
for r in range(-1, args.repeats):
    for key in VOICES if r % 2 == 0 else VOICES[::-1]:
        if key == "robotic":
            t = wall_ms(lambda: mb.redraw(streams))  # (every stream robotic again, like a new object)
            if r >= 0:
                redraw_ms.append(t)
        else:
            t = wall_ms(lambda: mb.set_voice(["whisper"] * S))
            if r >= 0:
                set_ms.append(t)
        mb_launches[key] = mb.kernel_launches
        run_ms()  # (one untimed run after the switch)
        t = run_ms()
        if r >= 0:
            mb_ms[key].append(t)
mb.close()

res = dict(pool_feed_us={k: stat(v) for k, v in pool_us.items()}, pool_host_us={k: stat(v) for k, v in pool_host_us.items()},
           pool_launches=pool_launches, mbatch_run_ms={k: stat(v) for k, v in mb_ms.items()},
           mbatch_kernel_launches=mb_launches, mbatch_set_voice_ms=stat(set_ms), mbatch_redraw_ms=stat(redraw_ms),
           mbatch_table_slices=slices, mbatch_table_bytes=slices * 2 * (1024 + 8) * 4)
lines = [f"voice setting, speed: mode robotic, fft 2048, stereo; {args.repeats} rounds after one warm-up round, legs alternating",
         f"pool: {CAP} slots, {B}-frame pv_pool_feed calls; per call wall time, host time up to the wait, kernels "
         f"(a round: median of {args.feeds} calls)",
         f"mixed batch: {S} clips of {args.min_seconds:g} ... {args.max_seconds:g} s ({sum(frames) / SR:.0f} s), 25 pitches, "
         f"one MixedBatch.run, device events; phase table {slices} slices = {res['mbatch_table_bytes']} bytes",
         f"{'what':<34} {'median':>10} {'min':>10} {'max':>10} {'launches':>9}"]
for key in VOICES:
    v = res["pool_feed_us"][key]
    lines.append(f"{'pool feed, all ' + key + ' (us)':<34} {v['median']:>10.1f} {v['min']:>10.1f} {v['max']:>10.1f} "
                 f"{pool_launches[key]:>9}")
for key in VOICES:
    v = res["pool_host_us"][key]
    lines.append(f"{'  its host part, ' + key + ' (us)':<34} {v['median']:>10.1f} {v['min']:>10.1f} {v['max']:>10.1f}")
for key in VOICES:
    v = res["mbatch_run_ms"][key]
    lines.append(f"{'mixed batch, all ' + key + ' (ms)':<34} {v['median']:>10.3f} {v['min']:>10.3f} {v['max']:>10.3f} "
                 f"{mb_launches[key]:>9}")
for name, v in (("set_voice, all whisper (ms)", res["mbatch_set_voice_ms"]), ("redraw (ms)", res["mbatch_redraw_ms"])):
    lines.append(f"{name:<34} {v['median']:>10.3f} {v['min']:>10.3f} {v['max']:>10.3f}")
lines.append(json.dumps(res))
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")
