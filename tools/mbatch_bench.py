#!/usr/bin/env python3
"""Mixed batch benchmark: 128 stereo 48 kHz clips (fft 2048, phase-locked, block 480, flush) whose lengths are drawn
uniformly from 5 ... 60 s with a fixed seed and whose pitches cycle through 25 values, -12 ... +12 st, ratio 1; input
resident on the device.  Times, alternating, after one warm-up run of each:
  mixed  one MixedBatch.run over all clips (device events around the run);
  a      one Batch(1, frames_i) per clip, run back to back (device events around the 128 runs; creation excluded);
  b      a mixed StreamPool of 128 slots fed 480-frame calls from host memory the way run_offline drives an engine:
         each slot its clip, then zero blocks until it has produced `frames` (wall clock; the pool is synchronous).
Prints one JSON line: the three medians with their spreads (max - min over the repeats), total channel-samples/s of
each, the mixed batch's launch groups and kernels per run, and whether the mixed outputs equal a's bit for bit.
  python tools/mbatch_bench.py [--streams 128] [--min-seconds 5] [--max-seconds 60] [--repeats 5] [--no-pool]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiomod_amd import engine as E, signals  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--min-seconds", type=float, default=5.0)
ap.add_argument("--max-seconds", type=float, default=60.0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--seed", type=int, default=20240)
ap.add_argument("--no-pool", action="store_true", help="skip alternative b")
args = ap.parse_args()
S, B, SR, C = args.streams, 480, 48000, 2
kw = dict(coremode=1, fftsize=2048)
rng = np.random.default_rng(args.seed)
frames = [int(f) for f in rng.integers(int(args.min_seconds * SR), int(args.max_seconds * SR) + 1, S)]
pitches = [float(-12 + i % 25) for i in range(S)]
streams = [(f, p, 1.0) for f, p in zip(frames, pitches)]
dev = torch.device("cuda:0")

# one second of the test voice per stream phase, tiled to each clip's length (the content does not change the work)
src = signals.voice(SR, C)
host = [np.ascontiguousarray(np.tile(np.roll(src, 977 * i, axis=1), (1, f // SR + 1))[:, :f]) for i, f in enumerate(frames)]

t0 = time.perf_counter()
mb = E.MixedBatch(streams, channels=C, block=B, **kw)
create_mixed_s = time.perf_counter() - t0
d_in = mb.pack(host)
d_out = mb.alloc_out()
t0 = time.perf_counter()
singles = [E.Batch(1, f, channels=C, block=B, semitones=p, **kw) for f, p, _ in streams]
create_singles_s = time.perf_counter() - t0
ins = [d_in[o:o + C * f].view(1, C, f) for o, f in zip(mb.in_offsets, frames)]
outs = [b.alloc_out() for b in singles]
assert [b.out_frames for b in singles] == mb.out_frames


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def run_mixed():
    mb.run(d_in, d_out)


def run_singles():
    for b, x, y in zip(singles, ins, outs):
        b.run(x, y)


pool = None if args.no_pool else E.StreamPool(S, channels=C, pitch_range=(-12, 12), semitones=0.0, **kw)
zeros = np.zeros((C, B), np.float32)


def run_pool():
    """every clip through its own slot, 480 frames per call, all live slots in one feed"""
    t_start = time.perf_counter()
    slot = {pool.open(semitones=p): i for i, p in enumerate(pitches)}
    produced = {s: 0 for s in slot}
    pos = {s: 0 for s in slot}
    while slot:
        blocks = {}
        for s, i in slot.items():
            blk = host[i][:, pos[s]:pos[s] + B] if pos[s] < frames[i] else zeros
            blocks[s] = blk
            pos[s] += B
        pool.feed(blocks)
        for s in list(slot):
            got = pool.available(s)
            if got:
                pool.retrieve(s, got)
            produced[s] += got
            if pos[s] >= frames[slot[s]] and produced[s] >= frames[slot[s]]:
                pool.close(s)
                del slot[s]
    return (time.perf_counter() - t_start) * 1e3


times = {"mixed": [], "a": [], "b": []}
for rep in range(args.repeats + 1):  # the first pass of each is the warm-up
    tm, ta = timed(run_mixed), timed(run_singles)
    tb = run_pool() if pool is not None else None
    if rep:
        times["mixed"].append(tm), times["a"].append(ta)
        if tb is not None:
            times["b"].append(tb)

same = all(torch.equal(v.view(torch.int32), y[0].view(torch.int32)) for v, y in zip(mb.split(d_out), outs))
total = C * sum(frames)


def stat(v):
    return None if not v else {"median_ms": round(float(np.median(v)), 3), "spread_ms": round(float(max(v) - min(v)), 3),
                               "gsamples_per_s": round(total / (float(np.median(v)) * 1e-3) / 1e9, 4)}


res = {k: stat(v) for k, v in times.items()}
best_alt = min(r["median_ms"] for k, r in res.items() if k != "mixed" and r)
spread = max(r["spread_ms"] for r in res.values() if r)
print(json.dumps({
    "workload": f"{S} stereo 48 kHz clips of {args.min_seconds:g} ... {args.max_seconds:g} s ({sum(frames) / SR:.0f} s in "
                f"all), 25 pitches -12 ... +12 st, fft 2048, phase-locked, block {B}, flush",
    "channel_samples": total, "mixed": res["mixed"], "a_batch_per_clip": res["a"], "b_mixed_pool": res["b"],
    "launch_groups": mb.launches, "kernel_launches": mb.kernel_launches,
    "create_s": {"mixed": round(create_mixed_s, 2), "a": round(create_singles_s, 2)},
    "margin_ms": round(best_alt - res["mixed"]["median_ms"], 3), "largest_spread_ms": spread,
    "beats_alternatives_by_more_than_spread": bool(best_alt - res["mixed"]["median_ms"] > spread),
    "bits_equal_to_a": bool(same)}))
sys.exit(0 if same else 1)
