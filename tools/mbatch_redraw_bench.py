#!/usr/bin/env python3
"""Mixed batch, redraw against rebuild, on the corpus of tools/mbatch_bench.py (128 stereo 48 kHz clips of 5 ... 60 s,
fft 2048, phase-locked, block 480, flush; same seed and sizes); a second and a third draw of lengths and pitches come
from the same generator.
  1. what creation costs: pv_mbatch_layout (planning only, no device) against MixedBatch(...) on the same streams, and
     the three-way split of pv_mbatch_last_build_timing for that creation;
  2. alternating, after one warm-up of each, `repeats` times each (wall clock, device synchronised before and after):
       a  close() + a new MixedBatch for the next draw   (all there was before redraw)
       b  redraw to the next draw
     Acceptance: b's median is below a's by more than the larger of the two spreads (max - min).
Prints one JSON line.
  python tools/mbatch_redraw_bench.py [--streams 128] [--min-seconds 5] [--max-seconds 60] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiomod_amd import engine as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--min-seconds", type=float, default=5.0)
ap.add_argument("--max-seconds", type=float, default=60.0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--seed", type=int, default=20240)
args = ap.parse_args()
S, B, SR, C = args.streams, 480, 48000, 2
kw = dict(coremode=1, fftsize=2048)
rng = np.random.default_rng(args.seed)


def draw(k):
    frames = [int(f) for f in rng.integers(int(args.min_seconds * SR), int(args.max_seconds * SR) + 1, S)]
    if k == 0:  # the benchmark corpus itself
        return [(f, float(-12 + i % 25), 1.0) for i, f in enumerate(frames)]
    return [(f, float(p), 1.0) for f, p in zip(frames, rng.integers(-12, 13, S))]


draws = [draw(k) for k in range(3)]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


torch.zeros(1, device="cuda:0")
layout_ms, _ = wall(lambda: E.mbatch_layout(draws[0], channels=C, block=B, **kw))
create_ms, mb = wall(lambda: E.MixedBatch(draws[0], channels=C, block=B, **kw))
create_split = mb.last_build_timing()
other = E.MixedBatch(draws[0], channels=C, block=B, **kw)  # leg a's object


def leg_a(k):
    global other
    other.close()
    other = E.MixedBatch(draws[k], channels=C, block=B, **kw)


ta, tb, split = [], [], None
for rep in range(args.repeats + 1):
    k = 1 + rep % 2
    a, _ = wall(lambda: leg_a(k))
    b, _ = wall(lambda: mb.redraw(draws[k]))
    if rep:  # (the first of each is the warm-up)
        ta.append(a), tb.append(b)
        split = mb.last_build_timing()
same = mb.out_frames == other.out_frames and mb.kernel_launches == other.kernel_launches
med_a, med_b = statistics.median(ta), statistics.median(tb)
spread_a, spread_b = max(ta) - min(ta), max(tb) - min(tb)
print(json.dumps(dict(
    streams=S, audio_seconds=sum(f for f, _, _ in draws[0]) / SR,
    layout_ms=layout_ms, create_ms=create_ms, create_minus_layout_ms=create_ms - layout_ms, create_split_us=create_split,
    rebuild_ms=dict(median=med_a, spread=spread_a, all=ta), redraw_ms=dict(median=med_b, spread=spread_b, all=tb),
    redraw_split_us=split, ratio=med_a / med_b, margin_cleared=bool(med_a - med_b > max(spread_a, spread_b)),
    same_layout_as_rebuilt=bool(same))))
