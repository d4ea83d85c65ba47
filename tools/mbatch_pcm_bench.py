#!/usr/bin/env python3
"""PCM wire of the mixed batch against the float run it wraps, on tools/mbatch_bench.py's corpus (128 stereo 48 kHz
clips of 5 ... 60 s, fixed seed, 25 pitches, fft 2048, phase-locked, block 480, flush; 16-bit input).  In one session,
alternating, `--repeats` passes after one warm-up pass:
  run           MixedBatch.run on device-resident float (the yardstick: the code the PCM wire leaves as it was);
  run_pcm       MixedBatch.run_pcm on device-resident PCM (device events around the call);
  run_pcm_host  MixedBatch.run_pcm_host from and to page-locked host memory (wall clock: the call is synchronous);
  ingest, egress   the two conversion kernels alone (device events), also as bytes moved per second (PCM + float side).
Prints one JSON line with median and range (min, max) of each, and whether run_pcm's output equals the host-converted
run's bit for bit.
  python tools/mbatch_pcm_bench.py [--streams 128] [--min-seconds 5] [--max-seconds 60] [--repeats 5] [--bits 16]"""
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
ap.add_argument("--streams", type=int, default=128)
ap.add_argument("--min-seconds", type=float, default=5.0)
ap.add_argument("--max-seconds", type=float, default=60.0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--seed", type=int, default=20240)
ap.add_argument("--bits", type=int, default=16, choices=(8, 16, 24, 32))
args = ap.parse_args()
S, B, SR, CH = args.streams, 480, 48000, 2
kw = dict(coremode=1, fftsize=2048)
rng = np.random.default_rng(args.seed)
frames = [int(f) for f in rng.integers(int(args.min_seconds * SR), int(args.max_seconds * SR) + 1, S)]
streams = [(f, float(-12 + i % 25), 1.0) for i, f in enumerate(frames)]

src = signals.voice(SR, CH, dtype=np.float64)  # one second, tiled to each clip's length, as integer samples [frames][CH]
scale = {8: 128.0, 16: 32768.0, 24: 8388608.0, 32: 2147483648.0}[args.bits]
ints = np.round(src * scale).astype(np.int64) + (128 if args.bits == 8 else 0)
clips = [np.ascontiguousarray(np.tile(np.roll(ints, 977 * i, axis=1), (1, f // SR + 1))[:, :f].T) for i, f in enumerate(frames)]

mb = E.MixedBatch(streams, channels=CH, block=B, **kw)
bits = args.bits
lay = mb.pcm_layout(bits)
h_in = torch.from_numpy(mb.pack_pcm_host(clips, bits)).pin_memory()
h_out = torch.zeros(lay["out_bytes"], dtype=torch.uint8).pin_memory()
d_pcm_in = h_in.to("cuda:0")
d_pcm_out = mb.alloc_pcm_out()
# the float input the reader's conversion gives (exact in float at 8 / 16 / 24 bits; one rounding at 32)
sub = 128 if bits == 8 else 0
d_in = mb.pack([((x.T - sub).astype(np.float64) / scale).astype(np.float32) for x in clips])
d_out = mb.alloc_out()
stream = torch.cuda.current_stream()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def kernel(which):
    E._check(mb.L.pv_mbatch_debug_pcm_kernel(mb.h, which, C.c_void_p(d_pcm_in.data_ptr()), C.c_void_p(d_pcm_out.data_ptr()),
                                             C.c_void_p(stream.cuda_stream)), "pv_mbatch_debug_pcm_kernel")


what = {
    "run": lambda: timed(lambda: mb.run(d_in, d_out)),
    "run_pcm": lambda: timed(lambda: mb.run_pcm(d_pcm_in, bits, d_pcm_out)),
    "run_pcm_host": lambda: wall(lambda: mb.run_pcm_host(h_in, bits, h_out)),
    "ingest": lambda: timed(lambda: kernel(0)),
    "egress": lambda: timed(lambda: kernel(1)),
}
times = {k: [] for k in what}
for rep in range(args.repeats + 1):  # the first pass is the warm-up (and makes the PCM job table resident)
    for k in ("run", "run_pcm", "run_pcm_host", "ingest", "egress"):
        t = what[k]()
        if rep:
            times[k].append(t)

mb.run(d_in, d_out)
mb.run_pcm(d_pcm_in, bits, d_pcm_out)
torch.cuda.synchronize()
want = torch.clamp(d_out * 32768.0, -32768.0, 32767.0).trunc().to(torch.int16)
same = all(torch.equal(p.reshape(-1), want[o:o + CH * f].view(CH, f).t().reshape(-1))
           for p, o, f in zip(mb.split_pcm(d_pcm_out), mb.out_offsets, mb.out_frames))
same_host = bool(torch.equal(h_out.to("cuda:0"), d_pcm_out)) if lay["out_bytes"] else True

total_in, total_out = CH * sum(frames), CH * sum(mb.out_frames)
moved = {"ingest": total_in * (bits // 8 + 4), "egress": total_out * (4 + 2)}


def stat(k):
    v = times[k]
    med = float(np.median(v))
    out = {"median_ms": round(med, 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
    if k in moved:
        out["gbytes_per_s"] = round(moved[k] / (med * 1e-3) / 1e9, 1)
    else:
        out["gsamples_per_s"] = round(total_in / (med * 1e-3) / 1e9, 3)
    return out


res = {k: stat(k) for k in what}
pair = res["ingest"]["median_ms"] + res["egress"]["median_ms"]
print(json.dumps({
    "workload": f"{S} stereo 48 kHz clips of {args.min_seconds:g} ... {args.max_seconds:g} s ({sum(frames) / SR:.0f} s in "
                f"all), {bits}-bit input, 25 pitches -12 ... +12 st, fft 2048, phase-locked, block {B}, flush",
    "channel_samples": total_in, "pcm_in_bytes": lay["in_bytes"], "pcm_out_bytes": lay["out_bytes"], **res,
    "kernel_pair_ms": round(pair, 3), "kernel_pair_share_of_run": round(pair / res["run"]["median_ms"], 4),
    "repeats": args.repeats, "pcm_equals_converted_run": bool(same), "host_equals_device": same_host}))
sys.exit(0 if same and same_host else 1)
