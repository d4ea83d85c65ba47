#!/usr/bin/env python3
"""Stream pool, host feed against device-resident feed: S live stereo streams (fft 2048, +4 st, phase-locked), 480-frame
calls, three legs on three pools of one process:
  (a) pv_pool_feed from host memory, then pv_pool_retrieve of every slot (the synchronous pair);
  (b) pv_pool_feed_device, float32, input resident on the device, output left there;
  (c) pv_pool_feed_device, int16 likewise.
One warm-up round, then --repeats rounds; a round runs --calls calls of each leg in turn (a, b, c, a, b, c, ...), so that
the legs see the same machine state.  A leg's round is timed from its first call to the end of a device
synchronisation behind its last one; a call's host time is the wall-clock time of the C call(s) alone ((a): the feed,
which includes its wait for the device, plus the 2 S retrieve / available calls).  Prints a table and one JSON line;
--out FILE writes both there too.   python tools/pool_device_bench.py [--slots 128] [--calls 200] [--repeats 5]"""
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
ap.add_argument("--slots", type=int, default=128)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
S, B, SR, NBLK = args.slots, 480, 48000, 16
kw = dict(semitones=4.0, coremode=1, fftsize=2048)
src = signals.voice(SR, 2)  # one second, read by every stream from its own offset
L = E.lib()
fp = C.POINTER(C.c_float)

# NBLK different blocks per stream, used in turn: host float32 [NBLK][S][2][B], and the same on the device in both wires
host = np.stack([np.stack([src[:, (k * B + 97 * j) % (SR - B):][:, :B] for j in range(S)]) for k in range(NBLK)])
host = np.ascontiguousarray(host, np.float32)
dev_f32 = torch.from_numpy(host).cuda()
dev_i16 = torch.from_numpy(np.rint(host * 32768.0).astype(np.int16)).cuda()
ptrs = []
for k in range(NBLK):
    t = (fp * (2 * S))()
    for j in range(S):
        for c in range(2):
            t[2 * j + c] = host[k, j, c].ctypes.data_as(fp)
    ptrs.append(t)

pools = [E.StreamPool(S, channels=2, **kw) for _ in range(3)]
slots = np.array([[p.open() for _ in range(S)] for p in pools][0], np.int32)
n = np.full(S, B, np.int32)
frames = np.zeros(S, np.int32)
out_host = np.zeros((2, 1 << 16), np.float32)
outp = (fp * 2)(out_host[0].ctypes.data_as(fp), out_host[1].ctypes.data_as(fp))
OUT_PITCH = 2048
out_f32 = torch.zeros((S, 2, OUT_PITCH), dtype=torch.float32, device="cuda")
out_i16 = torch.zeros((S, 2, OUT_PITCH), dtype=torch.int16, device="cuda")
stream = torch.cuda.current_stream().cuda_stream
count = [0, 0, 0]  # calls made per leg (which block comes next)


def check(st, what):
    if st != 0:
        raise SystemExit(f"{what}: {L.pv_last_error().decode()}")


def leg_host(calls):
    p, us = pools[0], []
    for _ in range(calls):
        t = ptrs[count[0] % NBLK]
        count[0] += 1
        t0 = time.perf_counter()
        st = L.pv_pool_feed(p.h, S, slots.ctypes.data, t, n.ctypes.data)
        for j in range(S):
            L.pv_pool_retrieve(p.h, int(slots[j]), outp, L.pv_pool_available(p.h, int(slots[j])))
        us.append((time.perf_counter() - t0) * 1e6)
        check(st, "pv_pool_feed")
    return us


def leg_device(leg, calls):
    p, us = pools[leg], []
    x, out, wire = (dev_f32, out_f32, 0) if leg == 1 else (dev_i16, out_i16, 1)
    for _ in range(calls):
        d = x[count[leg] % NBLK]
        count[leg] += 1
        t0 = time.perf_counter()
        st = L.pv_pool_feed_device(p.h, S, slots.ctypes.data, n.ctypes.data, d.data_ptr(), B, out.data_ptr(), OUT_PITCH,
                                   wire, frames.ctypes.data, stream)
        us.append((time.perf_counter() - t0) * 1e6)
        check(st, "pv_pool_feed_device")
    return us


LEGS = ("host feed + retrieve", "feed_device f32", "feed_device i16")
rate = [[], [], []]
per_call = [[], [], []]
for r in range(-1, args.repeats):  # (-1: the warm-up round, not recorded)
    for leg in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        us = leg_host(args.calls) if leg == 0 else leg_device(leg, args.calls)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if r >= 0:
            rate[leg].append(args.calls / dt)
            per_call[leg] += us
launches = []
for p in pools:
    v = C.c_int32(0)
    L.pv_pool_last_launches(p.h, C.byref(v))
    launches.append(v.value)
    p.close_pool()

lines = [f"{S} live stereo streams, +4 st, fft 2048, phase-locked, {B}-frame calls; {args.repeats} alternating rounds of "
         f"{args.calls} calls per leg after one warm-up round",
         f"{'leg':<22} {'calls/s median':>14} {'min':>9} {'max':>9} {'host us/call median':>20} {'p99':>9} {'launches':>9}"]
res = {}
for leg, name in enumerate(LEGS):
    rt, us = np.array(rate[leg]), np.array(per_call[leg])
    lines.append(f"{name:<22} {np.median(rt):>14.1f} {rt.min():>9.1f} {rt.max():>9.1f} {np.median(us):>20.1f} "
                 f"{np.percentile(us, 99):>9.1f} {launches[leg]:>9d}")
    res[name] = dict(calls_per_s_median=round(float(np.median(rt)), 1), calls_per_s_min=round(float(rt.min()), 1),
                     calls_per_s_max=round(float(rt.max()), 1), host_us_median=round(float(np.median(us)), 1),
                     host_us_p99=round(float(np.percentile(us, 99)), 1), launches_per_call=launches[leg])
lines.append(json.dumps(res))
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
