#!/usr/bin/env python3
"""Stream-pool snapshots: what a save and a restore cost.  Stereo streams, fft 2048, +4 st, phase-locked, 480-frame
calls; two pools of 128 slots in one process, every slot of the first one live and warmed up with --warm calls.
Per round, for S = 1 and S = 128 slots:
  save     wall time of pv_pool_save of S slots into preallocated host blobs (one kernel, one copy, the wait included);
  restore  wall time of pv_pool_restore of those blobs into the second pool (its slots are closed again afterwards);
  feed     a pv_pool_feed of the S restored slots right after the restore, against the same feed of the S source slots
           in the first pool (a "normal" feed), both 480 frames per slot.
--repeats rounds (default five) after one warm-up round; prints median and range, blob bytes per slot and one JSON line;
--out FILE writes the same there.   python tools/pool_snapshot_bench.py [--repeats 5] [--out profiles/r12/pool_snapshot.txt]"""
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
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warm", type=int, default=40)
ap.add_argument("--out", default=None)
args = ap.parse_args()
CAP, B, SR = 128, 480, 48000
kw = dict(semitones=4.0, coremode=1, fftsize=2048)
L = E.lib()
fp = C.POINTER(C.c_float)
src = signals.voice(SR, 2)


def check(st, what):
    if st != 0:
        raise SystemExit(f"{what}: {L.pv_last_error().decode()}")


A, Bp = E.StreamPool(CAP, channels=2, **kw), E.StreamPool(CAP, channels=2, **kw)
slots_a = np.array([A.open() for _ in range(CAP)], np.int32)
n = np.full(CAP, B, np.int32)
blocks = np.ascontiguousarray(np.stack([src[:, (97 * j) % (SR - B):][:, :B] for j in range(CAP)]), np.float32)
rows = (fp * (2 * CAP))(*[blocks[j, c].ctypes.data_as(fp) for j in range(CAP) for c in range(2)])
sink = np.zeros((2, 1 << 16), np.float32)
sinkp = (fp * 2)(sink[0].ctypes.data_as(fp), sink[1].ctypes.data_as(fp))


def feed(pool, slots):
    """one 480-frame feed of `slots` (everything retrieved afterwards, untimed); returns its wall time in us"""
    t0 = time.perf_counter()
    st = L.pv_pool_feed(pool.h, len(slots), slots.ctypes.data, rows, n.ctypes.data)
    dt = (time.perf_counter() - t0) * 1e6
    check(st, "pv_pool_feed")
    for s in slots:
        L.pv_pool_retrieve(pool.h, int(s), sinkp, L.pv_pool_available(pool.h, int(s)))
    return dt


for _ in range(args.warm):
    feed(A, slots_a)
size = int(L.pv_pool_snapshot_bytes(A.h, 0))
bufs = [np.empty(size, np.uint8) for _ in range(CAP)]
ptrs = (C.c_void_p * CAP)(*[b.ctypes.data for b in bufs])
caps = np.full(CAP, size, np.int64)
got = np.zeros(CAP, np.int64)
new = np.zeros(CAP, np.int32)
res = {}
for S in (1, CAP):
    t = dict(save=[], restore=[], feed_after_restore=[], feed_normal=[])
    for r in range(-1, args.repeats):  # (-1: warm-up, not recorded; it also grows the staging buffers)
        t0 = time.perf_counter()
        st = L.pv_pool_save(A.h, S, slots_a.ctypes.data, ptrs, caps.ctypes.data, got.ctypes.data)
        t_save = (time.perf_counter() - t0) * 1e6
        check(st, "pv_pool_save")
        t0 = time.perf_counter()
        st = L.pv_pool_restore(Bp.h, S, ptrs, got.ctypes.data, new.ctypes.data)
        t_restore = (time.perf_counter() - t0) * 1e6
        check(st, "pv_pool_restore")
        t_after = feed(Bp, new[:S])
        t_normal = feed(A, slots_a[:S])
        for s in new[:S]:
            Bp.close(int(s))
        if r >= 0:
            t["save"].append(t_save), t["restore"].append(t_restore)
            t["feed_after_restore"].append(t_after), t["feed_normal"].append(t_normal)
    res[S] = {k: dict(median_us=round(float(np.median(v)), 1), min_us=round(float(min(v)), 1),
                      max_us=round(float(max(v)), 1)) for k, v in t.items()}
info = E.blob_info(bufs[0][:int(got[0])].tobytes())
lines = [f"stream-pool snapshots: stereo, fft 2048, +4 st, phase-locked; pools of {CAP} slots, {args.warm} warm-up calls of "
         f"{B} frames; {args.repeats} rounds after one warm-up round",
         f"blob: {int(got[0])} bytes per slot ({info['payload_bytes']} of device rows, {info['pending_frames']} frames pending)",
         f"{'slots':>5} {'what':<20} {'median us':>10} {'min':>10} {'max':>10}"]
for S in (1, CAP):
    for k, v in res[S].items():
        lines.append(f"{S:>5} {k:<20} {v['median_us']:>10.1f} {v['min_us']:>10.1f} {v['max_us']:>10.1f}")
lines.append(json.dumps(dict(blob_bytes=int(got[0]), payload_bytes=info["payload_bytes"],
                             results={str(k): v for k, v in res.items()})))
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
A.close_pool(), Bp.close_pool()
