#!/usr/bin/env python3
"""The carrier setting: what a pool of vocoder voices costs against the same pool robotic, and whether the robotic pool
is as fast as it was (fft 2048, stereo, mode robotic, pitch 0; 128 slots, 480-frame pv_pool_feed calls).
  carrier  every slot with carrier ROSENBERG
  robotic  every slot robotic
  parent   the robotic leg on a library built from the parent commit (--parent-lib FILE: run in a second process that
           loads it through AUDIOMOD_PV_LIB; without the option the leg is reported as not measured)
One run: each leg is one worker process that keeps its pool; the legs alternate, --repeats rounds (default five)
after a warm-up round, a round being the median of --feeds calls.  Per leg: wall time per call (its wait included), the
host time up to the wait (pv_pool_last_timing) and the kernels launched.  Also times 128 x 480 host cosf calls, the
work per feed that 128 round-robin vocoder engines spend on their carriers.  Prints median and range per leg and one
JSON line; --out FILE appends the same there.
  python tools/carrier_bench.py [--repeats 5] [--parent-lib /path/libaudiomod_pv.so] [--out profiles/r21/carrier.txt]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--feeds", type=int, default=100)
ap.add_argument("--warm", type=int, default=40)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--worker", default=None, help="internal: serve the legs named here (comma-separated) over stdin/stdout")
args = ap.parse_args()
CAP, B, SR = 128, 480, 48000


def stat(v):
    return dict(median=round(float(np.median(v)), 3), min=round(float(min(v)), 3), max=round(float(max(v)), 3))


def worker(legs):
    from audiomod_amd import engine as E, signals
    if E.lib().pv_device_count() < 1:
        raise SystemExit("carrier_bench: no gfx950 device visible (there is no CPU fallback: nothing is measured)")
    L = E.lib()
    fp = C.POINTER(C.c_float)
    src = signals.voice(SR, 2)
    pools, slots = {}, {}
    for leg in legs:
        pools[leg] = E.StreamPool(CAP, channels=2, mode="robotic", fftsize=2048)
        slots[leg] = np.array([pools[leg].open() for _ in range(CAP)], np.int32)
        if leg == "carrier":
            for s in slots[leg]:
                pools[leg].set_carrier(int(s), "rosenberg")
    n = np.full(CAP, B, np.int32)
    blocks = np.ascontiguousarray(np.stack([src[:, (97 * j) % (SR - B):][:, :B] for j in range(CAP)]), np.float32)
    rows = (fp * (2 * CAP))(*[blocks[j, c].ctypes.data_as(fp) for j in range(CAP) for c in range(2)])
    sink = np.zeros((2, 1 << 16), np.float32)
    sinkp = (fp * 2)(sink[0].ctypes.data_as(fp), sink[1].ctypes.data_as(fp))

    def feed(leg):
        pool, sl = pools[leg], slots[leg]
        t0 = time.perf_counter()
        st = L.pv_pool_feed(pool.h, len(sl), sl.ctypes.data, rows, n.ctypes.data)
        dt = (time.perf_counter() - t0) * 1e6
        if st != 0:
            raise SystemExit(f"pv_pool_feed: {L.pv_last_error().decode()}")
        host_us, launches = pool.last_timing()[0], pool.last_launches()
        for s in sl:
            L.pv_pool_retrieve(pool.h, int(s), sinkp, L.pv_pool_available(pool.h, int(s)))
        return dt, host_us, launches

    print("ready", flush=True)
    for line in sys.stdin:
        leg, feeds = line.split()
        v = [feed(leg) for _ in range(int(feeds))]
        print(json.dumps(dict(us=float(np.median([x[0] for x in v])), host_us=float(np.median([x[1] for x in v])),
                              launches=max(x[2] for x in v))), flush=True)


if args.worker:
    worker(args.worker.split(","))
    sys.exit(0)


def start(legs, lib=None):
    env = dict(os.environ)
    if lib:
        env["AUDIOMOD_PV_LIB"] = lib
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", ",".join(legs)], stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True, env=env)
    if p.stdout.readline().strip() != "ready":
        raise SystemExit("carrier_bench: a worker did not start")
    return p


def ask(p, leg, feeds):
    p.stdin.write(f"{leg} {feeds}\n")
    p.stdin.flush()
    line = p.stdout.readline()
    if not line:
        raise SystemExit("carrier_bench: a worker ended early")
    return json.loads(line)


procs = {"carrier": start(["carrier"]), "robotic": start(["robotic"])}  # (a process per leg: all legs alike)
legs = [("carrier", "carrier"), ("robotic", "robotic")]
if args.parent_lib:
    procs["parent"] = start(["robotic"], os.path.abspath(args.parent_lib))
    legs.append(("parent", "robotic"))
for name, leg in legs:
    ask(procs[name], leg, args.warm)
us, host_us, launches = ({name: [] for name, _ in legs} for _ in range(3))
for r in range(-1, args.repeats):  # (-1: warm-up round, not recorded)
    for name, leg in legs if r % 2 == 0 else legs[::-1]:
        v = ask(procs[name], leg, args.feeds)
        if r >= 0:
            us[name].append(v["us"]), host_us[name].append(v["host_us"]), launches[name].append(v["launches"])
for p in set(procs.values()):
    p.stdin.close()
    p.wait()

# the host work the closed form replaces: one cosf per carrier sample and engine (CarrierGen::next), 128 x 480 per feed
# (timed through pv_plan_table, which runs CarrierGen for that many samples)
from audiomod_amd import engine as E  # noqa: E402  (host only here: pv_plan_table runs CarrierGen)
cos_us = []
E.plan_table(2, max_len=CAP * B, channels=2, mode="vocoder")  # (untimed: loads the library)
for _ in range(args.repeats):
    t0 = time.perf_counter()
    E.plan_table(2, max_len=CAP * B, channels=2, mode="vocoder")
    cos_us.append((time.perf_counter() - t0) * 1e6)

res = dict(feed_us={k: stat(v) for k, v in us.items()}, host_us={k: stat(v) for k, v in host_us.items()},
           launches={k: max(v) for k, v in launches.items()}, carriergen_128x480_us=stat(cos_us))
if "parent" in us:
    a, b = res["feed_us"]["robotic"], res["feed_us"]["parent"]
    res["robotic_ranges_overlap"] = bool(a["min"] <= b["max"] and b["min"] <= a["max"])
res["carrier_extra_host_us"] = round(res["host_us"]["carrier"]["median"] - res["host_us"]["robotic"]["median"], 3)
lines = [f"carrier setting, speed: mode robotic, fft 2048, stereo, pitch 0; {CAP} slots, {B}-frame pv_pool_feed calls; "
         f"{args.repeats} rounds after one warm-up round, legs alternating (a round: median of {args.feeds} calls)",
         f"{'what':<40} {'median':>10} {'min':>10} {'max':>10} {'launches':>9}"]
for name, _ in legs:
    v, h = res["feed_us"][name], res["host_us"][name]
    lines.append(f"{'pool feed, ' + name + ' (us)':<40} {v['median']:>10.1f} {v['min']:>10.1f} {v['max']:>10.1f} {res['launches'][name]:>9}")
    lines.append(f"{'  its host part (us)':<40} {h['median']:>10.1f} {h['min']:>10.1f} {h['max']:>10.1f}")
if not args.parent_lib:
    lines.append("pool feed, parent: not measured (python tools/carrier_bench.py --parent-lib <library built from the parent commit>)")
v = res["carriergen_128x480_us"]
lines.append(f"{'CarrierGen, 128 x 480 samples, host (us)':<40} {v['median']:>10.1f} {v['min']:>10.1f} {v['max']:>10.1f}")
lines.append(f"carrier leg's extra host time per feed: {res['carrier_extra_host_us']:.1f} us")
lines.append(json.dumps(res))
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")
