#!/usr/bin/env python3
"""Host-staged throughput: staging by stream (groups) against staging by time (segments), on the bench workload.

128 stereo streams x 60 s, +4 semitones, fft 2048 (bench.py's flagship), input and output in page-locked host memory.
Variants: the grouped object at 32 streams per group, and the segmented object (pv_hostio_create_segmented) at 1, 2, 4
and 8 launches per segment; float32 and int16 on the wire.  All variants live in one process and alternate: each is
warmed up once, then the timed rounds go round-robin over them, so drift of the machine hits all alike.  A run is
synchronous (pv_hostio_run returns when host_out is complete), so the time is a host clock around it.  Every output is
compared with the device-resident batch's (int16: with the reference's WAV writer applied to it).

    python tools/hostio_span_bench.py [--streams 128] [--seconds 60] [--rounds 3] [--out profiles/r06/hostio_spans]

Writes <out>.txt and <out>.json: G samples/s and GB/s each way per variant, the median of the rounds."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=128)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--group", type=int, default=32, help="streams per group of the grouped variant")
    ap.add_argument("--segments", type=int, nargs="*", default=[1, 2, 4, 8], help="launches per segment to try")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06", "hostio_spans"))
    args = ap.parse_args()

    import torch

    from audiomod_amd import engine as E
    from audiomod_amd import signals

    S, F = args.streams, args.seconds * 48000
    kw = dict(semitones=4.0, coremode=1, fftsize=2048)
    dev = torch.device("cuda:0")
    d_in = signals.synthetic_batch(torch, S, F, dev)
    batch = E.Batch(S, F, channels=2, block=480, flush=True, **kw)
    ref = batch.run(d_in)
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    launches = batch.launches
    batch.close()
    x = d_in.cpu().numpy()
    del d_in
    torch.cuda.empty_cache()
    want = {"f32": ref, "i16": np.trunc(np.clip(ref * np.float32(32768.0), -32768.0, 32767.0)).astype(np.int16)}
    wire_in = {"f32": x, "i16": np.round(x * 32768.0).astype(np.int16)}  # the inputs sit on the int16 grid: exact

    variants = [("grouped_%d" % args.group, dict(streams_per_group=args.group))]
    variants += [("segmented_%d" % k, dict(launches_per_segment=k)) for k in args.segments]
    results = []
    for wire in ("f32", "i16"):
        objs = []
        for name, arg in variants:
            h = E.HostIO(S, F, channels=2, block=480, flush=True, wire=wire, **arg, **kw)
            objs.append((name, h))
        hin = objs[0][1].pinned((S, 2, F))
        hout = objs[0][1].pinned((S, 2, objs[0][1].out_frames))
        hin[...] = wire_in[wire]
        times = {name: [] for name, _ in objs}
        same = {}
        for name, h in objs:                      # warm-up, and the equality check
            hout.view(np.uint8)[...] = 0xA5
            h.run(hin, hout)
            same[name] = bool(np.array_equal(hout, want[wire]) if wire == "i16"
                              else np.array_equal(hout.view(np.uint32), want[wire].view(np.uint32)))
        for _ in range(args.rounds):              # the variants alternate inside each round
            for name, h in objs:
                t0 = time.perf_counter()
                h.run(hin, hout)
                times[name].append(time.perf_counter() - t0)
        for name, h in objs:
            dt = statistics.median(times[name])
            results.append(dict(wire=wire, variant=name, ms_per_step=round(dt * 1e3, 2),
                                Gsamples_s=round(S * 2 * F / dt / 1e9, 2),
                                pcie_GBps_each_way=round(S * 2 * F * hin.itemsize / dt / 1e9, 2),
                                staging_MB=round(h.staging_bytes() / 1e6, 1), rounds_ms=[round(t * 1e3, 2) for t in times[name]],
                                equals_device_resident_output=same[name]))
        for _, h in objs[1:]:
            h.close()
        objs[0][1].close()

    head = dict(streams=S, seconds=args.seconds, launches=launches, rounds=args.rounds, config=kw,
                device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out + ".json", "w") as f:
        json.dump(dict(head, results=results), f, indent=1)
    lines = ["host-staged throughput, %d stereo streams x %d s, +4 st, fft 2048 (%d launches per batch run); median of %d "
             "alternating rounds after a warm-up; %s" % (S, args.seconds, launches, args.rounds, head["device"]),
             "%-5s %-14s %10s %12s %14s %11s %s" % ("wire", "variant", "ms/step", "G samples/s", "GB/s each way",
                                                     "staging MB", "equals device-resident")]
    for r in results:
        lines.append("%-5s %-14s %10.2f %12.2f %14.2f %11.1f %s" % (r["wire"], r["variant"], r["ms_per_step"], r["Gsamples_s"],
                                                                  r["pcie_GBps_each_way"], r["staging_MB"],
                                                                  r["equals_device_resident_output"]))
    with open(args.out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if all(r["equals_device_resident_output"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
