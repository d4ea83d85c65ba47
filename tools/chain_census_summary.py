#!/usr/bin/env python3
"""Summarise census files written through AUDIOMOD_PV_CHAIN_CENSUS (include/audiomod_pv.h): how many of the 240
instantiations of the fused kernel (4 sets x 60 rungs) were launched, which were not, and the slot-table resampler and
analysis kernels seen.

    AUDIOMOD_PV_CHAIN_CENSUS=$PWD/census.txt python -m pytest tests -q -m gpu
    tools/chain_census_summary.py census.txt [more files: their union]
"""
import collections
import sys

SETS = ("batch", "pool", "pmix", "mb")


def rungs():
    out = []
    for nc in (256, 512, 1024, 2048):
        for core in (-1, 0, 1, 2, 3):
            if core == 3 and nc != 1024:
                continue
            for res in (0, 1):
                for fast in ((0,) if core < 0 else (0, 1)):
                    out.append((nc, core, res, fast))
    return out


def read(paths):
    seen = collections.defaultdict(collections.Counter)
    for path in paths:
        for line in open(path):
            f = line.split()
            if not f:
                continue
            d = dict(kv.split("=") for kv in f[1:])
            count = int(d.pop("count"))
            key = (d.pop("set"),) + tuple(int(v) for v in d.values())
            seen[f[0]][key] += count
    return seen


def main(argv):
    if len(argv) < 2:
        sys.exit(__doc__)
    seen = read(argv[1:])
    want = [(s,) + r for s in SETS for r in rungs()]
    assert len(want) == 240
    hit = [k for k in want if seen["chain"].get(k)]
    print("fused kernel: %d of %d instantiations launched" % (len(hit), len(want)))
    for s in SETS:
        missing = [k[1:] for k in want if k[0] == s and not seen["chain"].get(k)]
        print("  %-5s %2d of 60; not launched (nc, plain_core, res, fast): %s" %
              (s, 60 - len(missing), " ".join("(%d,%d,%d,%d)" % m for m in missing) or "none"))
    unknown = sorted(set(seen["chain"]) - set(want))
    if unknown:
        print("  keys outside the ladder: %s" % unknown)
    print("slot-table resampler (set, fast, interpolated): %s" % " ".join(
        "%s/%d/%d" % k for k in sorted(seen["resample"])))
    print("slot-table analysis (set, nc, split): %s" % " ".join("%s/%d/%d" % k for k in sorted(seen["analyze"])))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
