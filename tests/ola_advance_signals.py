"""The overlap-add advance (a slice's shift increment) from 1 to the FFT size, one row per regime: the table, and what
the oracle says of each row.

The fused synthesis + overlap-add kernel (pv_kernels.hip chain_slice_tail at fft 512 ... 4096, chain_finish_slice at
256 and 8192) adds a frame at P mod (N + 4) of a row's accumulator ring, finalises the `advance` samples behind P and
zeroes them.  What it does depends on
    the advance    which of a lane's quads reach into the finalised region: the two pieces with scalar zero-masks
                   (advances up to 512 - lead), the later pieces with the in-place test; the denominators prefetched for
                   the first 128 quads and loaded late beyond them; at 256 / 8192 the prefix of 4 x 64 samples and the
                   loop behind it, and advances below 64, where most lanes idle
    the lead       P mod (N + 4) mod 4, the ring position within its quad: four instantiations, three of which carry a
                   sample across lanes; the ring wraps where a quad index passes (N + 4) / 4
and the host plans depend on it too (ChainBuilder: the lead quads of the denominators, the warm-up rule of the run lists;
Core::init: the frame ring's look-back, the tile path's limit of frames per tile, the stream ring's size).  The engine's own
hops give advances of N/8 ... N/4 + 1 and, in the fixed-advance modes, leads of 0 only; a caller-chosen hop (hopsize)
reaches everything else.

ROBOTIC has a fixed advance equal to the hop and is bit for bit end to end, so those rows are held with no tolerance;
the plain rows follow the reference's increment recurrence (next_increment).  An advance of exactly N leaves the window sum
under a frame's first sample at 0: the reference divides by it and emits non-finite samples there, and so does the engine.
Above N the reference's behaviour is undefined (OracleUndefined) and every form refuses.

FIGURES holds, per row, what the oracle gave: (slices, the set of advances, the histogram of leads, ring wraps,
non-finite output samples[, dropped slices, their leads]).  tests/test_ola_advance_host.py checks every literal against the
oracle; tests/test_ola_advance_gpu.py runs the rows through every engine form."""
import collections
import functools

import numpy as np

from audiomod_amd import signals
from oracle import oracle_py as O

BLOCK = 480
UNDEFINED = "undefined"          # the reference overruns its accumulators: nothing to be on par with
ENGINE_REFUSES = "engine refuses"  # the oracle runs it; the engine refuses at creation, with a reason

Row = collections.namedtuple("Row", "name cfg channels frames block kind")


def _rob(fft, hop, frames, channels=2):
    return Row(f"rob{fft}_h{hop}", dict(mode="robotic", fftsize=fft, hopsize=hop), channels, frames, BLOCK, "robotic")


def _plain(name, frames, kind="plain", **cfg):
    return Row(name, cfg, 2, frames, BLOCK, kind)


ROBOTIC_ROWS = (
    [_rob(512, h, 4000) for h in (1, 2, 3, 5, 6, 7)]   # (6 | 7: the tile path's limit of frames per tile, Core::init)
    + [_rob(512, h, 8000) for h in (63, 64, 65, 255, 256, 257, 507, 508, 509, 511, 512)]
    + [_rob(1024, h, 12000) for h in (253, 509, 512, 515, 765, 769, 1021, 1023, 1024)]
    + [_rob(2048, h, 30000) for h in (2045, 2047, 2048)]
    + [_rob(4096, 4093, 50000)]
    + [_rob(256, 1, 3000), _rob(256, 255, 4000), _rob(256, 256, 4000)]
    + [_rob(8192, 8189, 60000, channels=1)]
)
# calls so large that the reference's output ring (16 N samples) overruns: it drops slices there (advance 0, the frames
# pile up on one position), as tests/test_gpu_parity.py OVERRUN_GPU has it; odd hops, so that they pile up at every lead
OVERRUN_ROWS = [
    Row("rob512_h5_overrun", dict(mode="robotic", fftsize=512, hopsize=5), 2, 27000, 9000, "robotic"),
    Row("rob512_h3_overrun", dict(mode="robotic", fftsize=512, hopsize=3), 2, 26500, 8833, "robotic"),
]
SHIFT = dict(mode="normal_pitchshift")
STRETCH = dict(mode="time_stretch")
PLAIN_ROWS = [
    _plain("p512_+4_h2", 4000, fftsize=512, semitones=4.0, hopsize=2, **SHIFT),
    _plain("p512_-24_h8", 4000, fftsize=512, semitones=-24.0, hopsize=8, **SHIFT),
    _plain("s512_0.3_h8_core1", 4000, fftsize=512, time_ratio=0.3, hopsize=8, coremode=1, **STRETCH),
    _plain("s512_0.3_h8_core0", 4000, fftsize=512, time_ratio=0.3, hopsize=8, coremode=0, **STRETCH),
    _plain("p1024_+7_h340", 16000, fftsize=1024, semitones=7.0, hopsize=340, **SHIFT),
    _plain("p2048_+7_h1020", 40000, fftsize=2048, semitones=7.0, hopsize=1020, **SHIFT),
    _plain("p2048_+4_h1621", 40000, fftsize=2048, semitones=4.0, hopsize=1621, **SHIFT),
    _plain("p1024_+12_h511", 16000, fftsize=1024, semitones=12.0, hopsize=511, **SHIFT),
    _plain("p1024_+12_h512", 16000, fftsize=1024, semitones=12.0, hopsize=512, **SHIFT),
    _plain("p512_+4_h406", 12000, fftsize=512, semitones=4.0, hopsize=406, **SHIFT),
    _plain("s512_1.5_h341_core2", 12000, fftsize=512, time_ratio=1.5, hopsize=341, coremode=2, **STRETCH),
    _plain("s512_1.5_h340_core0", 12000, fftsize=512, time_ratio=1.5, hopsize=340, coremode=0, **STRETCH),
    _plain("g512_-7_h300", 12000, fftsize=512, semitones=-7.0, hopsize=300, mode="gender_change"),
    _plain("s2048_1.5_h1360", 40000, fftsize=2048, time_ratio=1.5, hopsize=1360, **STRETCH),
]
UNDEFINED_ROWS = [
    Row("rob512_h513", dict(mode="robotic", fftsize=512, hopsize=513), 2, 8000, BLOCK, UNDEFINED),
    _plain("p512_+4_h407", 12000, kind=UNDEFINED, fftsize=512, semitones=4.0, hopsize=407, **SHIFT),
]
# lrint(hop x ratio / 2) = 0: the reference runs it (every advance 1); derive() refuses it, with a reason
REFUSED_ROWS = [_plain("p512_-24_h4", 4000, kind=ENGINE_REFUSES, fftsize=512, semitones=-24.0, hopsize=4, **SHIFT)]

ROWS = ROBOTIC_ROWS + OVERRUN_ROWS + PLAIN_ROWS + UNDEFINED_ROWS + REFUSED_ROWS
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
DEFINED = [r.name for r in ROWS if r.kind != UNDEFINED]                 # the oracle runs them
SERVED = [r.name for r in ROWS if r.kind in ("robotic", "plain")]       # ... and so does the engine
OVERRUN = [r.name for r in OVERRUN_ROWS]

# name: (slices, advances, (leads 0..3), ring wraps, non-finite samples[, dropped slices, (their leads)])
FIGURES = {
    "rob512_h1": (4417, (1,), (1105, 1104, 1104, 1104), 8, 0),
    "rob512_h2": (2209, (2,), (1105, 0, 1104, 0), 8, 0),
    "rob512_h3": (1473, (3,), (369, 368, 368, 368), 8, 0),
    "rob512_h5": (885, (5,), (222, 221, 221, 221), 8, 0),
    "rob512_h6": (737, (6,), (369, 0, 368, 0), 8, 0),
    "rob512_h7": (632, (7,), (158, 158, 158, 158), 8, 0),
    "rob512_h63": (127, (63,), (32, 31, 32, 32), 15, 0),
    "rob512_h64": (125, (64,), (125, 0, 0, 0), 15, 0),
    "rob512_h65": (124, (65,), (31, 31, 31, 31), 15, 0),
    "rob512_h255": (33, (255,), (9, 8, 8, 8), 16, 0),
    "rob512_h256": (32, (256,), (32, 0, 0, 0), 15, 0),
    "rob512_h257": (32, (257,), (8, 8, 8, 8), 15, 0),
    "rob512_h507": (16, (507,), (4, 4, 4, 4), 15, 0),
    "rob512_h508": (16, (508,), (16, 0, 0, 0), 15, 0),
    "rob512_h509": (16, (509,), (4, 4, 4, 4), 15, 0),
    "rob512_h511": (16, (511,), (4, 4, 4, 4), 15, 0),
    "rob512_h512": (16, (512,), (16, 0, 0, 0), 15, 30),
    "rob1024_h253": (48, (253,), (12, 12, 12, 12), 11, 0),
    "rob1024_h509": (24, (509,), (6, 6, 6, 6), 11, 0),
    "rob1024_h512": (24, (512,), (24, 0, 0, 0), 11, 0),
    "rob1024_h515": (24, (515,), (6, 6, 6, 6), 12, 0),
    "rob1024_h765": (16, (765,), (4, 4, 4, 4), 11, 0),
    "rob1024_h769": (16, (769,), (4, 4, 4, 4), 11, 0),
    "rob1024_h1021": (12, (1021,), (3, 3, 3, 3), 11, 0),
    "rob1024_h1023": (12, (1023,), (3, 3, 3, 3), 11, 0),
    "rob1024_h1024": (12, (1024,), (12, 0, 0, 0), 11, 22),
    "rob2048_h2045": (15, (2045,), (4, 4, 4, 3), 14, 0),
    "rob2048_h2047": (15, (2047,), (4, 3, 4, 4), 14, 0),
    "rob2048_h2048": (15, (2048,), (15, 0, 0, 0), 14, 28),
    "rob4096_h4093": (13, (4093,), (4, 3, 3, 3), 12, 0),
    "rob256_h1": (3449, (1,), (863, 862, 862, 862), 13, 0),
    "rob256_h255": (17, (255,), (5, 4, 4, 4), 16, 0),
    "rob256_h256": (17, (256,), (17, 0, 0, 0), 16, 30),
    "rob8192_h8189": (8, (8189,), (2, 2, 2, 2), 7, 0),
    "rob512_h5_overrun": (6997, (5,), (1628, 1790, 1628, 1951), 63, 0, 486, (0, 162, 0, 324)),
    "rob512_h3_overrun": (11438, (3,), (2913, 2912, 2914, 2699), 62, 0, 643, (214, 214, 215, 0)),
    "p512_+4_h2": (2209, (2, 3), (551, 554, 553, 551), 10, 0),
    "p512_-24_h8": (553, (2,), (277, 0, 276, 0), 2, 0),
    "s512_0.3_h8_core1": (1693, (2, 3), (384, 309, 383, 617), 7, 0),
    "s512_0.3_h8_core0": (1693, (2, 3), (384, 309, 383, 617), 7, 0),
    "p1024_+7_h340": (48, (509, 510), (11, 13, 12, 12), 23, 0),
    "p2048_+7_h1020": (40, (1528, 1529), (13, 11, 9, 7), 29, 0),
    "p2048_+4_h1621": (25, (2042, 2043), (7, 6, 6, 6), 24, 0),
    "p1024_+12_h511": (32, (1022,), (16, 0, 16, 0), 31, 0),
    "p1024_+12_h512": (32, (1024,), (32, 0, 0, 0), 31, 3968),
    "p512_+4_h406": (30, (511, 512), (8, 8, 6, 8), 29, 2046),
    "s512_1.5_h341_core2": (34, (511, 512), (10, 8, 8, 8), 33, 34),
    "s512_1.5_h340_core0": (34, (510,), (17, 0, 17, 0), 33, 0),
    "g512_-7_h300": (41, (200, 201), (26, 6, 5, 4), 15, 0),
    "s2048_1.5_h1360": (28, (2040,), (28, 0, 0, 0), 27, 0),
    "p512_-24_h4": (1105, (1,), (277, 276, 276, 276), 2, 0),
}


def fft_of(name):
    return BY_NAME[name].cfg["fftsize"]


def config(name):
    """the row's configuration as the keyword arguments of oracle_py.Oracle / engine.make_config (without channels)"""
    return dict(BY_NAME[name].cfg)


@functools.lru_cache(maxsize=None)
def clip(name, stream=0):
    """stream 0 is signals.voice(frames, 2, seed=3); the other streams of a batch differ by their seed"""
    r = BY_NAME[name]
    x = np.ascontiguousarray(signals.voice(r.frames, 2, seed=3 + 17 * stream)[:r.channels])
    x.setflags(write=False)
    return x


def call_list(name, ncalls):
    """the sizes of the offline loop's calls: the clip in blocks, then whole zero blocks (the flush)"""
    r = BY_NAME[name]
    calls = [min(r.block, r.frames - i) for i in range(0, r.frames, r.block)]
    return calls + [r.block] * (ncalls - len(calls))


Run = collections.namedtuple("Run", "y counts info shift slices_per_call")


@functools.lru_cache(maxsize=None)
def oracle(name, stream=0):
    """The row's clip through the oracle in the reference's offline loop (blocks of the row's size, then zero blocks
    until the clip's length has come out): output, per-call counts, info, the shift increment of every slice and the
    number of slices each call made.  Raises O.OracleUndefined for an UNDEFINED row."""
    r = BY_NAME[name]
    x = clip(name, stream)
    o = O.Oracle(r.channels, **r.cfg)
    outs, counts, per_call, produced, seen = [], [], [], 0, 0

    def call(blk, limit):
        nonlocal produced, seen
        got = o.process(blk)
        y = o.retrieve(got)
        counts.append(got)
        n = len(o.increments()[0])
        per_call.append(n - seen)
        seen = n
        w = got if limit is None or limit - produced > got else limit - produced
        outs.append(y[:, :w])
        produced += w

    try:
        for i in range(0, r.frames, r.block):
            call(x[:, i:i + r.block], None)
        z = np.zeros((r.channels, r.block), np.float32)
        while produced < r.frames:
            call(z, r.frames)
        shift = o.increments()[0].copy()
        info = o.info()
    finally:
        o.close()
    y = np.concatenate(outs, axis=1)
    y.setflags(write=False)
    shift.setflags(write=False)
    return Run(y, tuple(counts), info, shift, tuple(per_call))


def advances(name, stream=0):
    """(advance, P) per slice from the oracle's record: the advance is the shift increment, or 0 for a slice the
    reference dropped because its output ring was full; P is the sum of the advances before it.  Nothing is read
    within a call, so a call's ring, once too full, stays so: the slices it emits come first -- without resampling
    their increments sum to the call's count -- and the rest are dropped."""
    run = oracle(name, stream)
    adv = np.array(run.shift, dtype=np.int64)
    if name in OVERRUN:
        assert not run.info["resample"]
        t = 0
        for n, got in zip(run.slices_per_call, run.counts):
            c = np.cumsum(adv[t:t + n])
            k = int(np.searchsorted(c, got, side="right"))
            assert (c[k - 1] if k else 0) == got, (name, got)
            adv[t + k:t + n] = 0
            t += n
    P = np.concatenate([[0], np.cumsum(adv)[:-1]]) if len(adv) else adv
    return adv, P


def figures(name, stream=0):
    """what FIGURES holds for the row, computed from the oracle"""
    run = oracle(name, stream)
    adv, P = advances(name, stream)
    AR = fft_of(name) + 4
    live = adv[adv > 0]
    lead = (P % AR) % 4
    leads = tuple(int(np.count_nonzero(lead == k)) for k in range(4))
    wraps = int((P[-1] + adv[-1]) // AR)
    bad = int(np.count_nonzero(~np.isfinite(run.y)))
    out = (len(adv), tuple(sorted({int(a) for a in live})), leads, wraps, bad)
    if name in OVERRUN:
        dl = lead[adv == 0]
        out += (int(np.count_nonzero(adv == 0)), tuple(int(np.count_nonzero(dl == k)) for k in range(4)))
    return out
