"""Inputs that put the analysis kernels where the plane tests want them, and what the oracle's plane trace says of them.

Every case is a list of mono streams (float32 [1, frames] each) and a configuration.  tests/test_analysis_planes_host.py
asserts on the oracle's plane trace (oracle_py.Oracle.plane_trace) that each case reaches its situation;
tests/test_analysis_planes_gpu.py compares the device's planes of the same streams with that trace, bit for bit.

Levels.  The wave-per-frame kernels convert a pass of 256 bins (four per lane) with the short division and square root
when every component of the pass lies in [2^-48, 2^63), and with the IEEE operations otherwise (pv_kernels.hip
analyze_wave_role / analyze_split_role; the DC slot holds (1, 1) there and is in range by construction).  The level
cases are signals.voice times a power of two, which is exact in float32:
    ordinary    as it comes: every pass of every frame with sound in it is in range
    mixed       some passes in range, some with a few components below 2^-48
    out         every bin but the parked DC one below 2^-48
    subnormal   re^2 + im^2 subnormal in float32 for many bins: magnitudes lose bits, and the peak lists change
    zero        re^2 + im^2 underflows to 0 everywhere: no magnitude, no peak, per-bin steps throughout
    loud        the largest component in [2^63, 2^63.4): a pass out of range at the top, everything still finite
    dc          ordinary level on a DC offset
    holes       ordinary level with exact zeros over part of the stream: silent and partly silent frames
"""
import collections
import functools

import numpy as np

from audiomod_amd import signals
from oracle import oracle_py as O
from tests import phase_signals as S

BLOCK = 480
SHIFT = dict(mode="normal_pitchshift", semitones=4.0, coremode=1)
STRETCH = dict(mode="time_stretch", time_ratio=1.5, coremode=1)
FFTS = (256, 512, 1024, 2048, 4096, 8192)
LO, HI = np.float32(2.0 ** -48), np.float32(2.0 ** 63)   # the range test's bounds


def frames_of(fft):
    return 12000 if fft <= 2048 else 24000 if fft == 4096 else 40000


Case = collections.namedtuple("Case", "name fft cfg make")


def _pair(f):
    """two streams: the signal and its negative (the same magnitudes, every phase half a turn away)"""
    def make():
        x = f()
        return [x, -x]
    return make


def _voice(fft, exp2=0, offset=0.0, hole=False, stream=0, factor=1.0):
    def make():
        scale = factor * 2.0 ** exp2
        x = signals.voice(frames_of(fft), 1, stream=stream).astype(np.float64)
        if offset:
            x = x * 0.5 + offset
        if hole:
            x = holed(x, fft)
        y = (x * scale).astype(np.float32)
        assert np.array_equal(y.astype(np.float64), x * scale)   # the scaling is exact
        return y
    return make


def holed(x, fft):
    """tests/test_phase_forms_host.py's _holed with the hole sized by the frame: exact zeros over two frames and a half
    from a quarter of the stream on, so some frames are all zeros and the ones around them partly"""
    x = x.copy()
    start = x.shape[1] // 4
    x[:, start:start + 2 * fft + fft // 2] = 0.0
    return x


# 2^exp2 per fft size, calibrated on the trace: the voice's largest component is about 2^3.3 at 256 points and doubles
# with the frame.  OUT puts it below 2^-48, LOUD -- with a factor 9/8, still exact on the int16 grid -- at 2^63.1 ... 63.3.
EXP_MIXED, EXP_SUB, EXP_ZERO = -36, -70, -100
EXP_OUT = {256: -53, 512: -54, 1024: -55, 2048: -56, 4096: -57, 8192: -58}
EXP_LOUD = {256: (60, 1.0), 512: (59, 1.125), 1024: (58, 1.125), 2048: (57, 1.125), 4096: (56, 1.125), 8192: (55, 1.125)}


def tones(fft, bins, frames=None, amp=None, seed=0):
    """Cosines of equal amplitude at the centres of `bins` of an fft-point frame, seeded phases, on the int16 grid: a
    Hann frame of a bin-centred tone is its bin and half of it either side, so tones three bins apart are two peaks."""
    frames = frames_of(fft) if frames is None else frames
    rng = np.random.default_rng(seed + fft)
    n = np.arange(fft, dtype=np.int64)
    bins = np.asarray(bins, dtype=np.int64)
    ph = rng.uniform(0.0, 2 * np.pi, bins.size)
    period = np.cos((2 * np.pi / fft) * ((bins[:, None] * n[None, :]) % fft) + ph[:, None]).sum(axis=0)
    x = np.tile(period, frames // fft + 1)[:frames]
    amp = 0.9 / np.max(np.abs(period)) if amp is None else amp
    return S._grid((x * amp)[None, :])


def corner_bins(fft):
    """the peak search's corners: the first and last admissible bins; a pair 4k, 4k + 3 in one lane's run of four, in
    the last lane of a pass with the next peak in the pass behind it, and in mid-pass; at 4096 points the same where
    the split kernel's two waves meet"""
    hs = fft // 2
    b = [2, hs - 3]
    if hs >= 512:
        b += [252, 255, 258, 300, 303, 306]
    else:   # (one pass or less: a pair in mid-pass only)
        b += [60, 63, 66]
    if hs >= 2048:
        b += [1020, 1023, 1026, 1029]
    return sorted(b)


def outer_bins(fft):
    """maxima where no peak is looked for: bins 1 and hs - 2 (and two ordinary tones between them)"""
    hs = fft // 2
    return [1, hs // 2, hs // 2 + 3, hs - 2]


def _outer_dc_nyquist(fft):
    """a DC level and a line at half the sample rate: maxima at bins 0 and hs"""
    def make():
        n = np.arange(frames_of(fft))
        return S._grid((0.25 + 0.25 * np.where(n % 2 == 0, 1.0, -1.0) + 0.1 * tones(fft, [fft // 4], amp=1.0)[0])[None, :])
    return make


def _single(fft):
    """one line at a quarter of the sample rate, with a hole: steps with exactly one peak, and with none"""
    return lambda: holed(S.quarter(frames_of(fft), 1), fft)


def _comb(fft):
    return lambda: S.comb(fft, frames_of(fft), 1, seed=fft)


def _level_cases(fft):
    return [
        Case(f"ordinary_{fft}", fft, SHIFT, _pair(_voice(fft))),
        Case(f"mixed_{fft}", fft, SHIFT, _pair(_voice(fft, EXP_MIXED))),
        Case(f"out_{fft}", fft, SHIFT, _pair(_voice(fft, EXP_OUT[fft]))),
        Case(f"subnormal_{fft}", fft, SHIFT, _pair(_voice(fft, EXP_SUB))),
        Case(f"zero_{fft}", fft, SHIFT, _pair(_voice(fft, EXP_ZERO))),
        Case(f"loud_{fft}", fft, SHIFT, _pair(_voice(fft, EXP_LOUD[fft][0], factor=EXP_LOUD[fft][1]))),
        Case(f"dc_{fft}", fft, SHIFT, _pair(_voice(fft, offset=0.25))),
        Case(f"holes_{fft}", fft, SHIFT, _pair(_voice(fft, hole=True))),
    ]


def _corner_cases(fft):
    return [
        Case(f"corners_{fft}", fft, SHIFT, _pair(lambda: tones(fft, corner_bins(fft)))),
        Case(f"outer_{fft}", fft, SHIFT, _pair(lambda: tones(fft, outer_bins(fft)))),
        Case(f"dcnyq_{fft}", fft, SHIFT, _pair(_outer_dc_nyquist(fft))),
        Case(f"single_{fft}", fft, SHIFT, _pair(_single(fft))),
        Case(f"comb_{fft}", fft, SHIFT, _pair(_comb(fft))),
    ]


def _rows(fft, n):
    return lambda: [_voice(fft, stream=j)() for j in range(n)]


ADDRESS_CASES = [
    Case("stretch_1024", 1024, STRETCH, _pair(_voice(1024))),
    Case("stretch_4096", 4096, STRETCH, _pair(_voice(4096))),
    Case("hop300_1024", 1024, dict(SHIFT, hopsize=300), _pair(_voice(1024))),
    Case("rows3_1024", 1024, SHIFT, _rows(1024, 3)),
    Case("rows9_1024", 1024, SHIFT, _rows(1024, 9)),
    Case("rows3_4096", 4096, SHIFT, _rows(4096, 3)),
]
LEVEL_CASES = [c for fft in FFTS for c in _level_cases(fft)]
CORNER_CASES = [c for fft in FFTS for c in _corner_cases(fft)]
CASES = LEVEL_CASES + CORNER_CASES + ADDRESS_CASES
BY_NAME = {c.name: c for c in CASES}
LEVELS = ("ordinary", "mixed", "out", "subnormal", "zero", "loud", "dc", "holes")
CORNERS = ("corners", "outer", "dcnyq", "single", "comb")


@functools.lru_cache(maxsize=None)
def streams(name):
    xs = BY_NAME[name].make()
    for x in xs:
        assert x.dtype == np.float32 and x.shape == (1, frames_of(BY_NAME[name].fft))
        x.setflags(write=False)
    return tuple(xs)


@functools.lru_cache(maxsize=64)
def oracle(name, j):
    """stream j of a case on the oracle: (output, per-call counts, info with "trace", "flush_step" and "planes")"""
    c = BY_NAME[name]
    want, counts, info = O.run_offline(streams(name)[j], block=BLOCK, planes=True, fftsize=c.fft, **c.cfg)
    want.setflags(write=False)
    for v in info["planes"].values():
        v.setflags(write=False)
    return want, tuple(counts), info


def pass_census(planes, fft):
    """Per step and pass of 256 bins (one pass below 512 points): (all bins in range, no bin in range, sound), the
    DC bin left out of both -- the kernels park (1, 1) in its slot -- as boolean arrays [steps, passes] and [steps]."""
    hs = fft // 2
    re, im = np.abs(planes["re"][:, :hs]), np.abs(planes["im"][:, :hs])
    ok = (re >= LO) & (re < HI) & (im >= LO) & (im < HI)
    sound = np.any(planes["re"] != 0, axis=1) | np.any(planes["im"] != 0, axis=1)
    passes = max(hs // 256, 1)
    ok = ok.reshape(len(ok), passes, hs // passes)
    all_in = np.concatenate([ok[:, :1, 1:].all(axis=2), ok[:, 1:].all(axis=2)], axis=1)
    none_in = np.concatenate([(~ok[:, :1, 1:]).all(axis=2), (~ok[:, 1:]).all(axis=2)], axis=1)
    return all_in, none_in, sound
