"""The carrier setting without a GPU (include/audiomod_pv.h "Carrier setting"): the closed form of the vocoder carrier
(pv_plan_carrier, audiomod_amd/csrc/pv_carrier.h) against the sequential generator the single engine feeds from
(pv_plan_table(PV_TABLE_CARRIER): CarrierGen), bit for bit; windows at arbitrary positions; periodicity beyond 2^31 and
2^40; the new symbols and constants; what is refused without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from audiomod_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (48000, 44100, 22050, 16000)
CARRIERS = (("rosenberg", "vocoder"), ("chord", "vocoder_chord"))
N = 200000
TABLE_CARRIER = 2  # PV_TABLE_CARRIER
INVALID_ARG = 1    # PV_ERR_INVALID_ARG


def same_bits_or_nan(got, want):
    """bit for bit where `want` is finite or infinite; NaN at the same positions (payloads are not compared)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


_sequence = {}


def sequence(rate, carrier, mode):
    """the first N samples CarrierGen makes at this rate (computed once per case, never changed)"""
    key = (rate, carrier)
    if key not in _sequence:
        seq = E.plan_table(TABLE_CARRIER, max_len=N, channels=2, mode=mode, sample_rate=rate)
        assert seq.shape == (N,)
        seq.setflags(write=False)
        _sequence[key] = seq
    return _sequence[key]


def test_symbols_and_constants():
    L = E.lib()
    header = open(os.path.join(ROOT, "include", "audiomod_pv.h")).read()
    for name in ("pv_pool_set_carrier", "pv_pool_get_carrier", "pv_plan_carrier", "pv_debug_carrier"):
        assert hasattr(L, name), name
        assert re.search(r"\bint %s\(" % name, header), name
    for name, value in (("NONE", 0), ("ROSENBERG", 1), ("CHORD", 2)):
        assert re.search(r"#define PV_CARRIER_%s %d\b" % (name, value), header), name
    assert E.CARRIERS == {"none": 0, "rosenberg": 1, "chord": 2}
    # the setting is not a voice and adds no census kind
    assert E.VOICES == {"robotic": 0, "whisper": 1}
    E.chain_census(False)
    assert L.pv_debug_chain_census_count(9, 1, 1024, 0, 0, 0) == -1


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("carrier,mode", CARRIERS)
def test_closed_form_equals_the_sequential_generator(carrier, mode, rate):
    want = sequence(rate, carrier, mode)
    got = E.plan_carrier(rate, carrier, 0, N)
    assert same_bits_or_nan(got, want)
    # a voice whose opening phase has zero length (round(0.01 * period) == 0: a period below 50 samples) gives the
    # reference's 0 * inf, a NaN per period: the 440 Hz voice at 16 kHz, the chord's upper voices at 22.05 kHz too
    voices = (440.0,) if carrier == "rosenberg" else (440.0, 523.251, 659.255)
    assert bool(np.isnan(want).any()) == any(round(rate / f) < 50 for f in voices)
    assert np.isfinite(want).sum() > N // 2 and float(np.nanmax(np.abs(want))) > 0.05


@pytest.mark.parametrize("rate", (48000, 16000))
@pytest.mark.parametrize("carrier,mode", CARRIERS)
def test_windows_at_arbitrary_first(carrier, mode, rate):
    want = sequence(rate, carrier, mode)
    rng = np.random.default_rng(7)
    firsts = [0, 1, 109, 110, 111, N - 1, N - 4097] + [int(v) for v in rng.integers(0, N - 5000, 12)]
    counts = [1, 63, 64, 65, 110, 111, 4097]
    for k, first in enumerate(firsts):
        n = min(counts[k % len(counts)], N - first)
        assert same_bits_or_nan(E.plan_carrier(rate, carrier, first, n), want[first:first + n]), (first, n)
    assert E.plan_carrier(rate, carrier, 12345, 0).shape == (0,)


@pytest.mark.parametrize("carrier,mode,period", [("rosenberg", "vocoder", 110), ("chord", "vocoder_chord", 378510)])
def test_periodicity_across_the_32_bit_boundary(carrier, mode, period):
    """48 kHz: the single voice repeats after 110 samples, the chord after lcm(110, 93, 74) = 378510"""
    want = sequence(48000, carrier, mode)
    n = 5000
    for above in (1 << 31, 1 << 40):
        m = above // period + 1
        for r in (0, 1, 109, period - 1, 12345 % period):
            first = period * m + r
            assert first > above
            assert same_bits_or_nan(E.plan_carrier(48000, carrier, first, n), E.plan_carrier(48000, carrier, r, n)), (m, r)
            if r + n <= N:
                assert same_bits_or_nan(E.plan_carrier(48000, carrier, first, n), want[r:r + n]), (m, r)


def test_refusals_without_a_device():
    L = E.lib()
    out = (C.c_float * 16)()
    v = C.c_int(5)
    assert L.pv_pool_set_carrier(None, 0, 1) == INVALID_ARG
    assert L.pv_pool_get_carrier(None, 0, C.byref(v)) == INVALID_ARG and v.value == 5
    assert L.pv_plan_carrier(48000, 1, 0, 16, None) == INVALID_ARG
    for bad in (0, 3, 7, -1):  # NONE is no carrier to generate
        assert L.pv_plan_carrier(48000, bad, 0, 16, out) == INVALID_ARG, bad
    assert L.pv_plan_carrier(48000, 1, -1, 16, out) == INVALID_ARG
    assert L.pv_plan_carrier(48000, 2, 0, -1, out) == INVALID_ARG
    assert L.pv_plan_carrier(0, 1, 0, 16, out) == INVALID_ARG
    assert L.pv_plan_carrier(48000, 1, 0, 16, out) == 0
    # the diagnostics call decides its arguments before it looks for a device
    first, count = (C.c_int64 * 2)(0, -1), (C.c_int32 * 2)(4, 4)
    assert L.pv_debug_carrier(48000, 1, first, count, 2, out, 0) == INVALID_ARG
    first, count = (C.c_int64 * 2)(0, 4), (C.c_int32 * 2)(4, -4)
    assert L.pv_debug_carrier(48000, 1, first, count, 2, out, 0) == INVALID_ARG
    assert L.pv_debug_carrier(48000, 5, first, count, 2, out, 0) == INVALID_ARG
    assert L.pv_debug_carrier(48000, 1, None, count, 2, out, 0) == INVALID_ARG
    assert L.pv_debug_carrier(48000, 1, first, count, 2, None, 0) == INVALID_ARG
