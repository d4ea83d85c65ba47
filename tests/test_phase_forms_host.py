"""What the phase-locked stage's test signals do to the oracle, step by step (CPU only).

tests/phase_signals.py makes inputs that put the stage's peak lists and step patterns where tests/test_phase_forms_gpu.py
wants them: lists filled to the last slot, single per-bin (PROP) steps between locked (LOCK) ones at chosen positions of a
launch, steps with exactly one peak, PROP steps on frames that are not silent.  This file holds the table of cases and,
per case, literals for what the oracle's per-step trace (oracle_py.Oracle.phase_trace) must contain; every one of them
is asserted, none is a skip: a case that stops producing its situation fails here, before a GPU test that relies on it
could pass for the wrong reason.

Trace: one entry per (slice, channel) step in processing order, so row c of a stream is trace[c::channels]; the mode
strings below are run lengths of I (first step), P (per-bin propagation) and L (locked) of one row.  Step t of a row reads
the input frames [t * hop, t * hop + fft) (zeros past the end: the flush)."""
import collections
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from audiomod_amd import engine as E
from oracle import oracle_py as O
from tests import phase_signals as S

BLOCK = 480
SHIFT = dict(mode="normal_pitchshift", semitones=4.0, coremode=1)
HOP = {512: 50, 1024: 101, 2048: 203, 4096: 406, 8192: 812}   # the input hop of SHIFT, asserted below


def list_capacity(fft):
    """the most peaks a step can find: one every third bin of 2 ... fft/2 - 3"""
    return -(-(fft // 2 - 4) // 3)


Case = collections.namedtuple("Case", "name fft channels frames make expect")


def _comb(fft, frames, channels):
    return lambda: S.comb(fft, frames, channels, seed=fft)


def _gaps(frames, channels, gap_len, start=5050, gap_channel=0):
    return lambda: S.comb_gaps(1024, 101, frames, channels, seed=1024, gap_channel=gap_channel, gap_len=gap_len,
                               starts=(start,))


def _holed(x, start=6000, length=2000):
    """exact zeros over [start, start + length) of every channel: both of a signal's edges in mid-stream"""
    x = x.copy()
    x[:, start:start + length] = 0.0
    return x


def _beside_comb(f, frames):
    """channel 0: the edge-state signal, channel 1: a full comb -- the `no peak in the step before` rule then looks at
    the other channel's list"""
    return lambda: np.concatenate([_holed(f(frames, 1)), S.comb(1024, frames, 1, seed=7)], axis=0)


N1, HOP1 = 1024, 101
FULL = dict(full=True)
# comb: the list is full in every step before the flush.  Literals: full -> max == list_capacity(fft), reached in >= 80 %
# of the steps before the flush.
COMB_CASES = [
    Case("comb_512", 512, 2, 12000, _comb(512, 12000, 2), FULL),
    Case("comb_1024", 1024, 2, 16000, _comb(1024, 16000, 2), FULL),
    Case("comb_2048", 2048, 2, 12000, _comb(2048, 12000, 2), FULL),
    Case("comb_4096", 4096, 2, 24000, _comb(4096, 24000, 2), FULL),
    Case("comb_8192_mono", 8192, 1, 40000, _comb(8192, 40000, 1), FULL),
    Case("comb_8192", 8192, 2, 40000, _comb(8192, 40000, 2), FULL),
]
# Edge states at fft 1024, 16 000 frames (159 steps a row, 140 before the flush).  Literals:
#   modes     : the run lengths of each row's mode string, exactly
#   one_peak  : steps of row 0 with exactly one peak (the line at fs/4 where the frame is partly zeros: the leakage of the
#               cut falls off monotonically on both sides, so the line is the only strict maximum)
#   loud_prop : PROP steps of row 0 without a peak whose input frame is not silent (a DC level under a window cut by
#               zeros: everything falls off from bin 0, no peak at bins >= 2)
#   min_count : the smallest non-zero peak count of row 0 before the flush
EDGE_CASES = [
    Case("gap_single", N1, 2, 16000, _gaps(16000, 2, N1 + HOP1 // 2),   # one PROP step per row, the second row's right
         dict(modes=["I1 L49 P1 L108", "L50 P1 L108"], min_count=11)),  # behind a LOCK step with a full list
    Case("gap_pp", N1, 2, 16000, _gaps(16000, 2, N1 + HOP1 + HOP1 // 2),
         dict(modes=["I1 L49 P2 L107", "L50 P2 L107"], min_count=9)),
    Case("gap_pp_mono", N1, 1, 16000, _gaps(16000, 1, N1 + HOP1 // 2),
         dict(modes=["I1 L49 P2 L107"], min_count=11)),
    Case("gap_short", N1, 2, 16000, _gaps(16000, 2, N1 - 1),           # no PROP step: the list runs down and up again
         dict(modes=["I1 L158", "L159"], min_count=19)),
    Case("quarter_mono", N1, 1, 16000, lambda: _holed(S.quarter(16000, 1)),
         dict(modes=["I1 L59 P11 L88"], one_peak=29, min_count=1)),
    Case("quarter_stereo", N1, 2, 16000, lambda: _holed(S.quarter(16000, 2)),
         dict(modes=["I1 L59 P11 L88", "L60 P10 L89"], one_peak=29, min_count=1)),
    Case("quarter_comb", N1, 2, 16000, _beside_comb(S.quarter, 16000),
         dict(modes=["I1 L59 P10 L89", "L60 P10 L89"], one_peak=29, min_count=1)),
    Case("dc_mono", N1, 1, 16000, lambda: _holed(S.dc(16000, 1)),
         dict(modes=["I1 L49 P30 L69 P10"], loud_prop=29, min_count=4)),
    Case("dc_stereo", N1, 2, 16000, lambda: _holed(S.dc(16000, 2)),
         dict(modes=["I1 L49 P30 L69 P10", "L50 P29 L70 P10"], loud_prop=29, min_count=4)),
    Case("dc_comb", N1, 2, 16000, _beside_comb(S.dc, 16000),
         dict(modes=["I1 L49 P29 L70 P10", "L50 P29 L70 P10"], loud_prop=29, min_count=4)),
]
CASES = COMB_CASES + EDGE_CASES
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def signal(name):
    x = BY_NAME[name].make()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(output, per-call counts, info with the trace) of a case, computed once and shared"""
    c = BY_NAME[name]
    want, counts, info = O.run_offline(signal(name), block=BLOCK, trace=True, fftsize=c.fft, **SHIFT)
    want.setflags(write=False)
    return want, tuple(counts), info


def rows_of(info, channels):
    k, m = info["trace"]
    return [(k[c::channels], m[c::channels]) for c in range(channels)]


def run_lengths(modes):
    out, prev, n = [], None, 0
    for v in list(modes) + [None]:
        if v == prev:
            n += 1
            continue
        if prev is not None:
            out.append("IPL"[prev] + str(n))
        prev, n = v, 1
    return " ".join(out)


def frame_is_silent(x, row, t, fft, hop):
    return not np.any(x[row, t * hop:t * hop + fft])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_signal_reaches_its_situation(case):
    x = signal(case.name)
    assert x.shape == (case.channels, case.frames) and x.dtype == np.float32
    assert np.array_equal(x, np.round(x * 32768.0) / 32768.0) and np.abs(x).max() <= 0.9   # on the int16 grid
    _, _, info = oracle(case.name)
    hop = info["hop_in"]
    assert hop == HOP[case.fft]
    rows = rows_of(info, case.channels)
    steps = info["flush_step"] // case.channels
    assert all(len(k) == info["slices"] for k, _ in rows) and 0 < steps < info["slices"]
    e = case.expect
    if e.get("full"):
        cap = list_capacity(case.fft)
        for k, m in rows:
            assert k.max() == cap, (k.max(), cap)
            assert np.mean(k[:steps] == cap) >= 0.8, np.mean(k[:steps] == cap)
            assert np.all(m[1:steps] == 2)   # and every one of those steps is a LOCK step
    if "modes" in e:
        assert [run_lengths(m) for _, m in rows] == e["modes"]
    k0, m0 = rows[0]
    if "min_count" in e:
        pre = k0[:steps]
        assert pre[pre > 0].min() == e["min_count"], pre[pre > 0].min()
    if "one_peak" in e:
        assert int(np.sum(k0 == 1)) == e["one_peak"]
        # ... and such a step is a LOCK step behind a LOCK step before the flush: region [0, hs) in mid-stream
        assert any(k0[t] == 1 and m0[t] == 2 and m0[t - 1] == 2 for t in range(1, steps))
    if "loud_prop" in e:
        loud = [t for t in range(len(k0)) if m0[t] == 1 and k0[t] == 0 and not frame_is_silent(x, 0, t, case.fft, hop)]
        assert len(loud) == e["loud_prop"], loud
        assert sum(t < steps - 1 for t in loud) >= 10   # in mid-stream, on either edge of the hole: LOCK steps follow


def test_a_prop_step_follows_a_full_list_directly():
    """gap_single: row 1 never has an empty list, its PROP step comes from row 0's, and the LOCK step before it had a
    full list -- where the chain kernels materialise the lazy previous output by a search over all 170 regions"""
    _, _, info = oracle("gap_single")
    (k0, m0), (k1, m1) = rows_of(info, 2)
    t = int(np.flatnonzero(m1 == 1)[0])
    assert k0[t] == 0 and m0[t] == 1
    assert k1[:info["flush_step"] // 2].min() == list_capacity(N1) and m1[t - 1] == 2 and m1[t + 1] == 2


# ---- the placement sweep: one PROP step at every position of a launch, for every launch length used -----------------
SWEEP_STREAMS = 16
SWEEP_FRAMES = 11850   # 118 slices a row: final launches of 1, 2 and 3 slices among the chunkings below
SWEEP_START = 50 * HOP1            # stream j: one gap from frame (50 + j) * hop, so its PROP step is step 50 + j
SWEEP_CHUNKS = {8: (4, 6, 7, 8, 9, 16), 4: (4, 5, 12)}   # ring depth: AUDIOMOD_PV_CHUNK_SLICES values
SWEEP_FINAL = {1, 2, 3}            # lengths of final launches that must occur


@functools.lru_cache(maxsize=None)
def sweep_signal(j):
    x = S.comb_gaps(N1, HOP1, SWEEP_FRAMES, 2, seed=100 + j, gap_channel=j % 2, starts=(SWEEP_START + j * HOP1,))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def sweep_oracle(j):
    want, counts, info = O.run_offline(sweep_signal(j), block=BLOCK, trace=True, fftsize=N1, **SHIFT)
    want.setflags(write=False)
    return want, tuple(counts), info


def sweep_slices(chunk):
    """(slices of a row, launches) of the sweep's batch with `chunk` slices per launch, from the host planner"""
    old = os.environ.get("AUDIOMOD_PV_CHUNK_SLICES")
    os.environ["AUDIOMOD_PV_CHUNK_SLICES"] = str(chunk)
    try:
        spans = E.plan_spans(SWEEP_STREAMS, SWEEP_FRAMES, 1, channels=2, block=BLOCK, fftsize=N1, **SHIFT)
    finally:
        if old is None:
            del os.environ["AUDIOMOD_PV_CHUNK_SLICES"]
        else:
            os.environ["AUDIOMOD_PV_CHUNK_SLICES"] = old
    assert all(s["slice_end"] - s["slice_begin"] == chunk for s in spans[:-1])
    return spans[-1]["slice_end"], len(spans)


def test_the_sweep_puts_the_prop_step_at_every_position_of_a_launch():
    prop = []
    for j in range(SWEEP_STREAMS):
        _, _, info = sweep_oracle(j)
        rows = rows_of(info, 2)
        n, t = info["slices"], 50 + j
        got = [run_lengths(m) for _, m in rows]
        if j % 2 == 0:   # the gap in channel 0: both rows at step t, row 1 on account of row 0's empty list
            assert got == [f"I1 L{t - 1} P1 L{n - t - 1}", f"L{t} P1 L{n - t - 1}"], (j, got)
        else:            # in channel 1: row 0 one step later, on account of row 1's empty list in the step before
            assert got == [f"I1 L{t} P1 L{n - t - 2}", f"L{t} P1 L{n - t - 1}"], (j, got)
        assert rows[j % 2][0][t] == 0 and rows[1 - j % 2][0][:100].min() == list_capacity(N1)   # which row has the gap
        prop.append(t)
    finals = {}
    for depth, chunks in SWEEP_CHUNKS.items():
        for chunk in chunks:
            slices, launches = sweep_slices(chunk)
            assert slices == sweep_oracle(0)[2]["slices"] and launches == -(-slices // chunk)
            # launch i holds the steps [i * chunk, (i + 1) * chunk): tl = step % chunk
            assert {t % chunk for t in prop} == set(range(chunk)), (depth, chunk)
            assert all(t // chunk < launches - 1 for t in prop)   # in whole launches, ones behind it
            finals.setdefault(depth, set()).add(slices - (launches - 1) * chunk)
    assert SWEEP_FINAL <= finals[8] | finals[4], finals
    # launches of D - 2, D - 1, D, D + 1 and 2 D slices behind a ring of depth D; at depth 4 the shortest launch that can
    # be asked for is D, and D - 2 and D - 1 come as final launches
    assert {6, 7, 8, 9, 16} <= set(SWEEP_CHUNKS[8])
    assert {4, 5} <= set(SWEEP_CHUNKS[4]) and {2, 3} <= finals[4], finals


def test_the_phase_census_has_its_keys_and_no_others():
    """PV_CENSUS_PHASE (kind 3): set x form x {1, 3, 4, 8}; anything else is no key.  Without a launch every count is 0."""
    count = E.lib().pv_debug_chain_census_count
    for s in range(len(E.CENSUS_SETS)):
        for f in range(len(E.PHASE_FORMS)):
            assert all(count(3, s, f, b, 0, 0) >= 0 for b in (1, 3, 4, 8))
            assert [count(3, s, f, b, 0, 0) for b in (0, 2, 5, 16, -1)] == [-1] * 5
    assert count(3, 0, 4, 8, 0, 0) == -1 and count(3, 0, -1, 8, 0, 0) == -1 and count(3, 4, 0, 8, 0, 0) == -1
    if not os.environ.get("AUDIOMOD_PV_CHAIN_CENSUS"):   # (switched on for the whole process otherwise: left alone)
        E.chain_census(True)
        try:
            assert E.phase_census_read() == {}
        finally:
            E.chain_census(False)


# ---- the trace buffer itself, outside Python --------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_trace_buffer_under_sanitizers(tmp_path):
    """tests/native/oracle_trace_sanitize.c with the oracle, as one stand-alone program under ASan + UBSan: the buffer
    grows several times and is read back whole and in part"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "oracle_trace_sanitize")
    cmd = ["gcc", "-O1", "-g", "-std=gnu99", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function", f"-I{root}/oracle",
           os.path.join(root, "tests/native/oracle_trace_sanitize.c"), os.path.join(root, "oracle/pv_oracle.c"), "-o", exe,
           "-lm"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        pytest.skip("sanitizer runtimes not installed")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout + r.stderr
