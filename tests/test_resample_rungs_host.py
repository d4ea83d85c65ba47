"""The resampling kernel's ladder (pv_kernels.hip resample_rung / launch_resample) at large pitch ratios, one row per
regime: the table, and what can be checked about it without a GPU.

Pitch up is down-sampling: Speex stretches the filter with the ratio (64 taps up to +12 st, then 64 * ratio rounded up
to a multiple of 4... 2048 at +60), lowers the oversampling (8, 4 above +12, 2 above +24, 1 above +36) and the tile of
256 outputs spans 256 * ratio + taps samples.  The launcher picks its kernel from the LDS that table + rows x tile need:

  PV_ARITH_FAST   matrix cores (16 rows) while that is at most 64 KB: up to +16.83 st
                  else the vector kernel with 8 rows: from +16.84; above 64 KB from +28.88; no fit from +46.28
                  (the vector kernel with 16 rows only under AUDIOMOD_PV_RES_MFMA=0, rows >= 16, up to +16.83)
  PV_ARITH_EXACT  the reference-order kernel (4 rows): above 64 KB from +40.95; no fit from +56.77

RUNGS gives each regime a row: the pitch, the arithmetic settings it runs under, and the literal (rung, interpolated,
oversampling, above 64 KB) it is meant to reach -- or REFUSED.  Nothing here derives those literals: the library says
which rung a configuration gets (engine.resample_rung: the launcher's own function), and on the GPU the census says
what was launched (tests/test_resample_rungs_gpu.py).  All boundaries above were found by sweeping the library in 0.01
steps (test_regimes_change_only_at_the_tables_boundaries holds them); they are the same at every FFT size.

The near-zero rows: Speex compares `filt_len / oversample * den_rate` ... in 32-bit unsigned arithmetic when it picks
the oversampling; with den_rate near 2.7e8 the product wraps, and for some pitches in (0, 0.23) st the oversampling comes
out 4 instead of 8 (+0.16: 4; +0.10: 8; below zero the rates are the other way round and nothing wraps: -0.16: 8)."""
import collections
import os
import subprocess
import sys

import pytest

from audiomod_amd import engine as E

FAST, EXACT = E.ARITH_FAST, E.ARITH_EXACT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFT = 512            # the cheapest wave-FFT size; the ladder does not depend on it
ROWS = 18            # 9 stereo streams: one full 16-row group and a partial one
LDS_MAX = 160 * 1024 - 512
REFUSED = "refused"

Row = collections.namedtuple("Row", "name semitones ariths want taps")


def _r(name, semitones, ariths, want, taps):
    return Row(name, semitones, ariths, want, taps)


#      name            pitch  settings       (rung, interp, oversample, above 64 KB)   taps
RUNGS = [
    _r("+16.5_mfma_limit", 16.5, (FAST,), ("mfma", 1, 4, 0), 164),      # 64 064 of 65 536 bytes
    _r("+17_first_vec8", 17.0, (FAST,), ("vec8", 1, 4, 0), 168),
    _r("+24_direct_256", 24.0, (FAST,), ("vec8", 0, 4, 0), 256),
    _r("+24.5_oversample2", 24.5, (FAST,), ("vec8", 1, 2, 0), 264),
    _r("+30_vec8_big", 30.0, (FAST,), ("vec8", 1, 2, 1), 360),
    _r("+36_direct_512_big", 36.0, (FAST,), ("vec8", 0, 2, 1), 512),
    _r("+40_oversample1", 40.0, (FAST,), ("vec8", 1, 1, 1), 644),
    _r("+46_last_fit", 46.0, (FAST,), ("vec8", 1, 1, 1), 912),        # 160 912 of 163 328 bytes
    _r("+46.5_refused", 46.5, (FAST,), REFUSED, 940),
    _r("+60_refused", 60.0, (FAST, EXACT), REFUSED, 2048),
    _r("+24_exact", 24.0, (EXACT,), ("ref4", 0, 4, 0), 256),
    _r("+36_exact", 36.0, (EXACT,), ("ref4", 0, 2, 0), 512),
    _r("+40_exact", 40.0, (EXACT,), ("ref4", 1, 1, 0), 644),
    _r("+42_exact_big", 42.0, (EXACT,), ("ref4", 1, 1, 1), 724),
    _r("+56_exact_last_fit", 56.0, (EXACT,), ("ref4", 1, 1, 1), 1624),
    _r("+57_exact_refused", 57.0, (EXACT,), REFUSED, 1720),
    # pitch down is up-sampling: 64 taps, oversampling 8; the direct table where den <= oversample
    _r("-24_direct_den4_fast", -24.0, (FAST,), ("mfma", 0, 8, 0), 64),
    _r("-24_direct_den4_exact", -24.0, (EXACT,), ("ref4", 0, 8, 0), 64),
    _r("-30_interp_fast", -30.0, (FAST,), ("mfma", 1, 8, 0), 64),
    _r("-30_interp_exact", -30.0, (EXACT,), ("ref4", 1, 8, 0), 64),
    _r("-36_direct_den8_fast", -36.0, (FAST,), ("mfma", 0, 8, 0), 64),   # den = oversample: on the boundary
    _r("-36_direct_den8_exact", -36.0, (EXACT,), ("ref4", 0, 8, 0), 64),
    # the 32-bit wrap just above zero, its mirror below and a neighbour
    _r("+0.16_wrap4_fast", 0.16, (FAST,), ("mfma", 1, 4, 0), 64),
    _r("+0.16_wrap4_exact", 0.16, (EXACT,), ("ref4", 1, 4, 0), 64),
    _r("-0.16_mirror8_fast", -0.16, (FAST,), ("mfma", 1, 8, 0), 64),
    _r("-0.16_mirror8_exact", -0.16, (EXACT,), ("ref4", 1, 8, 0), 64),
    _r("+0.10_neighbour8_fast", 0.10, (FAST,), ("mfma", 1, 8, 0), 64),
    _r("+0.10_neighbour8_exact", 0.10, (EXACT,), ("ref4", 1, 8, 0), 64),
]
BY_NAME = {r.name: r for r in RUNGS}
CASES = [(r.name, a) for r in RUNGS for a in r.ariths]
ACCEPTED = [(n, a) for n, a in CASES if BY_NAME[n].want != REFUSED]
REFUSALS = [(n, a) for n, a in CASES if BY_NAME[n].want == REFUSED]
# the 16-row vector rung exists only under AUDIOMOD_PV_RES_MFMA=0 (read once per process): its own child process
VEC16 = dict(semitones=4.0, rows=16, want=("vec16", 1, 8, 0))
VEC16_DIRECT = dict(semitones=-24.0, rows=16, want=("vec16", 0, 8, 0))   # (tests/test_resample_mfma_gpu.py runs it: 18 rows)
# The mixed pool sizes its buffers for the worst case of its RANGE with an oversampling-8 table bound (pv_engine.cc
# pool_size_range), so it refuses a range whose upper end lies above +37.62 st (PV_ARITH_FAST) / +43.29 st (EXACT) although
# a uniform pool serves the pitch.  These accepted rows, and no others, are refused by a mixed pool of mixed_pool_range.
MIXED_POOL_REFUSES = {("+40_oversample1", FAST), ("+46_last_fit", FAST), ("+56_exact_last_fit", EXACT)}


def mixed_pool_range(semitones):
    """the range of the mixed pool that serves a row beside a slot at 0 st (tests/test_resample_rungs_gpu.py)"""
    return (min(semitones, 0.0) - 0.5, max(semitones, 0.0) + 0.5)


def case_id(case):
    name, arith = case
    return name if len(BY_NAME[name].ariths) == 1 else name + ("-fast" if arith == FAST else "-exact")


def config(row, **more):
    return dict(dict(mode="normal_pitchshift", fftsize=FFT, semitones=row.semitones), **more)


def regime(r):
    return REFUSED if r["refused"] else (r["rung"], r["interp"], r["oversample"], int(r["lds_bytes"] > 64 * 1024))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_library_picks_the_literal_rung(case):
    name, arith = case
    row = BY_NAME[name]
    for rows in (ROWS, 1, 2):   # the batch of 9 stereo streams, the mono one, the single-stream engine
        r = E.resample_rung(arith, rows, **config(row))
        assert r["resample"] == 1 and r["filt_len"] == row.taps, (name, r)
        assert regime(r) == row.want, (name, rows, r)
        if row.want == REFUSED:
            assert "above the limit" in r["reason"] and "%+.2f semitones" % row.semitones in r["reason"], r["reason"]
            assert r["lds_bytes"] > LDS_MAX
        else:
            assert r["lds_bytes"] <= LDS_MAX and r["reason"] == ""
        if not r["interp"]:   # a direct table: one of the two rates is 1, the other at most the oversampling
            assert min(r["res_num"], r["res_den"]) == 1 and r["res_den"] <= r["oversample"], r
    # the same at every size: the ladder reads the pitch alone
    for fft in (256, 2048, 8192):
        r = E.resample_rung(arith, ROWS, **config(row, fftsize=fft))
        if arith == FAST and fft in (256, 8192):
            # no free-form fused kernel at the generic sizes: they resample in the reference's order, with its limit
            assert r["rung"] == "ref4" and r["refused"] == (1 if row.semitones >= 56.77 else 0), (name, fft, r)
            continue
        assert regime(r) == row.want, (name, fft, r)


def test_generic_sizes_resample_in_the_reference_order_under_either_setting():
    for fft in (256, 8192):
        for arith in (FAST, EXACT):
            r = E.resample_rung(arith, ROWS, mode="normal_pitchshift", fftsize=fft, semitones=30.0)
            assert regime(r) == ("ref4", 1, 2, 0), (fft, arith, r)


def test_vec16_rung_under_the_vector_switch():
    """16 rows and more, AUDIOMOD_PV_RES_MFMA=0 (read once per process: a child), up to +16.83 st; both table kinds"""
    code = ("import sys; sys.path.insert(0, %r); from audiomod_amd import engine as E\n"
            "for st in (%r, %r):\n"
            "    for rows in (15, 16, 18):\n"
            "        r = E.resample_rung(E.ARITH_FAST, rows, mode='normal_pitchshift', fftsize=%d, semitones=st)\n"
            "        print(st, rows, r['rung'], r['interp'], r['oversample'], int(r['lds_bytes'] > 65536))\n"
            "r = E.resample_rung(E.ARITH_FAST, 18, mode='normal_pitchshift', fftsize=%d, semitones=17.0)\n"
            "print('17st', r['rung'])\n") % (ROOT, VEC16["semitones"], VEC16_DIRECT["semitones"], FFT, FFT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, AUDIOMOD_PV_RES_MFMA="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("\n")[:7] == ["4.0 15 vec8 1 8 0", "4.0 16 vec16 1 8 0", "4.0 18 vec16 1 8 0",
                                        "-24.0 15 vec8 0 8 0", "-24.0 16 vec16 0 8 0", "-24.0 18 vec16 0 8 0",
                                        "17st vec8"], r.stdout


def test_every_rung_and_table_kind_has_a_row():
    """launch_resample chooses among four kernels x {direct, interpolated}: all eight occur and have a row (the two of
    the 16-row vector kernel in the child process above and in tests/test_resample_mfma_gpu.py's vector child).  The 2-
    and 4-row kernels belong to the mixed batch alone."""
    have = {(r.want[0], r.want[1]) for r in RUNGS if r.want != REFUSED}
    have |= {(v["want"][0], v["want"][1]) for v in (VEC16, VEC16_DIRECT)}
    assert have == {(rung, interp) for rung in ("ref4", "vec8", "vec16", "mfma") for interp in (0, 1)}
    # above 64 KB: both kernels that can get there, with both table kinds for the 8-row kernel; the reference-order
    # kernel's direct tables stop at +48 st (21 KB + 4 rows x 21 KB: above 64 KB) -- refused territory for FAST, so
    # the row set keeps to interpolated there
    big = {(r.want[0], r.want[1]) for r in RUNGS if r.want != REFUSED and r.want[3]}
    assert big == {("vec8", 0), ("vec8", 1), ("ref4", 1)}
    assert {r.want[2] for r in RUNGS if r.want != REFUSED} == {8, 4, 2, 1}   # every oversampling
    assert len(BY_NAME) == len(RUNGS)
    assert {r.name for r in RUNGS if r.want == REFUSED} == {"+46.5_refused", "+60_refused", "+57_exact_refused"}


# ---- the regimes over the whole range, in 0.01 steps
def _expected(arith, st):
    """(rung, above 64 KB) or REFUSED, from the table's boundaries written out as literals"""
    if arith == FAST:
        if st >= 46.28:
            return REFUSED
        return ("mfma", 0) if st <= 16.83 else ("vec8", int(st >= 28.88))
    if st >= 56.77:
        return REFUSED
    return ("ref4", int(st >= 40.95))


def _oversample(st):
    return 8 if st <= 12.0 else 4 if st <= 24.0 else 2 if st <= 36.0 else 1


@pytest.mark.parametrize("arith", [FAST, EXACT], ids=["fast", "exact"])
def test_regimes_change_only_at_the_tables_boundaries(arith):
    nr = 8 if arith == FAST else 4
    for i in range(-6000, 6001):
        st = i / 100.0
        r = E.resample_rung(arith, ROWS, mode="normal_pitchshift", fftsize=FFT, semitones=st)
        if i == 0:
            assert r["resample"] == 0 and r["rung"] is None
            continue
        got = regime(r)
        assert (got if got == REFUSED else (got[0], got[3])) == _expected(arith, st), (st, r)
        assert r["interp"] == (0 if i % 1200 == 0 and abs(st) <= 36.0 else 1), (st, r)
        if st < 0 or st >= 0.23:
            assert r["oversample"] == _oversample(st), (st, r)
        else:
            assert r["oversample"] in (4, 8), (st, r)
        # the staging of pv_resample_mfma_kernel: a tile of 256 outputs spans at most floor(255 num/den) + 1 + taps
        # samples, and the padded row stride lds_floats - 2 holds that plus the four zeros behind it: its unpadded
        # (`fits == false`) branch is unreachable from any engine, at any pitch
        span = (255 * r["res_num"]) // r["res_den"] + 1 + r["filt_len"]
        assert r["lds_floats"] % 4 == 0 and span + 4 <= r["lds_floats"] - 2, (st, r)
        if i % 10 == 0 or got == REFUSED or abs(st - 46.28) < 0.05 or abs(st - 56.77) < 0.05:
            # "refused" against the planner's own constants and the layout rule restated here
            info = E.plan_simulate([480], channels=2, mode="normal_pitchshift", fftsize=FFT, semitones=st)[3]
            assert (info["res_num"], info["res_den"], info["res_filt_len"], info["res_oversample"], info["res_interp"]) == \
                (r["res_num"], r["res_den"], r["filt_len"], r["oversample"], r["interp"]), (st, info, r)
            taps, ov = info["res_filt_len"], info["res_oversample"]
            tab = ov * (taps + 1) * 16 if info["res_interp"] else (info["res_den"] * taps * 4 + 15) & ~15
            lds = (int(256 * (info["res_num"] / info["res_den"])) + taps + 4 + 4 + 3) & ~3
            assert (tab, lds) == (r["tab_bytes"], r["lds_floats"]), (st, r)
            assert (tab + 4 * lds * nr > LDS_MAX) == (got == REFUSED), (st, r)


# ---- refusal at creation: decided from the derived constants, before any device call -- so it shows without a GPU
def _refused(make, semitones):
    with pytest.raises(E.PvError) as e:
        make()
    msg = str(e.value)
    assert "not supported" in msg.lower() or "unsupported" in msg.lower(), msg
    assert "above the limit" in msg and "%+.2f semitones" % semitones in msg and "bytes of LDS" in msg, msg


@pytest.mark.parametrize("case", REFUSALS, ids=case_id)
def test_every_uniform_entry_point_refuses_at_creation(case):
    name, arith = case
    st = BY_NAME[name].semitones
    prev = E.set_arithmetic(arith)
    try:
        kw = dict(mode="normal_pitchshift", fftsize=FFT, semitones=st)
        _refused(lambda: E.PhaseVocoder(48000, 2, 1.0, st, E.NORMAL_SHIFT, E.PHASE_LOCKED, FFT), st)
        _refused(lambda: E.Batch(9, 6000, channels=2, **kw), st)
        _refused(lambda: E.Batch(1, 6000, channels=1, **kw), st)
        _refused(lambda: E.StreamPool(3, channels=2, **kw), st)
        _refused(lambda: E.HostIO(9, 6000, channels=2, **kw), st)
        _refused(lambda: E.HostIO(9, 6000, channels=2, launches_per_segment=2, **kw), st)
    finally:
        E.set_arithmetic(prev)


def test_the_dropin_class_refuses_in_its_constructor(tmp_path):
    demo = os.path.join(ROOT, "audiomod_amd", "lib", "shim_demo")
    assert os.path.exists(demo), "run `make` first"
    fin = str(tmp_path / "in.f32")
    open(fin, "wb").write(b"\0" * (4 * 2 * 480))
    cmd = [demo, "offline", fin, str(tmp_path / "out.f32"), str(tmp_path / "cnt.txt"), "2", "480", "48000", "1.0", "60.0",
           "0", "1", str(FFT), "480", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "above the limit" in r.stderr and "+60.00 semitones" in r.stderr, r.stderr[-1500:]
    assert not os.path.exists(str(tmp_path / "out.f32"))


MIXED_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
from audiomod_amd import engine as E
from tests import test_resample_rungs_host as T

def pool(arith, rng):
    prev = E.set_arithmetic(arith)
    try:
        E.StreamPool(3, channels=2, pitch_range=rng, semitones=0.0, mode="normal_pitchshift", fftsize=T.FFT).close_pool()
        return "created"
    except E.PvError as e:
        return str(e)
    finally:
        E.set_arithmetic(prev)

out = {T.case_id(c): pool(c[1], T.mixed_pool_range(T.BY_NAME[c[0]].semitones)) for c in T.ACCEPTED}
for arith, hi in T.MIXED_POOL_LIMITS:
    out["limit %%d %%.2f" %% (arith, hi)] = pool(arith, (0.0, hi))
print(json.dumps(out))
"""
# (arithmetic, upper end of the range): the last accepted and the first refused, found by a 0.01 sweep of pool_create
MIXED_POOL_LIMITS = [(FAST, 37.62), (FAST, 37.63), (EXACT, 43.29), (EXACT, 43.30)]


@pytest.fixture(scope="module")
def mixed_pools():
    """Every mixed-pool creation of this file in one child process that sees no device: pool_create checks the range
    before any device call, so a refused range says so and an accepted one gets as far as looking for a device."""
    import json
    r = subprocess.run([sys.executable, "-c", MIXED_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _range_refused(msg):
    assert ("stream pool range" in msg and "LDS" in msg) or "no gfx950" in msg, msg
    return "stream pool range" in msg


@pytest.mark.parametrize("case", ACCEPTED, ids=case_id)
def test_the_mixed_pool_refuses_exactly_the_listed_rows(mixed_pools, case):
    name, arith = case
    assert _range_refused(mixed_pools[case_id(case)]) == (case in MIXED_POOL_REFUSES), (name, mixed_pools[case_id(case)])
    # the mixed batch checks each stream by the uniform rule: it lays every accepted row out
    prev = E.set_arithmetic(arith)
    try:
        lay = E.mbatch_layout([(6000, BY_NAME[name].semitones, 1.0)], channels=2, mode="normal_pitchshift", fftsize=FFT)
        assert lay["out_frames"] == [6000]
    finally:
        E.set_arithmetic(prev)


def test_mixed_pool_range_limits(mixed_pools):
    got = [_range_refused(mixed_pools["limit %d %.2f" % (a, hi)]) for a, hi in MIXED_POOL_LIMITS]
    assert got == [False, True, False, True], got
    assert MIXED_POOL_REFUSES <= set(ACCEPTED)


# ---- the oracle alone at the GPU test's shapes: conditions the reference meets without us
@pytest.fixture(scope="module")
def voice():
    from audiomod_amd import signals
    return signals.voice(6000, 2, seed=3)


ORACLE_SHAPES = [(FFT, st) for st in sorted({r.semitones for r in RUNGS if r.want != REFUSED})] + \
    [(fft, 30.0) for fft in (2048, 256, 8192)]


@pytest.mark.parametrize("fftsize,semitones", ORACLE_SHAPES)
def test_the_oracle_gives_audio_at_every_accepted_pitch(voice, fftsize, semitones):
    import numpy as np
    from oracle import oracle_py as O
    kw = dict(mode="normal_pitchshift", fftsize=fftsize, semitones=semitones)
    y, counts, info = O.run_offline(voice, **kw)
    calls = [480] * 12 + [240] + [480] * (len(counts) - 13)   # 6000 frames in blocks of 480, then the zero flush
    planned = E.plan_simulate(calls, channels=2, **kw)[0]
    assert list(counts) == [int(a) for a in planned]   # no output slice dropped: the counts are the planner's
    assert y.shape == voice.shape and np.isfinite(y).all()
    assert float(np.sqrt(np.mean(y.astype(np.float64) ** 2))) > 1e-3
    assert info["resample"] == 1
