"""The fused synthesis + overlap-add kernel's ladder (pv_kernels.hip launch_chain), one case per rung: the table, and
what can be checked about it without a GPU.

The kernel exists in four sets (batch, pool, pmix, mb) of 60 instantiations each: NC 256 ... 2048 (fft 512 ... 4096) x
{kPlainCore 0 / 1 / 2 x kRes x kFast, kPlainCore -1 x kRes} plus kPlainCore 3 x kRes x kFast at NC 1024.  TABLE has one
PRIMARY entry per rung -- a configuration inside the stream pool's scope, so the same entry drives all four sets -- and
the rung it is meant to reach, written out as the literal (nc, plain_core, res, fast).  Nothing here derives that
literal: the library says which rung a configuration gets (engine.chain_rung, the engine's own route), and on the GPU
the census says which instantiation was launched (tests/test_chain_rungs_gpu.py).

Routes: plain core c with resampling = normal_pitchshift at core mode c with a pitch; without = time_stretch at core
mode c, pitch 0 and a time ratio; core 3 = gender_change / formant_pitchshift at fft 2048, core mode 1 (gender_change at
0 semitones still compensates, freq_comp 0.8, and does not resample); -1 = robotic, at 0 semitones or with a pitch.
kFast is the arithmetic setting; the all-modes kernel has no free-form twin, so a -1 entry runs under both settings and
expects the same rung.  EXTRA entries are second routes into -1 (formant / gender at the sizes and core modes without
a specialisation: the frequency-compensation branch of the all-modes kernel).

`values`: three (semitones, time_ratio) that stay in the entry's rung and resampler table kind, for the sets whose slots
differ (pmix, mb); the uniform sets run values[0].  Per size the resampling entries use +4 (interpolated table, down),
-7 (interpolated, up) and +-12 (direct table)."""
import collections

import pytest

from audiomod_amd import engine as E

FAST, EXACT = E.ARITH_FAST, E.ARITH_EXACT
FRAMES, BLOCK, CHUNK_SLICES = 24000, 480, 4
MB_FRAMES = (24000, 17003, 9001)

P4 = ((4.0, 1.0), (3.7, 1.0), (5.0, 1.0))       # interpolated table, down-sampling
M7 = ((-7.0, 1.0), (-5.0, 1.0), (-0.5, 1.0))    # interpolated table, up-sampling
D12 = ((12.0, 1.0), (-12.0, 1.0), (12.0, 1.0))  # direct table (the only two pitches of the range that have one)
STRETCH = ((0.0, 1.5), (0.0, 0.8), (0.0, 1.25))
ZERO = ((0.0, 1.0),) * 3                        # a rung that admits 0 semitones only: one value, different signals

Entry = collections.namedtuple("Entry", "name kw rung ariths values primary")


def _e(name, kw, rung, ariths, values, primary=True):
    return Entry(name, kw, rung, ariths, values, primary)


TABLE = [
    _e("shift_512_c0_fast", dict(mode="normal_pitchshift", fftsize=512, coremode=0), (256, 0, 1, 1), (FAST,), P4),
    _e("stretch_512_c0_fast", dict(mode="time_stretch", fftsize=512, coremode=0), (256, 0, 0, 1), (FAST,), STRETCH),
    _e("shift_512_c0_exact", dict(mode="normal_pitchshift", fftsize=512, coremode=0), (256, 0, 1, 0), (EXACT,), P4),
    _e("stretch_512_c0_exact", dict(mode="time_stretch", fftsize=512, coremode=0), (256, 0, 0, 0), (EXACT,), STRETCH),
    _e("shift_512_c1_fast", dict(mode="normal_pitchshift", fftsize=512, coremode=1), (256, 1, 1, 1), (FAST,), M7),
    _e("stretch_512_c1_fast", dict(mode="time_stretch", fftsize=512, coremode=1), (256, 1, 0, 1), (FAST,), STRETCH),
    _e("shift_512_c1_exact", dict(mode="normal_pitchshift", fftsize=512, coremode=1), (256, 1, 1, 0), (EXACT,), M7),
    _e("stretch_512_c1_exact", dict(mode="time_stretch", fftsize=512, coremode=1), (256, 1, 0, 0), (EXACT,), STRETCH),
    _e("shift_512_c2_fast", dict(mode="normal_pitchshift", fftsize=512, coremode=2), (256, 2, 1, 1), (FAST,), D12),
    _e("stretch_512_c2_fast", dict(mode="time_stretch", fftsize=512, coremode=2), (256, 2, 0, 1), (FAST,), STRETCH),
    _e("shift_512_c2_exact", dict(mode="normal_pitchshift", fftsize=512, coremode=2), (256, 2, 1, 0), (EXACT,), D12),
    _e("stretch_512_c2_exact", dict(mode="time_stretch", fftsize=512, coremode=2), (256, 2, 0, 0), (EXACT,), STRETCH),
    _e("robotic_512_res", dict(mode="robotic", fftsize=512), (256, -1, 1, 0), (FAST, EXACT), P4),
    _e("robotic_512", dict(mode="robotic", fftsize=512), (256, -1, 0, 0), (FAST, EXACT), ZERO),
    _e("shift_1024_c0_fast", dict(mode="normal_pitchshift", fftsize=1024, coremode=0), (512, 0, 1, 1), (FAST,), P4),
    _e("stretch_1024_c0_fast", dict(mode="time_stretch", fftsize=1024, coremode=0), (512, 0, 0, 1), (FAST,), STRETCH),
    _e("shift_1024_c0_exact", dict(mode="normal_pitchshift", fftsize=1024, coremode=0), (512, 0, 1, 0), (EXACT,), P4),
    _e("stretch_1024_c0_exact", dict(mode="time_stretch", fftsize=1024, coremode=0), (512, 0, 0, 0), (EXACT,), STRETCH),
    _e("shift_1024_c1_fast", dict(mode="normal_pitchshift", fftsize=1024, coremode=1), (512, 1, 1, 1), (FAST,), M7),
    _e("stretch_1024_c1_fast", dict(mode="time_stretch", fftsize=1024, coremode=1), (512, 1, 0, 1), (FAST,), STRETCH),
    _e("shift_1024_c1_exact", dict(mode="normal_pitchshift", fftsize=1024, coremode=1), (512, 1, 1, 0), (EXACT,), M7),
    _e("stretch_1024_c1_exact", dict(mode="time_stretch", fftsize=1024, coremode=1), (512, 1, 0, 0), (EXACT,), STRETCH),
    _e("shift_1024_c2_fast", dict(mode="normal_pitchshift", fftsize=1024, coremode=2), (512, 2, 1, 1), (FAST,), D12),
    _e("stretch_1024_c2_fast", dict(mode="time_stretch", fftsize=1024, coremode=2), (512, 2, 0, 1), (FAST,), STRETCH),
    _e("shift_1024_c2_exact", dict(mode="normal_pitchshift", fftsize=1024, coremode=2), (512, 2, 1, 0), (EXACT,), D12),
    _e("stretch_1024_c2_exact", dict(mode="time_stretch", fftsize=1024, coremode=2), (512, 2, 0, 0), (EXACT,), STRETCH),
    _e("robotic_1024_res", dict(mode="robotic", fftsize=1024), (512, -1, 1, 0), (FAST, EXACT), M7),
    _e("robotic_1024", dict(mode="robotic", fftsize=1024), (512, -1, 0, 0), (FAST, EXACT), ZERO),
    _e("shift_2048_c0_fast", dict(mode="normal_pitchshift", fftsize=2048, coremode=0), (1024, 0, 1, 1), (FAST,), P4),
    _e("stretch_2048_c0_fast", dict(mode="time_stretch", fftsize=2048, coremode=0), (1024, 0, 0, 1), (FAST,), STRETCH),
    _e("shift_2048_c0_exact", dict(mode="normal_pitchshift", fftsize=2048, coremode=0), (1024, 0, 1, 0), (EXACT,), P4),
    _e("stretch_2048_c0_exact", dict(mode="time_stretch", fftsize=2048, coremode=0), (1024, 0, 0, 0), (EXACT,), STRETCH),
    _e("shift_2048_c1_fast", dict(mode="normal_pitchshift", fftsize=2048, coremode=1), (1024, 1, 1, 1), (FAST,), M7),
    _e("stretch_2048_c1_fast", dict(mode="time_stretch", fftsize=2048, coremode=1), (1024, 1, 0, 1), (FAST,), STRETCH),
    _e("shift_2048_c1_exact", dict(mode="normal_pitchshift", fftsize=2048, coremode=1), (1024, 1, 1, 0), (EXACT,), M7),
    _e("stretch_2048_c1_exact", dict(mode="time_stretch", fftsize=2048, coremode=1), (1024, 1, 0, 0), (EXACT,), STRETCH),
    _e("shift_2048_c2_fast", dict(mode="normal_pitchshift", fftsize=2048, coremode=2), (1024, 2, 1, 1), (FAST,), D12),
    _e("stretch_2048_c2_fast", dict(mode="time_stretch", fftsize=2048, coremode=2), (1024, 2, 0, 1), (FAST,), STRETCH),
    _e("shift_2048_c2_exact", dict(mode="normal_pitchshift", fftsize=2048, coremode=2), (1024, 2, 1, 0), (EXACT,), D12),
    _e("stretch_2048_c2_exact", dict(mode="time_stretch", fftsize=2048, coremode=2), (1024, 2, 0, 0), (EXACT,), STRETCH),
    _e("formant_2048_fast", dict(mode="formant_pitchshift", fftsize=2048, coremode=1), (1024, 3, 1, 1), (FAST,), P4),
    _e("gender_2048_exact", dict(mode="gender_change", fftsize=2048, coremode=1), (1024, 3, 1, 0), (EXACT,), M7),
    _e("gender0_2048_fast", dict(mode="gender_change", fftsize=2048, coremode=1), (1024, 3, 0, 1), (FAST,), ZERO),
    _e("gender0_2048_exact", dict(mode="gender_change", fftsize=2048, coremode=1), (1024, 3, 0, 0), (EXACT,), ZERO),
    _e("robotic_2048_res", dict(mode="robotic", fftsize=2048), (1024, -1, 1, 0), (FAST, EXACT), D12),
    _e("robotic_2048", dict(mode="robotic", fftsize=2048), (1024, -1, 0, 0), (FAST, EXACT), ZERO),
    _e("shift_4096_c0_fast", dict(mode="normal_pitchshift", fftsize=4096, coremode=0), (2048, 0, 1, 1), (FAST,), P4),
    _e("stretch_4096_c0_fast", dict(mode="time_stretch", fftsize=4096, coremode=0), (2048, 0, 0, 1), (FAST,), STRETCH),
    _e("shift_4096_c0_exact", dict(mode="normal_pitchshift", fftsize=4096, coremode=0), (2048, 0, 1, 0), (EXACT,), P4),
    _e("stretch_4096_c0_exact", dict(mode="time_stretch", fftsize=4096, coremode=0), (2048, 0, 0, 0), (EXACT,), STRETCH),
    _e("shift_4096_c1_fast", dict(mode="normal_pitchshift", fftsize=4096, coremode=1), (2048, 1, 1, 1), (FAST,), M7),
    _e("stretch_4096_c1_fast", dict(mode="time_stretch", fftsize=4096, coremode=1), (2048, 1, 0, 1), (FAST,), STRETCH),
    _e("shift_4096_c1_exact", dict(mode="normal_pitchshift", fftsize=4096, coremode=1), (2048, 1, 1, 0), (EXACT,), M7),
    _e("stretch_4096_c1_exact", dict(mode="time_stretch", fftsize=4096, coremode=1), (2048, 1, 0, 0), (EXACT,), STRETCH),
    _e("shift_4096_c2_fast", dict(mode="normal_pitchshift", fftsize=4096, coremode=2), (2048, 2, 1, 1), (FAST,), D12),
    _e("stretch_4096_c2_fast", dict(mode="time_stretch", fftsize=4096, coremode=2), (2048, 2, 0, 1), (FAST,), STRETCH),
    _e("shift_4096_c2_exact", dict(mode="normal_pitchshift", fftsize=4096, coremode=2), (2048, 2, 1, 0), (EXACT,), D12),
    _e("stretch_4096_c2_exact", dict(mode="time_stretch", fftsize=4096, coremode=2), (2048, 2, 0, 0), (EXACT,), STRETCH),
    _e("robotic_4096_res", dict(mode="robotic", fftsize=4096), (2048, -1, 1, 0), (FAST, EXACT), P4),
    _e("robotic_4096", dict(mode="robotic", fftsize=4096), (2048, -1, 0, 0), (FAST, EXACT), ZERO),
    # second routes into the all-modes kernel: its frequency-compensation branch
    _e("gender_512", dict(mode="gender_change", fftsize=512, coremode=1), (256, -1, 1, 0), (FAST, EXACT), M7, False),
    _e("formant_1024", dict(mode="formant_pitchshift", fftsize=1024, coremode=1), (512, -1, 1, 0), (FAST, EXACT), P4[::-1], False),
    _e("formant_4096", dict(mode="formant_pitchshift", fftsize=4096, coremode=1), (2048, -1, 1, 0), (FAST, EXACT), P4[::-1], False),
    _e("gender_2048_c0", dict(mode="gender_change", fftsize=2048, coremode=0), (1024, -1, 1, 0), (FAST, EXACT), P4, False),
    _e("formant_2048_c2", dict(mode="formant_pitchshift", fftsize=2048, coremode=2), (1024, -1, 1, 0), (FAST, EXACT), M7, False),
]
BY_NAME = {e.name: e for e in TABLE}
CASES = [(e.name, a) for e in TABLE for a in e.ariths]   # what the GPU tests are parametrised over, beside the set
PLAIN = [e for e in TABLE if e.primary and e.rung[1] in (0, 1, 2) and e.ariths == (EXACT,)]   # 4 sizes x 3 cores x 2


def case_id(case):
    name, arith = case
    return name if len(BY_NAME[name].ariths) == 1 else name + ("-fast" if arith == FAST else "-exact")


def config(entry, value=None):
    """The configuration of one stream of the entry: its own (values[0]) or at another of its values."""
    semitones, ratio = entry.values[0] if value is None else value
    return dict(entry.kw, semitones=semitones, time_ratio=ratio)


def all_rungs():
    out = []
    for nc in (256, 512, 1024, 2048):
        for res in (0, 1):
            out.append((nc, -1, res, 0))
            for fast in (0, 1):
                out += [(nc, core, res, fast) for core in (0, 1, 2)]
                if nc == 1024:
                    out.append((nc, 3, res, fast))
    return out


def test_the_table_covers_every_rung_exactly_once():
    want = all_rungs()
    assert len(want) == 60 and len(set(want)) == 60
    primary = [e.rung for e in TABLE if e.primary]
    assert sorted(primary) == sorted(want)
    assert len(BY_NAME) == len(TABLE)
    for e in TABLE:
        # kFast is the arithmetic setting, except that the all-modes kernel has no free-form twin
        assert e.ariths == ((FAST, EXACT) if e.rung[1] < 0 else ((FAST,) if e.rung[3] else (EXACT,))), e.name
        assert len(e.values) == 3
        if not e.primary:
            assert e.rung[1] == -1
    assert len(PLAIN) == 24
    # per size, the resampling entries bring an interpolated table in both directions and a direct one
    for fft in (512, 1024, 2048, 4096):
        pitches = {e.values[0][0] for e in TABLE if e.kw["fftsize"] == fft and e.rung[2] == 1}
        assert {4.0, -7.0} <= pitches and pitches & {12.0, -12.0}, (fft, pitches)


def _rung_of(arith, cfg):
    r = E.chain_rung(arith, **cfg)
    return r, (r["nc"], r["plain_core"], r["resample"], r["fast"])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_library_picks_the_literal_rung(case):
    name, arith = case
    e = BY_NAME[name]
    for value in e.values:   # every slot / stream value of the pmix and mb objects stays in the rung
        r, got = _rung_of(arith, config(e, value))
        assert got == e.rung, (name, value, got)
        if e.rung[1] >= 0:   # a specialisation: the other setting picks its twin, everything else the same
            _, twin = _rung_of(FAST if arith == EXACT else EXACT, config(e, value))
            assert twin == e.rung[:3] + (1 - e.rung[3],), (name, value, twin)


# launch bounds of the kernels in waves (pv_kernels.hip chain_kernel_max_threads), restated as literals: what engine
# creation sizes the launch by has to be the bound of the rung the ladder picks
def _bound(rung):
    nc, core, _, fast = rung
    return 8 if nc == 2048 else (12 if core < 0 or (core == 3 and not fast) else 16)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_engine_creation_agrees_with_the_ladder(case):
    name, arith = case
    e = BY_NAME[name]
    for value in e.values:
        r, got = _rung_of(arith, config(e, value))
        assert r["wave_bound"] == _bound(got), (name, value, r)
        assert r["reciprocal_wden"] == got[3], (name, value, r)   # reciprocals exactly where the free-form twin runs


def test_table_kinds_of_the_values():
    """+4 / -7 interpolate, +-12 are direct; the stretch and zero values do not resample"""
    for e in TABLE:
        infos = [E.plan_simulate([BLOCK], channels=2, **config(e, v))[3] for v in e.values]
        assert all(i["resample"] == e.rung[2] for i in infos), e.name
        if e.rung[2]:
            kinds = {i["res_interp"] for i in infos}
            assert kinds == ({0} if e.values[0][0] in (12.0, -12.0) else {1}), (e.name, kinds)


@pytest.mark.parametrize("fftsize", [512, 1024, 2048, 4096])
def test_shapes_carry_state_across_launches(fftsize):
    """24 000 frames: at least 16 slices per row, so with 4 slices per launch (Batch / MixedBatch) at least 4 launches,
    and the pools' 480-frame calls produce slices in at least 3 calls."""
    for e in TABLE:
        if e.kw["fftsize"] != fftsize:
            continue
        for value in e.values[:1] + e.values:
            calls = [BLOCK] * (FRAMES // BLOCK)
            avail, shift, _, info = E.plan_simulate(calls, channels=2, **config(e, value))
            assert len(shift) >= 16, (e.name, value, len(shift))
            assert sum(1 for a in avail if a > 0) >= 3, (e.name, value)
        lay = E.mbatch_layout([(f, s, r) for f, (s, r) in zip(MB_FRAMES, e.values)], channels=2, block=BLOCK, **e.kw)
        assert lay["slices"][0] >= 16 and min(lay["slices"]) > CHUNK_SLICES, (e.name, lay["slices"])
