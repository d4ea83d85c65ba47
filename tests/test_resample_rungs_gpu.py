"""Every rung of the resampling ladder at large pitch ratios, on the GPU, against the oracle: the rows of
tests/test_resample_rungs_host.py RUNGS under the arithmetic settings they name.

Per accepted row: the census (engine.resample_census_read) shows exactly the row's rung in the set under test and no
other resampling key; the output counts equal the oracle's; whole-output RMS <= 1e-4 (the project's contract) and the
error-shape bar of tests/helpers.py hold (floor: the oracle against itself with nudged sines and cosines, as
tests/test_parity_shape_gpu.py has it); and the forms that serve the row -- single-stream engine in ragged calls, Batch,
uniform pool, mixed pool, MixedBatch -- give the same bits for the same stream.  The bit-exact tier (ROBOTIC under
PV_ARITH_EXACT, no tolerance) at these pitches is in tests/test_parity_exact_gpu.py.

Shapes: fft 512, 2 channels, 6000 frames of signals.voice; Batch runs 9 stereo streams (18 rows: a full 16-row group
and a partial one) and one mono stream (a single row); +30 st also runs at fft 2048, 256 and 8192.  No configuration
that the host arithmetic refuses is ever launched: refused rows assert the status and message of the create calls and
that the census stays empty."""
import functools
import os

import numpy as np
import pytest

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import assert_shape, bits_equal, oracle_floor, parity_shape
from tests.test_resample_rungs_host import (ACCEPTED, BY_NAME, FAST, FFT, MIXED_POOL_REFUSES, REFUSALS, case_id,
                                            mixed_pool_range)

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4
FRAMES = 6000
RAGGED = [1, 479, 4097, 13, 480, 7, 333]   # partial last tiles of every kind; the rest of the clip follows in one call
NSTEREO = 9


@pytest.fixture(autouse=True)
def census_off_afterwards():
    yield
    E.chain_census(False)


def _arith(arith):
    return E.set_arithmetic(arith)


@functools.lru_cache(maxsize=None)
def clip(stream, channels=2):
    x = signals.voice(FRAMES, 2, seed=3 + 17 * stream)
    return np.ascontiguousarray(x[:channels])


@functools.lru_cache(maxsize=None)
def oracle(stream, channels, flush, fftsize, semitones):
    """(output, per-call counts) of the oracle, run once per (clip, configuration) and shared"""
    y, counts, info = O.run_offline(clip(stream, channels), flush=flush, mode="normal_pitchshift", fftsize=fftsize,
                                    semitones=semitones)
    assert info["resample"] == 1
    y.setflags(write=False)
    return y, tuple(counts)


@functools.lru_cache(maxsize=None)
def floor(stream, channels, flush, fftsize, semitones, arith):
    return oracle_floor(O.run_offline, clip(stream, channels), arith, want=oracle(stream, channels, flush, fftsize,
                        semitones)[0], flush=flush, mode="normal_pitchshift", fftsize=fftsize, semitones=semitones)


def held_to_the_oracle(label, got, stream, channels, flush, fftsize, semitones, arith):
    want = oracle(stream, channels, flush, fftsize, semitones)[0]
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert float(np.sqrt(np.mean(np.asarray(want, np.float64) ** 2))) > 1e-3, label   # there is audio to compare
    s = parity_shape(got, want)
    print(f"{label}: rms {s['rms']:.3e} max_abs {s['max_abs']:.3e} win_rms {s['win_rms']:.3e}")
    assert s["rms"] <= RMS_TOL, (label, s)
    assert_shape(label, got, want, floor(stream, channels, flush, fftsize, semitones, arith), arith)


def census_is(label, want):
    got = E.resample_census_read()
    log = os.environ.get("AUDIOMOD_PARITY_SHAPE_LOG")
    if log:
        with open(log, "a") as fh:
            fh.write(f"{label} census {sorted(got.items())}\n")
    assert set(got) == {want} and got[want] > 0, (label, got, want)


def run_batch(streams, channels, fftsize, semitones, flush=True):
    import torch
    x = np.stack([clip(s, channels) for s in streams])
    b = E.Batch(len(streams), FRAMES, channels=channels, flush=flush, mode="normal_pitchshift", fftsize=fftsize,
                semitones=semitones)
    out = b.run(torch.from_numpy(x).cuda(), d_out=torch.full((len(streams), channels, b.out_frames), float("nan"),
                                                               device="cuda"))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    b.close()
    return out


def run_ragged(semitones, fftsize=FFT, flush=False):
    """flush: zero blocks until the clip's length has come out, as the offline loop does (the stream does not depend on
    how the calls cut it, so the oracle's flushed run in blocks of 480 is the reference)"""
    x = clip(0)
    pv = E.PhaseVocoder(48000, 2, 1.0, semitones, E.NORMAL_SHIFT, E.PHASE_LOCKED, fftsize)
    pos, outs = 0, []
    for n in RAGGED + [FRAMES - sum(RAGGED)]:
        pv.processInData(x[:, pos:pos + n])
        pos += n
        outs.append(pv.getOutData(pv.getOutSamples()))
    assert pos == FRAMES
    produced = sum(o.shape[1] for o in outs)
    zeros = np.zeros((2, 480), np.float32)
    for _ in range(200 if flush else 0):
        if produced >= FRAMES:
            break
        pv.processInData(zeros)
        outs.append(pv.getOutData(pv.getOutSamples()))
        produced += outs[-1].shape[1]
    pv.close()
    y = np.concatenate(outs, axis=1)
    return y[:, :FRAMES] if flush else y


def run_pool(semitones, mixed):
    kw = dict(mode="normal_pitchshift", fftsize=FFT)
    if mixed:
        pool = E.StreamPool(3, channels=2, pitch_range=mixed_pool_range(semitones), semitones=0.0, **kw)
        pool.open(semitones=0.0)   # a neighbour that does not resample
        slot = pool.open(semitones=semitones)
    else:
        pool = E.StreamPool(3, channels=2, semitones=semitones, **kw)
        pool.open()
        slot = pool.open()
    x, got, counts = clip(0), [], []
    for i in range(0, FRAMES, 480):
        pool.feed({slot: x[:, i:i + 480]})
        n = pool.available(slot)
        counts.append(n)
        got.append(pool.retrieve(slot, n))
    pool.close_pool()
    return np.concatenate(got, axis=1), counts


def run_mixed_batch(semitones):
    import torch
    streams = [(FRAMES, semitones, 1.0), (FRAMES - 1234, 0.0, 1.0)]
    mb = E.MixedBatch(streams, channels=2, flush=False, mode="normal_pitchshift", fftsize=FFT)
    out = mb.run(mb.pack([clip(0), clip(1)[:, :FRAMES - 1234]]))
    torch.cuda.synchronize()
    y = mb.split(out)[0].cpu().numpy()
    mb.close()
    return y


@pytest.mark.parametrize("case", ACCEPTED, ids=case_id)
def test_batch_rung_census_and_parity(case, monkeypatch):
    """Batch: 18 rows, then a single row.  Under PV_ARITH_EXACT a batch this small takes the tile path (overlap-add
    and resampling in one kernel, no resampling launch of its own) unless the fused path is asked for: it is, so that
    the reference-order resampling kernel is what runs and what the census counts."""
    name, arith = case
    row = BY_NAME[name]
    st = row.semitones
    rung, interp, _, big = row.want
    prev = _arith(arith)
    try:
        if arith != FAST:
            monkeypatch.setenv("AUDIOMOD_PV_FUSED", "2")
        E.chain_census(True)
        out = run_batch(tuple(range(NSTEREO)), 2, FFT, st)
        census_is(f"{name} batch18", ("batch", rung, interp, big))
        for s in (0, 7, 8):   # the first stream, the last of the full row group, the partial group
            held_to_the_oracle(f"{name} batch18 stream {s}", out[s], s, 2, True, FFT, st, arith)
        E.chain_census(True)
        mono = run_batch((0,), 1, FFT, st)
        one = E.resample_rung(arith, 1, mode="normal_pitchshift", fftsize=FFT, semitones=st)
        census_is(f"{name} batch1", ("batch", rung, interp, int(one["lds_bytes"] > 64 * 1024)))
        held_to_the_oracle(f"{name} batch1", mono[0], 0, 1, True, FFT, st, arith)
    finally:
        _arith(prev)


@pytest.mark.parametrize("case", ACCEPTED, ids=case_id)
def test_forms_agree_and_each_is_held_to_the_oracle(case):
    """The same stereo clip through the single-stream engine (ragged calls), a one-stream Batch, the uniform pool, a
    mixed pool whose range contains the pitch and a MixedBatch, without the zero flush: the same bits, the oracle's
    counts, and the bars.  The mixed pool sizes for its range's worst case and refuses the rows listed by name in
    MIXED_POOL_REFUSES (tests/test_resample_rungs_host.py holds the list on the host) -- those rows must be refused, with
    the reason, and no other row may be; every form that serves the row has to agree."""
    name, arith = case
    row = BY_NAME[name]
    st = row.semitones
    rung, interp, _, big = row.want
    slot_rung = "vec8" if arith == FAST else "ref4"
    q = E.resample_rung(arith, 2, mode="normal_pitchshift", fftsize=FFT, semitones=st)
    slot_big = int(q["tab_bytes"] + 4 * q["lds_floats"] * (8 if arith == FAST else 4) > 64 * 1024)
    prev = _arith(arith)
    try:
        want, wcounts = oracle(0, 2, False, FFT, st)
        forms = {}
        E.chain_census(True)
        forms["engine"] = run_ragged(st)
        got = E.resample_census_read()
        # (the single-stream engine is always on the fused path: its resampling is a launch of its own)
        assert set(got) == {("batch", rung, interp, int(q["lds_bytes"] > 64 * 1024))}, (name, got)
        forms["batch"] = run_batch((0,), 2, FFT, st, flush=False)[0]
        E.chain_census(True)
        forms["pool"], counts = run_pool(st, mixed=False)
        census_is(f"{name} pool", ("pool", slot_rung, interp, slot_big))
        assert counts == list(wcounts), (name, counts, wcounts)
        E.chain_census(True)
        if case in MIXED_POOL_REFUSES:
            with pytest.raises(E.PvError) as e:
                run_pool(st, mixed=True)
            assert "stream pool range" in str(e.value) and "LDS" in str(e.value), str(e.value)
            assert E.resample_census_read() == {}
        else:
            forms["mixed_pool"] = run_pool(st, mixed=True)[0]
            got = E.resample_census_read()
            assert {k[:3] for k in got} == {("pmix", slot_rung, interp)}, (name, got)
        # (free-form: the mixed batch's own kernel, two rows for a stereo stream; in the reference's order it launches
        # the mixed pool's kernel, counted under that set)
        E.chain_census(True)
        forms["mixed_batch"] = run_mixed_batch(st)
        got = E.resample_census_read()
        assert {k[:3] for k in got} == {("mb", "vec2", interp) if arith == FAST else ("pmix", "ref4", interp)}, (name, got)
        assert len(forms) == (4 if case in MIXED_POOL_REFUSES else 5)
        for form, y in forms.items():
            assert y.shape == want.shape, (name, form, y.shape, want.shape)
            assert bits_equal(y, forms["engine"]), (name, form)
        held_to_the_oracle(f"{name} forms", forms["engine"], 0, 2, False, FFT, st, arith)
    finally:
        _arith(prev)


@pytest.mark.parametrize("arith", [E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
@pytest.mark.parametrize("fftsize", [2048, 256, 8192])
def test_plus_30_at_the_other_sizes(fftsize, arith, monkeypatch):
    """+30 st: 360 taps, oversampling 2.  fft 2048 is a wave-FFT size (the 8-row kernel above 64 KB under FAST); 256 and
    8192 take the generic route (frames from memory, launch_frames_chain) and resample in the reference's order under
    either setting."""
    st = 30.0
    want_rung = ("vec8", 1, 1) if (arith == FAST and fftsize == 2048) else ("ref4", 1, 0)
    prev = _arith(arith)
    try:
        q = E.resample_rung(arith, 6, mode="normal_pitchshift", fftsize=fftsize, semitones=st)
        assert (q["rung"], q["interp"], int(q["lds_bytes"] > 64 * 1024)) == want_rung and q["oversample"] == 2
        monkeypatch.setenv("AUDIOMOD_PV_FUSED", "2")
        E.chain_census(True)
        out = run_batch((0, 1, 2), 2, fftsize, st)
        census_is(f"+30 fft{fftsize} batch6", ("batch",) + want_rung)
        for s in (0, 2):
            held_to_the_oracle(f"+30 fft{fftsize} batch6 stream {s}", out[s], s, 2, True, fftsize, st, arith)
        monkeypatch.delenv("AUDIOMOD_PV_FUSED")
        y = run_ragged(st, fftsize, flush=True)   # (unflushed, 6000 frames at fft 8192 give silence only)
        held_to_the_oracle(f"+30 fft{fftsize} engine", y, 0, 2, True, fftsize, st, arith)
    finally:
        _arith(prev)


def _refused(make, st):
    with pytest.raises(E.PvError) as e:
        make()
    msg = str(e.value)
    assert "above the limit" in msg and "%+.2f semitones" % st in msg and "bytes of LDS" in msg, msg


@pytest.mark.parametrize("case", REFUSALS, ids=case_id)
def test_refused_rows_are_refused_everywhere_and_launch_nothing(case):
    name, arith = case
    st = BY_NAME[name].semitones
    prev = _arith(arith)
    try:
        kw = dict(mode="normal_pitchshift", fftsize=FFT, semitones=st)
        E.chain_census(True)
        _refused(lambda: E.PhaseVocoder(48000, 2, 1.0, st, E.NORMAL_SHIFT, E.PHASE_LOCKED, FFT), st)
        _refused(lambda: E.Batch(NSTEREO, FRAMES, channels=2, **kw), st)
        _refused(lambda: E.StreamPool(3, channels=2, **kw), st)
        _refused(lambda: E.HostIO(NSTEREO, FRAMES, channels=2, **kw), st)
        _refused(lambda: E.HostIO(NSTEREO, FRAMES, channels=2, launches_per_segment=2, **kw), st)
        for make in (lambda: E.StreamPool(3, channels=2, pitch_range=(0.0, st), mode="normal_pitchshift", fftsize=FFT),
                     lambda: E.MixedBatch([(FRAMES, st, 1.0)], channels=2, mode="normal_pitchshift", fftsize=FFT)):
            with pytest.raises(E.PvError) as e:   # the mixed forms' own checks
                make()
            assert "LDS" in str(e.value), str(e.value)
        assert E.resample_census_read() == {} and E.chain_census_read() == ({}, {}, {}) and E.phase_census_read() == {}
        # a pool at an accepted pitch still serves afterwards
        got, counts = run_pool(4.0, mixed=False)
        assert counts == list(oracle(0, 2, False, FFT, 4.0)[1])
        held_to_the_oracle(f"{name} pool afterwards", got, 0, 2, False, FFT, 4.0, arith)
    finally:
        _arith(prev)


def test_the_resample_census_file_receives_a_process_counts_at_exit(tmp_path):
    """AUDIOMOD_PV_RESAMPLE_CENSUS: the census is on from the start and the rung keys are appended to that file when the
    process ends, one line per key; AUDIOMOD_PV_CHAIN_CENSUS's file keeps the four kinds it always had"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rungs, chain = tmp_path / "rungs.txt", tmp_path / "chain.txt"
    rungs.write_text("kept\n")
    code = ("import sys; sys.path.insert(0, %r); from tests import test_resample_rungs_gpu as T; "
            "T.run_batch((0, 1, 2), 2, T.FFT, 30.0); T.run_pool(-24.0, mixed=False); print('census-child ok')" % (root,))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, AUDIOMOD_PV_RESAMPLE_CENSUS=str(rungs), AUDIOMOD_PV_CHAIN_CENSUS=str(chain)))
    assert r.returncode == 0 and "census-child ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    lines = rungs.read_text().splitlines()
    assert lines[0] == "kept"
    assert sorted(l.rsplit(" ", 1)[0] for l in lines[1:]) == ["resample_rung set=batch rung=vec8 interp=1 over64k=1",
                                                             "resample_rung set=pool rung=vec8 interp=0 over64k=0"], lines
    assert all(int(l.rsplit("count=", 1)[1]) > 0 for l in lines[1:]), lines
    kinds = {l.split(" ", 1)[0] for l in chain.read_text().splitlines()}
    assert kinds and kinds <= {"chain", "resample", "analyze", "phase"}, kinds
