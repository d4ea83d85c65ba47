"""Mixed batch on the GPU (include/audiomod_pv.h pv_mbatch_*): every stream of a MixedBatch must come out bit for bit as
the single-stream engine of its own configuration writes it -- whatever the other streams' lengths and pitches, however
many launch groups the run takes, and run after run."""
import functools

import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import bits_equal, rel_rms

pytestmark = pytest.mark.gpu

# (frames, semitones, time_ratio): a clip shorter than one frame, a stream that does not resample beside ones that do,
# +-12 st (direct tables) beside interpolated ones, two streams of equal length at different pitches
STREAMS = ((1, -12.0, 1.0), (479, -5.0, 1.0), (4097, 0.0, 1.0), (9000, 4.0, 1.0), (24000, 7.0, 0.75), (24000, 12.0, 1.5))

CASES = {
    "fft512_cm0": (STREAMS, True, dict(fftsize=512, coremode=0)),
    "fft512_cm1": (STREAMS, True, dict(fftsize=512, coremode=1)),
    "fft512_cm2": (STREAMS, True, dict(fftsize=512, coremode=2)),
    "fft2048_cm1": (STREAMS, True, dict(fftsize=2048, coremode=1)),
    "gender_fft2048": (STREAMS + ((6000, -7.0, 1.0),), True, dict(mode="gender_change", fftsize=2048)),
    "formant_fft2048": (STREAMS + ((6000, 7.0, 1.0),), True, dict(mode="formant_pitchshift", fftsize=2048)),
    "robotic": (STREAMS, True, dict(mode="robotic", fftsize=1024)),
    # time_stretch is the mode the CLI loop runs without a flush (include/audiomod_pv.h, batch engine: flush == 0), so
    # that is how it is driven here; the same streams with the flush on cover flush + time ratio at this size too
    "stretch_fft4096": (STREAMS, False, dict(mode="time_stretch", fftsize=4096)),
    "stretch_fft4096_flush": (STREAMS, True, dict(mode="time_stretch", fftsize=4096)),
}


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


@functools.lru_cache(maxsize=None)
def _clip(frames, seed):
    x = signals.voice(frames, 2, seed=seed)
    x.setflags(write=False)
    return x


def _clips(streams, seed0=300):
    return [_clip(f, seed0 + i) for i, (f, _, _) in enumerate(streams)]


@functools.lru_cache(maxsize=None)
def _single(frames, seed, semitones, ratio, flush, block, arith, cfg):
    """what the single-stream engine writes for one clip (computed once per distinct stream and setting)"""
    assert E.get_arithmetic() == arith
    y = E.run_offline(_clip(frames, seed), block=block, flush=flush, semitones=semitones, time_ratio=ratio, **dict(cfg))[0]
    y.setflags(write=False)
    return y


def _refs(streams, flush, kw, block=480, seed0=300):
    a = E.get_arithmetic()
    return [_single(f, seed0 + i, s, r, flush, block, a, tuple(sorted(kw.items()))) for i, (f, s, r) in enumerate(streams)]


def _run(mb, clips):
    y = mb.run(mb.pack(clips))
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in mb.split(y)]


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, f"{what}: stream {i} has shape {g.shape}, expected {w.shape}"
        assert bits_equal(g, w), f"{what}: stream {i} differs in {int((g.view(np.uint32) != w.view(np.uint32)).sum())} samples"


@pytest.mark.parametrize("name", sorted(CASES))
def test_streams_match_single_stream_engine(name, arith):
    streams, flush, kw = CASES[name]
    mb = E.MixedBatch(streams, channels=2, flush=flush, **kw)
    assert mb.out_frames == [w.shape[1] for w in _refs(streams, flush, kw)]
    _assert_same(_run(mb, _clips(streams)), _refs(streams, flush, kw), name)
    mb.close()


def test_block_64_matches_single_stream_engine():
    kw = dict(fftsize=512, coremode=1)
    mb = E.MixedBatch(STREAMS, channels=2, block=64, **kw)
    _assert_same(_run(mb, _clips(STREAMS)), _refs(STREAMS, True, kw, block=64), "block 64")
    mb.close()


@pytest.mark.parametrize("name", ["fft512_cm1", "fft2048_cm1", "fft512_cm0"])
def test_many_launch_groups_and_streams_ending_at_different_groups(name, monkeypatch):
    streams, flush, kw = CASES[name]
    whole = E.MixedBatch(streams, channels=2, flush=flush, **kw)
    monkeypatch.setenv("AUDIOMOD_PV_CHUNK_SLICES", "16")
    mb = E.MixedBatch(streams, channels=2, flush=flush, **kw)
    monkeypatch.delenv("AUDIOMOD_PV_CHUNK_SLICES")
    assert mb.launches >= 8 and mb.launches > whole.launches
    assert mb.out_frames == whole.out_frames
    got = _run(mb, _clips(streams))
    _assert_same(got, _refs(streams, flush, kw), name + " in 16-slice groups")
    _assert_same(got, _run(whole, _clips(streams)), name + " in 16-slice groups against whole launches")
    mb.close(), whole.close()


@pytest.mark.parametrize("chunk", [None, "16"], ids=["whole", "chunk16"])
def test_run_twice(chunk, monkeypatch):
    streams, flush, kw = CASES["fft2048_cm1"]
    if chunk:
        monkeypatch.setenv("AUDIOMOD_PV_CHUNK_SLICES", chunk)
    mb = E.MixedBatch(streams, channels=2, flush=flush, **kw)
    want = _refs(streams, flush, kw)
    d_in = mb.pack(_clips(streams))
    d_out = mb.alloc_out()
    for k in range(2):  # the same input: the same bits (state reset, both accumulator halves)
        d_out.fill_(float("nan"))
        mb.run(d_in, d_out)
        torch.cuda.synchronize()
        _assert_same([v.cpu().numpy() for v in mb.split(d_out)], want, f"run {k}")
    # other input through the same object: that input's bits
    _assert_same(_run(mb, _clips(streams, seed0=700)), _refs(streams, flush, kw, seed0=700), "second input")
    _assert_same(_run(mb, _clips(streams)), want, "first input again")
    mb.close()


def test_order_independence():
    streams, flush, kw = CASES["fft2048_cm1"]
    fwd = E.MixedBatch(streams, channels=2, flush=flush, **kw)
    rev = E.MixedBatch(streams[::-1], channels=2, flush=flush, **kw)
    assert rev.out_frames == fwd.out_frames[::-1]
    clips = _clips(streams)
    _assert_same(_run(rev, clips[::-1])[::-1], _run(fwd, clips), "reversed stream list")
    fwd.close(), rev.close()


def test_uniform_streams_equal_the_batch_engine():
    F, kw = 24000, dict(fftsize=2048, coremode=1)
    x = signals.synthetic_batch(torch, 5, F, "cuda:0")
    batch = E.Batch(5, F, channels=2, semitones=4.0, **kw)
    want = batch.run(x)
    mb = E.MixedBatch([(F, 4.0, 1.0)] * 5, channels=2, **kw)
    got = mb.split(mb.run(x.reshape(-1)))
    torch.cuda.synchronize()
    assert mb.out_frames == [batch.out_frames] * 5
    _assert_same([g.cpu().numpy() for g in got], [want[i].cpu().numpy() for i in range(5)], "uniform batch")
    batch.close(), mb.close()


def test_against_oracle():
    """BASELINE's contract: 1e-4 RMS against the oracle, stream by stream"""
    streams, flush, kw = CASES["fft2048_cm1"]
    got = _run(E.MixedBatch(streams, channels=2, flush=flush, **kw), _clips(streams))
    for i in (1, 3):  # -5 st and +4 st
        f, s, r = streams[i]
        want = O.run_offline(_clip(f, 300 + i), semitones=s, time_ratio=r, **kw)[0]
        assert got[i].shape == want.shape
        assert rel_rms(got[i], want) <= 1e-4, (i, rel_rms(got[i], want))


def test_launch_count_does_not_grow_with_the_pitches():
    """25 streams at 25 pitches against 25 streams at one: a launch group launches each stage once per kernel variant
    present -- analysis, match, rotation chain, at most two fused kernels (resampling or not) and two resampling kernels
    (direct or interpolated table) here, so at most 7 kernels per group however many pitches -- and the number of groups
    follows the longest stream's slice count (+12 st has the smallest hop: 16 / 10.08 of +4 st's slices)."""
    F, kw = 48000, dict(fftsize=512, coremode=1)
    many = E.MixedBatch([(F, float(s), 1.0) for s in range(-12, 13)], channels=2, **kw)
    one = E.MixedBatch([(F, 4.0, 1.0)] * 25, channels=2, **kw)
    assert many.launches <= 2 * one.launches, (many.launches, one.launches)
    assert one.kernel_launches <= 5 * one.launches  # analysis, match, chain, fused, resampling
    assert many.kernel_launches <= 7 * many.launches
    many.close(), one.close()
