"""Mixed batch, re-drawing in place (include/audiomod_pv.h pv_mbatch_redraw): a re-drawn object must be
indistinguishable from a freshly created one -- whose descriptors the host builds -- in every accessor, in the
per-sample descriptor arrays the device now builds, and in every output bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals
from tests.helpers import bits_equal

pytestmark = pytest.mark.gpu

# draw A (frames, semitones, time_ratio): a clip shorter than one frame, a stream that does not resample, +-12 st (direct
# tables), -5 / +4 / +7 st (interpolated, down and up), ratios 0.75 and 1.5, two clips of equal length
A = ((1, -12.0, 1.0), (479, -5.0, 1.0), (4097, 0.0, 1.0), (9000, 4.0, 1.0), (24000, 7.0, 0.75), (24000, 12.0, 1.5))
# draw B: the pitches moved over the clips, every length changed (the 1-frame clip to 6000, one to 1 frame, one
# shorter), the last two streams exact twins
B = ((6000, 7.0, 0.75), (1, 0.0, 1.0), (3001, -12.0, 1.0), (20011, 12.0, 1.5), (12000, -5.0, 1.0), (12000, -5.0, 1.0))
# draw C: four times A's total length, and a larger overlap-add advance than any of A's (ratio 2.0 at +12 st)
C_DRAW = ((60000, 12.0, 2.0), (50000, -5.0, 1.0), (40000, 0.0, 1.0), (40000, 7.0, 0.75), (30000, 4.0, 1.5), (30011, -12.0, 1.0))

CASES = {
    "fft512_cm0": (True, dict(fftsize=512, coremode=0)),
    "fft512_cm1": (True, dict(fftsize=512, coremode=1)),
    "fft512_cm2": (True, dict(fftsize=512, coremode=2)),
    "fft2048_cm1": (True, dict(fftsize=2048, coremode=1)),
    "formant_fft2048": (True, dict(mode="formant_pitchshift", fftsize=2048)),
    "robotic": (True, dict(mode="robotic", fftsize=1024)),
    "stretch_fft4096": (False, dict(mode="time_stretch", fftsize=4096)),
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


def _run(mb, streams):
    y = mb.run(mb.pack(_clips(streams)))
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in mb.split(y)]


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, f"{what}: stream {i} has shape {g.shape}, expected {w.shape}"
        assert bits_equal(g, w), f"{what}: stream {i} differs in {int((g.view(np.uint32) != w.view(np.uint32)).sum())} samples"


def _accessors(mb):
    n = len(mb.streams)
    L = mb.L
    assert L.pv_mbatch_nstreams(mb.h) == n
    direct = dict(out_frames=[L.pv_mbatch_out_frames(mb.h, i) for i in range(n)],
                  in_offsets=[L.pv_mbatch_in_offset(mb.h, i) for i in range(n)],
                  out_offsets=[L.pv_mbatch_out_offset(mb.h, i) for i in range(n)],
                  in_floats=L.pv_mbatch_in_floats(mb.h), out_floats=L.pv_mbatch_out_floats(mb.h),
                  launches=L.pv_mbatch_launches(mb.h), kernel_launches=L.pv_mbatch_kernel_launches(mb.h))
    for k, v in direct.items():  # the wrapper's cached copies follow the object
        assert getattr(mb, k) == v, k
    direct["info"] = [mb.info(i) for i in range(n)]
    return direct


def _assert_descriptors(got, want, what):
    """both kinds, every stream, byte for byte; names the first differing entry"""
    for i in range(len(want.streams)):
        for kind, name in ((E.DESC_WDEN, "denominators"), (E.DESC_OTAB, "output table")):
            g, w = got.debug_descriptors(i, kind), want.debug_descriptors(i, kind)
            assert g.shape == w.shape, f"{what}: stream {i} {name}: {g.size * 4} bytes, a created object has {w.size * 4}"
            bad = np.nonzero(g != w)[0]
            if len(bad):
                k = int(bad[0]) // (2 if kind == E.DESC_OTAB else 1)
                pytest.fail(f"{what}: stream {i} {name}: {len(bad)} words differ, first at entry {k}: "
                            f"{hex(int(g[bad[0]]))} for {hex(int(w[bad[0]]))}")


def _redrawn_against_created(name, first, second, what, descriptors=False, block=480, min_launches=0):
    flush, kw = CASES[name] if isinstance(name, str) else name
    mb = E.MixedBatch(first, channels=2, block=block, flush=flush, **kw)
    out_first = _run(mb, first)
    mb.redraw(second)
    got = _run(mb, second)
    fresh = E.MixedBatch(second, channels=2, block=block, flush=flush, **kw)
    assert _accessors(mb) == _accessors(fresh), what
    assert mb.launches >= min_launches
    if descriptors:
        _assert_descriptors(mb, fresh, what)
    _assert_same(got, _run(fresh, second), what)
    fresh.close()
    return mb, out_first


@pytest.mark.parametrize("name", sorted(CASES))
def test_redrawn_object_is_a_freshly_created_one(name, arith):
    mb, _ = _redrawn_against_created(name, A, B, name + ": A redrawn to B")
    t = mb.last_build_timing()
    assert t["plan_us"] > 0 and t["host_us"] > 0 and t["device_us"] > 0
    mb.close()


@pytest.mark.parametrize("name", ["fft512_cm1", "fft2048_cm1"])
def test_descriptors_equal_the_host_builders(name, arith):
    mb, _ = _redrawn_against_created(name, A, B, name + " descriptors", descriptors=True)
    mb.close()


@pytest.mark.parametrize("name", ["fft512_cm1", "fft2048_cm1"])
def test_many_launch_groups(name, arith, monkeypatch):
    monkeypatch.setenv("AUDIOMOD_PV_CHUNK_SLICES", "16")
    mb, _ = _redrawn_against_created(name, A, B, name + " in 16-slice groups", descriptors=True, min_launches=8)
    monkeypatch.delenv("AUDIOMOD_PV_CHUNK_SLICES")
    # the knob is the object's: a redraw without it in the environment still makes 16-slice groups
    n = mb.launches
    mb.redraw(B)
    assert mb.launches == n
    mb.close()


# an up-shift driven with calls larger than the reference's output ring: the plan drops slices (adv == 0)
DROP_KW, DROP_BLOCK = dict(fftsize=512, coremode=1), 12000
DROP_DRAW = ((24000, 5.0, 1.0), (36000, 5.0, 1.0), (24000, 7.0, 1.0), (479, 0.0, 1.0), (30000, 4.0, 1.5), (1, -12.0, 1.0))


def test_dropped_slices(arith):
    avail, _, _, info = E.plan_simulate([DROP_BLOCK, DROP_BLOCK], channels=2, semitones=5.0, **DROP_KW)
    assert avail.max() >= info["outbuf_capacity"] - 2 * info["fftsize"]  # the ring really fills up ...
    assert avail[1] < DROP_BLOCK - info["fftsize"]  # ... and output is lost: slices of the plan do not advance
    mb, _ = _redrawn_against_created((True, DROP_KW), A, DROP_DRAW, "dropped slices", descriptors=True, block=DROP_BLOCK)
    mb.close()


def test_back_again_and_growth(arith):
    name = "fft2048_cm1"
    flush, kw = CASES[name]
    mb, out_a = _redrawn_against_created(name, A, B, "A to B")
    mb.redraw(A)  # nothing stale survives the shrink to B
    _assert_same(_run(mb, A), out_a, "A again after B")
    assert sum(f for f, _, _ in C_DRAW) >= 4 * sum(f for f, _, _ in A)
    mb.redraw(C_DRAW)  # longer descriptors and a larger advance than the rings were sized for
    fresh = E.MixedBatch(C_DRAW, channels=2, flush=flush, **kw)
    assert _accessors(mb) == _accessors(fresh)
    _assert_descriptors(mb, fresh, "grown to C")
    _assert_same(_run(mb, C_DRAW), _run(fresh, C_DRAW), "grown to C")
    fresh.close()
    mb.redraw(A)
    _assert_same(_run(mb, A), out_a, "A again after C")
    mb.close()


NAN = float("nan")
REFUSALS = {
    "nan_pitch": (A[:2] + ((1000, NAN, 1.0),) + A[3:], 1, "stream 2: pitch / time ratio is not a finite number"),
    "frames0": (A[:4] + ((0, 4.0, 1.0),) + A[5:], 1, "stream 4: frames must be at least 1"),
    # (ten octaves up: what tests/test_mbatch_host.py uses for "a stream whose cfg_i the engine itself refuses")
    "engine_refuses": (A[:3] + ((9000, 120.0, 1.0),) + A[4:], None, "stream 3: the engine refuses this configuration"),
}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusals_change_nothing(which, arith):
    flush, kw = CASES["fft2048_cm1"]
    mb = E.MixedBatch(A, channels=2, flush=flush, **kw)
    want, before = _run(mb, A), _accessors(mb)
    streams, status, text = REFUSALS[which]
    if status is None:
        one = E.make_config(2, semitones=120.0, fftsize=2048)
        status = E.lib().pv_plan_simulate(C.byref(one), None, 0, None, None, None, 0, None, None)
        assert status != 0
    assert mb.L.pv_mbatch_redraw(mb.h, E._mixed_streams(streams)) == status
    msg = mb.L.pv_last_error().decode()
    assert msg.startswith("mixed batch") and text in msg, msg
    with pytest.raises(E.PvError, match="mixed batch"):
        mb.redraw(streams)
    assert mb.streams == [tuple(s) for s in A]
    assert _accessors(mb) == before
    _assert_same(_run(mb, A), want, "after the refused redraw")
    mb.close()


def test_redrawn_streams_equal_the_single_stream_engine():
    """the anchor outside the mixed batch: PV_ARITH_EXACT, every stream of the re-drawn object against run_offline"""
    prev = E.set_arithmetic(E.ARITH_EXACT)
    try:
        flush, kw = CASES["fft2048_cm1"]
        mb = E.MixedBatch(A, channels=2, flush=flush, **kw)
        mb.redraw(B)
        got = _run(mb, B)
        want = [E.run_offline(_clip(f, 300 + i), block=480, flush=flush, semitones=s, time_ratio=r, **kw)[0]
                for i, (f, s, r) in enumerate(B)]
        _assert_same(got, want, "redrawn against the single-stream engine")
        mb.close()
    finally:
        E.set_arithmetic(prev)
