"""The host-staged path (include/audiomod_pv.h pv_hostio_*, audiomod_amd/csrc/pv_hostio.hip): groups of streams go
through three buffer slots on three HIP streams -- copy-in, kernels, copy-out -- and the only guard against a slot
being overwritten while it is still read or copied out is the event waits of groups g >= 3 in pv_hostio_run.  Here
every job has more than three groups, so every slot is reused and every one of those waits executes; every stream is
its own signal, so an early overwrite shows as another stream's audio.

The reference of each case is the device-resident Batch of the same configuration on the same input: float32 on the
wire is bit-equal to it, int16 on the wire equals trunc(clip(ref * 32768, -32768, 32767)) (the reference's WAV writer:
main/wavfile.cc:1295-1306,1334-1342)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals

pytestmark = pytest.mark.gpu

F = 24000
PITCH = dict(semitones=4.0, coremode=1, fftsize=2048)


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


@functools.lru_cache(maxsize=None)
def _voices(nstreams, frames, channels, first=0):
    """[nstreams, channels, frames] on the int16 grid, every stream its own voice"""
    x = np.stack([signals.voice(frames, channels, stream=first + s) for s in range(nstreams)])
    x.setflags(write=False)
    return x


def _device_resident(x, **kw):
    """what Batch writes for x [nstreams, channels, frames] (the whole batch at once, synchronously)"""
    b = E.Batch(x.shape[0], x.shape[2], channels=x.shape[1], **kw)
    torch.cuda.synchronize()
    out = b.run(torch.from_numpy(np.array(x, np.float32)).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    b.close()
    return out


def _to_wire(x, wire):
    if wire == "f32":
        return np.ascontiguousarray(x, np.float32)
    q = x.astype(np.float64) * 32768.0
    assert np.array_equal(q, np.round(q)) and q.min() >= -32768 and q.max() <= 32767, "the input is not on the int16 grid"
    return q.astype(np.int16)


def _expected(ref, wire):
    if wire == "f32":
        return ref
    return np.trunc(np.clip(ref * np.float32(32768.0), -32768.0, 32767.0)).astype(np.int16)


def _equal(got, want):
    """bit for bit, either wire type"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    u = np.uint32 if got.dtype == np.float32 else np.uint16
    return np.array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(want).view(u))


def _wrong_streams(got, want):
    return [s for s in range(want.shape[0]) if not _equal(got[s], want[s])]


def _staged(x, wire, per_group, passes=1, pinned=True, **kw):
    """x through a HostIO object `passes` times, the output buffer poisoned before each; returns the outputs"""
    S, ch, frames = x.shape
    h = E.HostIO(S, frames, channels=ch, streams_per_group=per_group, wire=wire, **kw)
    if pinned:
        hin, hout = h.pinned(x.shape), h.pinned((S, ch, h.out_frames))
    else:
        hin, hout = np.empty(x.shape, h.dtype), np.empty((S, ch, h.out_frames), h.dtype)
    hin[...] = _to_wire(x, wire)
    outs = []
    for _ in range(passes):
        hout.view(np.uint8)[...] = 0xA5
        h.run(hin, hout)
        outs.append(hout.copy())
    h.close()
    return outs


def _check(x, wire, per_group, passes=1, pinned=True, **kw):
    want = _expected(_device_resident(x, **kw), wire)
    for k, got in enumerate(_staged(x, wire, per_group, passes=passes, pinned=pinned, **kw)):
        assert got.shape == want.shape
        assert _equal(got, want), f"pass {k}: streams {_wrong_streams(got, want)} differ from the device-resident batch"
    return want


# ---- slot reuse -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", ["f32", "i16"])
@pytest.mark.parametrize("nstreams,per_group", [(15, 2), (7, 1)], ids=["15_by_2", "7_by_1"])
def test_every_slot_reused(nstreams, per_group, wire, arith):
    """15 streams in groups of 2: 8 groups, every slot reused at least twice, a one-stream last group; 7 in groups of 1.
    Two passes over one object.

    This test is probabilistic against a missing wait: without it a slot is overwritten early only if the device lags
    the host by three groups at that moment.  A library built without the two `g >= kSlots` waits of pv_hostio_run
    (the upload's wait for ev_run, the run's wait for ev_down), run twice against this file on an MI355X: 4 and 5 failing
    cases, all of them here -- 15_by_2 in 7 of its 8 runs, 7_by_1 in 1 of 8 -- each time in the streams of the last
    groups (stream 8, overwritten by the one-stream last group's upload; once streams 6-8), in one of the two passes.
    Four times the frames did not make it more likely (1 of 4)."""
    assert (nstreams + per_group - 1) // per_group >= 7
    _check(_voices(nstreams, F, 2), wire, per_group, passes=2, **PITCH)


# ---- group edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", ["f32", "i16"])
@pytest.mark.parametrize("nstreams,per_group", [(3, 8), (3, 3), (1, 1), (1, 16)],
                         ids=["group_larger_clamped", "group_equal", "one_stream", "one_stream_group_16"])
def test_group_edges(nstreams, per_group, wire, arith):
    _check(_voices(nstreams, F, 2), wire, per_group, passes=2, **PITCH)


# ---- stale rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", ["f32", "i16"])
def test_nothing_stale_survives_a_run(wire, arith):
    """One object, run(x1), run(x2), run(x1): the third result is the first; where x2 repeats x1's streams (0..K-1) the
    middle run repeats the first's rows, elsewhere it gives x2's.  7 streams in groups of 2: the last group is one stream
    short, its surplus row computes on whatever the slot held -- which must reach neither the last stream's output nor
    the host buffer behind it."""
    S, K, per_group = 7, 3, 2
    x1 = _voices(S, F, 2)
    x2 = np.concatenate([x1[:K], _voices(S - K, F, 2, first=40)])
    want1, want2 = (_expected(_device_resident(x, **PITCH), wire) for x in (x1, x2))
    assert _equal(want2[:K], want1[:K]) and not any(_equal(want2[s], want1[s]) for s in range(K, S))
    h = E.HostIO(S, F, channels=2, streams_per_group=per_group, wire=wire, **PITCH)
    hin = h.pinned(x1.shape)
    guarded = h.pinned((S + 1, 2, h.out_frames))  # one row more than the job writes
    hout = guarded[:S]
    got = []
    for x in (x1, x2, x1):
        hin[...] = _to_wire(x, wire)
        guarded.view(np.uint8)[...] = 0xA5
        h.run(hin, hout)
        assert (guarded[S].view(np.uint8) == 0xA5).all(), "the short last group wrote its surplus row to the host"
        got.append(hout.copy())
    h.close()
    assert _equal(got[0], want1), f"first run: streams {_wrong_streams(got[0], want1)}"
    assert _equal(got[1], want2), f"middle run: streams {_wrong_streams(got[1], want2)}"
    assert _equal(got[1][:K], got[0][:K])
    assert _equal(got[2], got[0]), f"third run: streams {_wrong_streams(got[2], got[0])}"


# ---- saturation -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _full_scale_noise(nstreams):
    x = np.stack([np.random.default_rng(5 + s).uniform(-1, 1, (2, F)) for s in range(nstreams)])
    x = (np.clip(np.round(x * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("kw", [dict(semitones=4.0, fftsize=2048), dict(semitones=-7.0, fftsize=512)],
                         ids=["up4_fft2048", "down7_fft512"])
def test_int16_saturates_as_the_wav_writer(kw, arith):
    """Full-scale uniform noise on the int16 grid: the output overshoots both rails (the oracle alone, one stream of seed
    5: 442 / 432 samples beyond the upper / lower rail at +4 st, 382 / 388 at -7 st, peak 1.87), so both saturating
    branches of pv_f32_to_i16 decide samples.  7 streams in groups of 2: the slots are reused as well."""
    x = _full_scale_noise(7)
    ref = _device_resident(x, **kw)
    scaled = ref.astype(np.float64) * 32768.0
    above, below = int((scaled > 32767.0).sum()), int((scaled < -32768.0).sum())
    assert above >= 100 and below >= 100, (above, below)
    want = _expected(ref, "i16")
    assert int((want == 32767).sum()) >= above and int((want == -32768).sum()) >= below
    got = _staged(x, "i16", 2, **kw)[0]
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{len(bad)} samples differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} for "
                           f"{want[tuple(bad[0])]} (float {ref[tuple(bad[0])]!r})")


# ---- unpinned memory --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wire", ["f32", "i16"])
def test_ordinary_host_memory_gives_the_same_bits(wire, arith):
    _check(_voices(7, F, 2), wire, 2, passes=2, pinned=False, **PITCH)


# ---- other shapes, each in groups that force reuse --------------------------------------------------------------------
SHAPES = {
    "no_flush": (2, dict(PITCH, flush=False)),
    "block_64": (2, dict(PITCH, block=64)),
    "block_4724": (2, dict(PITCH, block=4724)),
    "stretch_fft4096": (2, dict(mode="time_stretch", time_ratio=1.5, fftsize=4096, flush=False)),
    "mono": (1, dict(PITCH)),
    "three_channels": (3, dict(PITCH)),
}


@pytest.mark.parametrize("wire", ["f32", "i16"])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_other_shapes(name, wire, arith):
    channels, kw = SHAPES[name]
    want = _check(_voices(7, F, channels), wire, 2, **kw)
    if name == "stretch_fft4096":
        assert want.shape[2] != F  # out_frames != frames


@pytest.mark.parametrize("wire", ["f32", "i16"])
def test_a_job_without_output(wire, arith):
    """Shorter than one FFT frame and no flush: zero output frames is a valid job (tests/test_gpu_parity.py
    test_batch_with_no_output_at_all), in groups that reuse the slots, and needs no output buffer."""
    kw = dict(flush=False, semitones=7.04, fftsize=8192)
    h = E.HostIO(7, 1482, channels=2, streams_per_group=2, wire=wire, **kw)
    assert h.out_frames == 0
    hin = h.pinned((7, 2, 1482))
    hin[...] = _to_wire(_voices(7, 1482, 2), wire)
    assert h.L.pv_hostio_run(h.h, hin.ctypes.data, None) == 0
    out = h.run(hin)
    assert out.shape == (7, 2, 0)
    h.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["nstreams0", "frames0", "group0", "wire2", "null_config"])
def test_refusals(what):
    a = dict(nstreams=4, frames=F, per_group=2, wire=0)
    a.update({"nstreams0": dict(nstreams=0), "frames0": dict(frames=0), "group0": dict(per_group=0),
              "wire2": dict(wire=2), "null_config": {}}[what])
    cfg = E.make_config(2, **PITCH)
    L = E.lib()
    h = C.c_void_p()
    st = L.pv_hostio_create(None if what == "null_config" else C.byref(cfg), a["nstreams"], a["frames"], 480, 1, 0,
                            a["per_group"], a["wire"], C.byref(h))
    assert st == 1  # PV_ERR_INVALID_ARG
    assert not h.value
