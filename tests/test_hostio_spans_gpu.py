"""Host staging by time (include/audiomod_pv.h pv_hostio_create_segmented): one batch of all streams run in segments
through three window slots.  float32 on the wire: segmented == grouped HostIO == device-resident Batch, on the bits;
int16 on the wire: segmented == grouped (and both equal the reference's WAV writer applied to the batch's output).
Every job has more than three segments, so every window slot is reused; launches of 8 slices (AUDIOMOD_PV_CHUNK_SLICES)
give that on short inputs.  The staging memory of the segmented object does not depend on the job's length."""
import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals

pytestmark = pytest.mark.gpu

CHUNK = "8"
# name: (configuration, streams, frames, flush, launches per segment to try)
SHAPES = {
    "pitch_5_stereo": (dict(channels=2, semitones=4.0, coremode=1, fftsize=2048), 5, 30011, True, (1, 3)),
    "stretch_3_fft4096": (dict(channels=2, mode="time_stretch", time_ratio=1.5, fftsize=4096), 3, 30011, False, (2,)),
    "mono_4_fft1024": (dict(channels=1, semitones=-5.0, fftsize=1024), 4, 30011, True, (2,)),
}


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


@pytest.fixture(autouse=True)
def _chunks(monkeypatch):
    monkeypatch.setenv("AUDIOMOD_PV_CHUNK_SLICES", CHUNK)


def _voices(S, F, ch):
    """[S, ch, F] on the int16 grid, every stream its own voice"""
    return np.stack([signals.voice(F, ch, stream=s) for s in range(S)]).astype(np.float32)


def _to_i16(x):
    q = x.astype(np.float64) * 32768.0
    assert np.array_equal(q, np.round(q)) and q.min() >= -32768 and q.max() <= 32767, "the input is not on the int16 grid"
    return q.astype(np.int16)


def _equal(got, want):
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    u = np.uint32 if got.dtype == np.float32 else np.uint16
    return np.array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(want).view(u))


def _staged(x_wire, wire, passes=1, **kw):
    """x_wire [S, ch, F] through a HostIO object `passes` times, the output poisoned before each pass"""
    S, ch, F = x_wire.shape
    h = E.HostIO(S, F, wire=wire, **kw)
    hin, hout = h.pinned(x_wire.shape), h.pinned((S, ch, h.out_frames))
    hin[...] = x_wire
    outs = []
    for _ in range(passes):
        hout.view(np.uint8)[...] = 0xA5
        h.run(hin, hout)
        outs.append(hout.copy())
    h.close()
    return outs


def _device_resident(x, flush, **kw):
    b = E.Batch(x.shape[0], x.shape[2], flush=flush, **kw)
    torch.cuda.synchronize()
    out = b.run(torch.from_numpy(np.array(x, np.float32)).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    launches = b.launches
    b.close()
    return out, launches


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_float_wire_segmented_grouped_and_resident_agree(name, arith):
    kw, S, F, flush, per = SHAPES[name]
    x = _voices(S, F, kw["channels"])
    ref, launches = _device_resident(x, flush, **kw)
    assert launches > 3 * max(per), launches   # more than three segments: every slot is reused
    grouped = _staged(x, "f32", streams_per_group=2, flush=flush, **kw)[0]
    assert _equal(grouped, ref)
    for k in per:
        for p, got in enumerate(_staged(x, "f32", passes=2, launches_per_segment=k, flush=flush, **kw)):
            assert _equal(got, ref), f"{k} launches per segment, pass {p}"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_int16_wire_segmented_equals_grouped(name, arith):
    kw, S, F, flush, per = SHAPES[name]
    x = _voices(S, F, kw["channels"])
    x[0, 0, 5], x[0, 0, 6] = -1.0, 32767.0 / 32768.0      # -32768 and 32767 on the wire
    x[S - 1, -1, F - 1], x[S - 1, -1, F - 2] = -1.0, 32767.0 / 32768.0
    xi = _to_i16(x)
    assert xi.min() == -32768 and xi.max() == 32767
    ref, _ = _device_resident(x, flush, **kw)
    want = np.trunc(np.clip(ref * np.float32(32768.0), -32768.0, 32767.0)).astype(np.int16)
    grouped = _staged(xi, "i16", streams_per_group=2, flush=flush, **kw)[0]
    assert _equal(grouped, want)
    for k in per:
        got = _staged(xi, "i16", launches_per_segment=k, flush=flush, **kw)[0]
        assert _equal(got, grouped), f"{k} launches per segment"


def test_int16_saturation_agrees_with_the_grouped_path(arith):
    """ROBOTIC at 0 semitones on a full-scale square-ish signal: outputs exceed full scale, both ways, so the saturation
    of the conversion back runs on many samples."""
    S, F, kw = 3, 30011, dict(channels=2, mode="robotic", semitones=0.0, fftsize=2048)
    t = np.arange(F)
    x = np.empty((S, 2, F), np.float32)
    for s in range(S):
        for c in range(2):
            sq = np.where(((t + 17 * c) // (60 + 23 * s)) % 2 == 0, 1.0, -1.0)
            x[s, c] = np.clip(np.round(sq * 32768.0), -32768, 32767) / 32768.0
    xi = _to_i16(x)
    assert xi.min() == -32768 and xi.max() == 32767
    ref, launches = _device_resident(x, True, **kw)
    assert launches > 6
    over = int((np.abs(ref) * np.float32(32768.0) > 32767.0).sum())
    assert over > 100, over   # the input really drives the output past full scale
    grouped = _staged(xi, "i16", streams_per_group=1, **kw)[0]
    assert (grouped == 32767).any() and (grouped == -32768).any()
    for k in (1, 2):
        assert _equal(_staged(xi, "i16", launches_per_segment=k, **kw)[0], grouped), k


@pytest.mark.parametrize("wire", ["f32", "i16"])
def test_staging_memory_does_not_grow_with_the_length(wire):
    kw = dict(channels=2, semitones=4.0, coremode=1, fftsize=2048)
    size = {}
    for mode, arg in (("segmented", dict(launches_per_segment=2)), ("grouped", dict(streams_per_group=2))):
        for F in (30011, 60022):
            h = E.HostIO(5, F, wire=wire, **arg, **kw)
            size[(mode, F)] = h.staging_bytes()
            h.close()
    assert size[("segmented", 30011)] == size[("segmented", 60022)] > 0
    assert size[("grouped", 60022)] > size[("grouped", 30011)] > 0
    assert size[("segmented", 30011)] < size[("grouped", 30011)]
