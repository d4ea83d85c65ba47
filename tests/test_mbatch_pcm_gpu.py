"""PCM wire of the mixed batch on the GPU (include/audiomod_pv.h pv_mbatch_run_pcm): the two conversion kernels swept
value by value against the WAV reader's and writer's expressions in numpy, and run_pcm against the host-converted run,
bit for bit -- d_pcm_out is the writer's conversion of what MixedBatch.run writes for the reader's conversion of
d_pcm_in, and the padding between clips is never touched."""
import functools

import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals
from tests.test_mbatch_pcm_host import expected_layout

pytestmark = pytest.mark.gpu

DEPTHS = (16, 8, 24, 32)
# (frames, semitones, time_ratio): around one 16-byte piece of stereo int16 (8 samples), a clip shorter than a block, one
# that ends just behind a conversion tile (4096 samples), one behind two, a long one with a time ratio
STREAMS = ((1, -12.0, 1.0), (7, 0.0, 1.0), (8, 4.0, 1.0), (9, 4.0, 1.0), (479, -5.0, 1.0), (2049, 0.0, 1.0),
           (4097, 7.0, 1.0), (9000, 12.0, 0.75))
FOUR = (STREAMS[0], STREAMS[3], STREAMS[5], STREAMS[6])
CFG = dict(fftsize=512, coremode=1)
PATTERN = 0xA5


# ------------------------------------------------------------------ the reader's and the writer's expressions
def reader(x, bits):
    """WavIn::read: (float)(integer * 2^-k) in double (8 bit: minus one)"""
    x = np.asarray(x).astype(np.float64)
    if bits == 8:
        return (x * (1.0 / 128.0) - 1.0).astype(np.float32)
    return (x * (1.0 / float(1 << (bits - 1)))).astype(np.float32)


def writer(x):
    """WavOut16::write: saturate(x * 32768, -32768, 32767) in float, truncated toward zero"""
    v = np.asarray(x, np.float32) * np.float32(32768.0)
    return np.trunc(np.clip(v, np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)


def _as_clip(values, channels):
    """a 1-D value array as [frames][channels], the last frame filled up with the first values"""
    pad = (-len(values)) % channels
    v = np.concatenate([values, values[:pad]]) if pad else values
    return v.reshape(-1, channels)


def _sweep_ingest(values, bits, channels):
    clip = _as_clip(values, channels)
    got = E.debug_pcm_ingest(clip, bits)
    want = np.ascontiguousarray(reader(clip, bits).T)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad[0]) == 0, (bits, channels, len(bad[0]), clip.T[bad][:4], got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_ingest_every_8_16_and_24_bit_value(channels):
    _sweep_ingest(np.arange(256, dtype=np.int32), 8, channels)
    _sweep_ingest(np.arange(-32768, 32768, dtype=np.int32), 16, channels)
    _sweep_ingest(np.arange(-(1 << 23), 1 << 23, dtype=np.int32), 24, channels)


@pytest.mark.parametrize("chunk", range(8))
def test_ingest_32_bit_values_around_every_multiple_of_2_to_the_7_and_up(chunk):
    """Every value within 4 of a multiple of 2^k, k = 7 ... 31, both signs (the multiples of 2^7 contain the others), in
    eight chunks of the range and with the extremes; every value is swept once, the chunks taking 1, 2 and 3 channels
    in turn."""
    per = 1 << 22
    j = np.arange(-(1 << 24) + chunk * per, -(1 << 24) + (chunk + 1) * per + (1 if chunk == 7 else 0), dtype=np.int64)
    v = (j[:, None] * 128 + np.arange(-4, 5, dtype=np.int64)[None, :]).reshape(-1)
    v = v[(v >= -(1 << 31)) & (v < (1 << 31))]
    if chunk in (0, 7):
        v = np.concatenate([v, np.array([-(1 << 31), -(1 << 31) + 1, (1 << 31) - 2, (1 << 31) - 1], np.int64)])
    _sweep_ingest(v.astype(np.int32), 32, 1 + chunk % 3)


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_ingest_32_bit_random_values(channels):
    """2^26 seeded random values, a third of them per channel count"""
    rng = np.random.default_rng(2600 + channels)
    v = rng.integers(-(1 << 31), 1 << 31, size=(1 << 26) // 3 + 1, dtype=np.int64).astype(np.int32)
    _sweep_ingest(v, 32, channels)


@functools.lru_cache(maxsize=None)
def _writer_values():
    k = np.arange(-32769, 32769, dtype=np.float64)
    f = (k / 32768.0).astype(np.float32)
    den = np.float32(1e-45)
    special = np.array([0.0, -0.0, den, -den, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 1.5, -1.5, 3e38, -3e38,
                        np.inf, -np.inf], np.float32)
    v = np.concatenate([f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf)), special])
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_egress_on_every_int16_boundary_and_the_special_values(channels):
    clip = _as_clip(_writer_values(), channels)  # [frames][channels]
    with np.errstate(over="ignore"):
        want = writer(clip)
    got = E.debug_pcm_egress(np.ascontiguousarray(clip.T))
    bad = np.nonzero(got != want)
    assert len(bad[0]) == 0, (channels, len(bad[0]), clip[bad][:4], got[bad][:4], want[bad][:4])


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_piece_and_group_edges(channels):
    """frame counts around one piece, one 24-bit group and one tile, at every depth and both ways"""
    rng = np.random.default_rng(77 + channels)
    for frames in (1, 7, 8, 9, 15, 16, 17, 2049):
        for bits in DEPTHS:
            lo, hi = (0, 256) if bits == 8 else (-(1 << (bits - 1)), 1 << (bits - 1))
            clip = rng.integers(lo, hi, size=(frames, channels), dtype=np.int64)
            got = E.debug_pcm_ingest(clip, bits)
            want = reader(clip, bits).T
            assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), (frames, bits)
        x = rng.uniform(-1.2, 1.2, size=(channels, frames)).astype(np.float32)
        assert np.array_equal(E.debug_pcm_egress(x), writer(x.T)), frames


# ------------------------------------------------------------------ run_pcm against the host-converted run
@functools.lru_cache(maxsize=None)
def _pcm_clip(frames, channels, bits, seed):
    """integer samples [frames][channels] of a voice-like signal at `bits` bits, the low bits below int16 filled"""
    v = signals.voice(frames, channels, seed=seed, dtype=np.float64).T
    rng = np.random.default_rng(seed)
    if bits == 8:
        x = np.clip(np.round(v * 128.0) + 128, 0, 255)
    elif bits == 16:
        x = np.round(v * 32768.0)
    else:
        x = np.round(v * 32768.0) * (1 << (bits - 16)) + rng.integers(0, 1 << (bits - 16), size=v.shape)
    x = np.ascontiguousarray(x.astype(np.int64))
    x.setflags(write=False)
    return x


def _clips(streams, channels, bits, seed0=500):
    return [_pcm_clip(f, channels, b, seed0 + i) for i, ((f, _, _), b) in enumerate(zip(streams, bits))]


def _cycle(streams):
    return [DEPTHS[i % 4] for i in range(len(streams))]


def _reference(mb, clips, bits):
    """the writer's conversion of what run() writes for the reader's conversion of the clips"""
    y = mb.run(mb.pack([reader(x, b).T for x, b in zip(clips, bits)]))
    torch.cuda.synchronize()
    return [writer(v.cpu().numpy().T) for v in mb.split(y)]


def _run_pcm(mb, clips, bits, **kw):
    """run_pcm into a pattern-filled buffer: the clips' int16 arrays, after checking that the padding kept the pattern"""
    out = torch.full((mb.pcm_layout(bits)["out_bytes"],), PATTERN, dtype=torch.uint8, device="cuda")
    mb.run_pcm(mb.pack_pcm(clips, bits), bits, out, **kw)
    torch.cuda.synchronize()
    return _split_checked(mb, out.cpu().numpy())


def _split_checked(mb, raw):
    lay = mb.pcm_layout()
    used = np.zeros(len(raw), bool)
    for o, f in zip(lay["out_offsets"], mb.out_frames):
        used[o:o + 2 * mb.channels * f] = True
    assert np.all(raw[~used] == PATTERN), "padding bytes between clips were written"
    return [v.copy() for v in mb.split_pcm(raw)]


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, f"{what}: stream {i} has shape {g.shape}, expected {w.shape}"
        assert np.array_equal(g, w), f"{what}: stream {i} differs in {int((g != w).sum())} samples"


@pytest.fixture
def exact():
    prev = E.set_arithmetic(E.ARITH_EXACT)
    yield
    E.set_arithmetic(prev)


def _case(streams, channels, flush=True, **kw):
    cfg = dict(CFG, **kw)
    mb = E.MixedBatch(streams, channels=channels, flush=flush, **cfg)
    bits = _cycle(streams)
    clips = _clips(streams, channels, bits)
    lay = mb.pcm_layout(bits)
    assert lay == expected_layout([f for f, _, _ in streams], mb.out_frames, channels, bits)
    _assert_same(_run_pcm(mb, clips, bits), _reference(mb, clips, bits), f"{channels} channels {kw}")
    mb.close()


def test_run_pcm_is_the_converted_run_stereo_fast():
    assert E.get_arithmetic() == E.ARITH_FAST
    _case(STREAMS, 2)


def test_run_pcm_is_the_converted_run_stereo_exact(exact):
    _case(STREAMS, 2)


@pytest.mark.parametrize("channels", [1, 3])
def test_run_pcm_is_the_converted_run_mono_and_three_channels(channels):
    _case(FOUR, channels)


def test_run_pcm_time_stretch_without_a_flush():
    streams = ((479, 0.0, 1.5), (2049, 0.0, 0.75), (4097, 0.0, 1.25), (9000, 0.0, 2.0))
    _case(streams, 2, flush=False, mode="time_stretch")


def test_run_pcm_depths_all_equal_and_default():
    """in_bits = NULL is 16 bits for every clip; one depth for all"""
    mb = E.MixedBatch(FOUR, channels=2, **CFG)
    for bits in (None, 24):
        lst = [bits or 16] * len(FOUR)
        clips = _clips(FOUR, 2, lst)
        out = torch.full((mb.pcm_layout(bits)["out_bytes"],), PATTERN, dtype=torch.uint8, device="cuda")
        mb.run_pcm(mb.pack_pcm(clips, bits), bits, out)
        torch.cuda.synchronize()
        _assert_same(_split_checked(mb, out.cpu().numpy()), _reference(mb, clips, lst), f"bits {bits}")
    mb.close()


def test_run_pcm_run_run_pcm_give_the_same_bits():
    mb = E.MixedBatch(STREAMS, channels=2, **CFG)
    bits = _cycle(STREAMS)
    clips = _clips(STREAMS, 2, bits)
    first = _run_pcm(mb, clips, bits)
    want = _reference(mb, clips, bits)  # (a float run in between)
    second = _run_pcm(mb, clips, bits)
    _assert_same(first, want, "first PCM run")
    _assert_same(second, want, "PCM run after a float run")
    other = [DEPTHS[(i + 1) % 4] for i in range(len(STREAMS))]  # other depths on the same object: a new job table
    clips2 = _clips(STREAMS, 2, other)
    _assert_same(_run_pcm(mb, clips2, other), _reference(mb, clips2, other), "other depths")
    _assert_same(_run_pcm(mb, clips, bits), want, "the first depths again")
    mb.close()


def test_run_pcm_after_a_redraw_equals_a_fresh_object():
    mb = E.MixedBatch(FOUR, channels=2, **CFG)
    bits = _cycle(FOUR)
    _run_pcm(mb, _clips(FOUR, 2, bits), bits)
    drawn = ((9000, 3.0, 1.0), (8, -4.0, 1.0), (4097, 12.0, 0.75), (17, 0.0, 1.0))  # longer in total: the buffers grow
    mb.redraw(drawn)
    fresh = E.MixedBatch(drawn, channels=2, **CFG)
    clips = _clips(drawn, 2, bits, seed0=900)
    assert mb.pcm_layout(bits) == fresh.pcm_layout(bits)
    got = _run_pcm(mb, clips, bits)
    _assert_same(got, _run_pcm(fresh, clips, bits), "redrawn against fresh")
    _assert_same(got, _reference(fresh, clips, bits), "redrawn against the converted run")
    mb.redraw(FOUR)  # and back to a shorter draw: nothing shrinks, the offsets follow
    clips = _clips(FOUR, 2, bits)
    _assert_same(_run_pcm(mb, clips, bits), _reference(mb, clips, bits), "second redraw")
    mb.close(), fresh.close()


def test_run_pcm_host_equals_run_pcm():
    mb = E.MixedBatch(STREAMS, channels=2, **CFG)
    bits = _cycle(STREAMS)
    clips = _clips(STREAMS, 2, bits)
    want = _run_pcm(mb, clips, bits)
    h_in = mb.pack_pcm_host(clips, bits)
    h_out = np.full(mb.pcm_layout(bits)["out_bytes"], PATTERN, np.uint8)
    mb.run_pcm_host(h_in, bits, h_out)
    _assert_same([v.copy() for v in mb.split_pcm(h_out)], want, "pageable host buffers")
    pin_in = torch.from_numpy(h_in).pin_memory()
    pin_out = torch.zeros(len(h_out), dtype=torch.uint8).pin_memory()
    mb.run_pcm_host(pin_in, bits, pin_out)
    _assert_same([v.copy() for v in mb.split_pcm(pin_out.numpy())], want, "page-locked host buffers")
    mb.close()


def test_run_pcm_takes_its_input_from_the_stream_it_is_given():
    """pv_mbatch_run's ordering rule: the input is whatever an operation enqueued just before on the same stream leaves"""
    mb = E.MixedBatch(STREAMS, channels=2, **CFG)
    bits = _cycle(STREAMS)
    clips = _clips(STREAMS, 2, bits)
    want = _run_pcm(mb, clips, bits)
    packed = mb.pack_pcm(clips, bits)
    d_in = torch.zeros_like(packed)
    out = torch.full((mb.pcm_layout(bits)["out_bytes"],), PATTERN, dtype=torch.uint8, device="cuda")
    a = torch.ones(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(8):  # work that keeps the stream busy, then the copy that fills the input
            a = a @ a * 1e-4
        d_in.copy_(packed, non_blocking=True)
        mb.run_pcm(d_in, bits, out, stream=s)
    s.synchronize()
    _assert_same(_split_checked(mb, out.cpu().numpy()), want, "input written just before, on the same stream")
    mb.close()
