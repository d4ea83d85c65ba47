"""Batch spans on the GPU (include/audiomod_pv.h pv_batch_run_span): for any division of a batch's launches into
spans, the concatenated outputs are pv_batch_run's bit for bit, no kernel touches a window outside the reported ranges,
and the spans follow their stream's order with no host synchronisation in between.

Every case runs in launches of a few slices (AUDIOMOD_PV_CHUNK_SLICES), so short inputs give many launches.  The
reference of a case is the SAME object's synchronous pv_batch_run; two cases are also held against the oracle.

Windows.  Each input window is a fresh tensor of exactly rows x in_pitch floats, NaN everywhere but the reported
[in_begin, in_end): a load outside the range poisons the output (NaN goes through every stage).  Each output window is
filled with a sentinel and must keep it outside [out_begin, out_end).  Pitches are the smallest the contract allows."""
import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

SENTINEL = -12345.671875   # exactly representable; no case's audio comes near it
PV_ERR_INVALID_ARG = 1

# name: (configuration, streams, frames, flush, slices per launch, arithmetic settings)
BOTH = (E.ARITH_FAST, E.ARITH_EXACT)
CASES = {
    "a_pitch_fft2048_cm1": (dict(channels=2, semitones=4.0, coremode=1, fftsize=2048), 2, 20000, True, "8", BOTH),
    "b_stretch_fft4096": (dict(channels=2, mode="time_stretch", time_ratio=1.5, fftsize=4096), 2, 20000, False, "4", BOTH),
    "c_formant_down7": (dict(channels=2, mode="formant_pitchshift", semitones=-7.0, fftsize=2048), 2, 20000, True, "4", BOTH),
    "d_fft256_up15": (dict(channels=2, semitones=15.558, fftsize=256), 2, 2000, True, "8", BOTH),
    "e_mono_fft1024_hop300": (dict(channels=1, semitones=3.0, fftsize=1024, sample_rate=44100, hopsize=300), 2, 20000,
                              True, "8", BOTH),
    "robotic_down9": (dict(channels=2, mode="robotic", semitones=-9.0, fftsize=2048), 2, 20000, True, "4", (E.ARITH_EXACT,)),
    "vocoder": (dict(channels=2, mode="vocoder", fftsize=2048), 2, 20000, True, "4", BOTH),
    "whisper": (dict(channels=2, mode="whisper", fftsize=2048), 2, 20000, True, "4", BOTH),
    "wide_96_streams": (dict(channels=2, semitones=4.0, coremode=1, fftsize=2048), 96, 6000, True, "4", BOTH),
}
PARAMS = [pytest.param((name, arith), id=f"{name}-{'exact' if arith else 'fast'}")
          for name, c in CASES.items() for arith in c[5]]


def _same(got, want):
    return got.shape == want.shape and torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


class Ctx:
    """one case under one arithmetic setting: the engine, the input (pinned host and device) and pv_batch_run's output"""

    def __init__(self, name, arith, monkeypatch):
        kw, S, F, flush, chunk, _ = CASES[name]
        monkeypatch.setenv("AUDIOMOD_PV_CHUNK_SLICES", chunk)
        try:
            self.b = E.Batch(S, F, block=480, flush=flush, **kw)
        finally:
            monkeypatch.delenv("AUDIOMOD_PV_CHUNK_SLICES")
        ch = kw["channels"]
        voices = [signals.voice(F, ch, seed=31, stream=s % 7, sample_rate=kw.get("sample_rate", 48000)) for s in range(S)]
        x = np.stack([np.roll(v, 37 * (s // 7), axis=1) for s, v in enumerate(voices)]).astype(np.float32)
        self.host = torch.from_numpy(x).pin_memory()
        self.x = self.host.cuda()
        torch.cuda.synchronize()
        self.want = self.b.run(self.x)
        torch.cuda.synchronize()
        self.want = self.want.clone()
        assert bool(torch.isfinite(self.want).all())
        assert self.b.launches >= 7, self.b.launches

    def close(self):
        self.b.close()


_CTX = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    torch.cuda.synchronize()
    for c in _CTX.values():
        c.close()
    _CTX.clear()


@pytest.fixture
def ctx(request, monkeypatch):
    name, arith = request.param
    prev = E.set_arithmetic(arith)
    try:
        if (name, arith) not in _CTX:
            _CTX[(name, arith)] = Ctx(name, arith, monkeypatch)
        yield _CTX[(name, arith)]
    finally:
        E.set_arithmetic(prev)


def _pattern(kind, launches):
    if kind == "each":
        return [1] * launches
    if kind == "whole":
        return [launches]
    cuts = [1, 3, 2]                      # uneven: 1, 3, 2, rest
    assert launches > sum(cuts)
    return cuts + [launches - sum(cuts)]


def _pitch(n):
    return max(4, (n + 3) // 4 * 4)


def _run_spans(c, sizes, first=0):
    """Enqueues the spans `sizes` from launch `first` on ONE non-default stream, the input produced on that stream
    immediately before and no host synchronisation anywhere; returns (span info, output window) pairs."""
    b = c.b
    s = torch.cuda.Stream()
    done = []
    with torch.cuda.stream(s):
        x = torch.empty_like(c.x)
        x.copy_(c.host, non_blocking=True)
        f = first
        for n in sizes:
            sp = b.span(f, n)
            li = sp["in_end"] - sp["in_begin"]
            win = torch.full((b.nstreams, b.channels, _pitch(li)), float("nan"), dtype=torch.float32, device="cuda")
            if li:
                win[:, :, :li] = x[:, :, sp["in_begin"]:sp["in_end"]]
            out = torch.full((b.nstreams, b.channels, _pitch(sp["out_end"] - sp["out_begin"])), SENTINEL,
                             dtype=torch.float32, device="cuda")
            b.run_span(f, n, win, out)
            done.append((sp, out))
            f += n
    s.synchronize()
    return done


def _assemble(c, done):
    """the spans' outputs put together; asserts the sentinel outside every span's range"""
    got = torch.full_like(c.want, SENTINEL)
    for sp, out in done:
        lo, hi = sp["out_begin"], sp["out_end"]
        got[:, :, lo:hi] = out[:, :, :hi - lo]
        assert bool((out[:, :, hi - lo:] == SENTINEL).all()), f"span {sp} wrote beyond its output range"
    return got


@pytest.mark.parametrize("kind", ["each", "uneven", "whole"])
@pytest.mark.parametrize("ctx", PARAMS, indirect=True)
def test_spans_are_the_whole_run_bit_for_bit(ctx, kind):
    done = _run_spans(ctx, _pattern(kind, ctx.b.launches))
    assert done[0][0]["out_begin"] == 0 and done[-1][0]["out_end"] == ctx.b.out_frames
    got = _assemble(ctx, done)
    assert bool(torch.isfinite(got).all()), "a kernel read outside a window's reported input range"
    assert _same(got, ctx.want)


@pytest.mark.parametrize("ctx", [pytest.param(("a_pitch_fft2048_cm1", a), id="fast" if a == 0 else "exact") for a in BOTH],
                         indirect=True)
def test_a_span_out_of_sequence_is_refused_and_changes_nothing(ctx):
    b, L = ctx.b, ctx.b.launches
    done = _run_spans(ctx, [2])
    win = torch.zeros((b.nstreams, b.channels, _pitch(b.frames)), device="cuda")
    out = torch.zeros((b.nstreams, b.channels, _pitch(b.out_frames)), device="cuda")
    args = (C_void(win), win.shape[2], C_void(out), out.shape[2], None)
    for first, n in ((3, 1), (1, 1), (2, L), (L, 1), (2, 0), (-1, 1)):
        assert b.L.pv_batch_run_span(b.h, first, n, *args) == PV_ERR_INVALID_ARG, (first, n)
    # a bad pitch or a misaligned base for the right span: refused too
    assert b.L.pv_batch_run_span(b.h, 2, 1, C_void(win), 6, C_void(out), out.shape[2], None) == PV_ERR_INVALID_ARG
    assert b.L.pv_batch_run_span(b.h, 2, 1, C_void(win, 4), win.shape[2], C_void(out), out.shape[2], None) == PV_ERR_INVALID_ARG
    torch.cuda.synchronize()
    # the correct sequence afterwards still gives the right bits
    done += _run_spans(ctx, [1, L - 3], first=2)
    assert _same(_assemble(ctx, done), ctx.want)


def C_void(t, offset=0):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + offset)


@pytest.mark.parametrize("ctx", [pytest.param(("a_pitch_fft2048_cm1", a), id="fast" if a == 0 else "exact") for a in BOTH],
                         indirect=True)
def test_a_whole_run_after_some_spans_restarts(ctx):
    b = ctx.b
    _run_spans(ctx, [1, 2])
    out = b.run(ctx.x)
    torch.cuda.synchronize()
    assert _same(out, ctx.want)
    # ... and the spans must start over: launch 3 no longer follows anything
    sp = b.span(3, 1)
    win = torch.zeros((b.nstreams, b.channels, _pitch(sp["in_end"] - sp["in_begin"])), device="cuda")
    with pytest.raises(E.PvError):
        b.run_span(3, 1, win)
    assert _same(_assemble(ctx, _run_spans(ctx, _pattern("uneven", b.launches))), ctx.want)


@pytest.mark.parametrize("ctx", [pytest.param(("robotic_down9", E.ARITH_EXACT), id="robotic")], indirect=True)
def test_robotic_spans_are_the_oracle_bit_for_bit(ctx):
    kw, S, F, flush, _, _ = CASES["robotic_down9"]
    got = _assemble(ctx, _run_spans(ctx, _pattern("uneven", ctx.b.launches))).cpu().numpy()
    cfg = {k: v for k, v in kw.items() if k != "channels"}
    for s in range(S):
        want = O.run_offline(ctx.host[s].numpy(), block=480, flush=flush, **cfg)[0]
        assert got[s].shape == want.shape
        assert np.array_equal(got[s].view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), f"stream {s}"


@pytest.mark.parametrize("ctx", [pytest.param(("a_pitch_fft2048_cm1", a), id="fast" if a == 0 else "exact") for a in BOTH],
                         indirect=True)
def test_pitch_shift_spans_meet_the_rms_contract_against_the_oracle(ctx):
    kw, S, F, flush, _, _ = CASES["a_pitch_fft2048_cm1"]
    got = _assemble(ctx, _run_spans(ctx, _pattern("each", ctx.b.launches))).cpu().numpy()
    cfg = {k: v for k, v in kw.items() if k != "channels"}
    for s in range(S):
        want = np.asarray(O.run_offline(ctx.host[s].numpy(), block=480, flush=flush, **cfg)[0], np.float64)
        assert got[s].shape == want.shape
        rms = float(np.sqrt(np.mean((got[s].astype(np.float64) - want) ** 2)))
        print(f"stream {s}: RMS against the oracle {rms:.3e}")
        assert rms <= 1e-4, rms
