"""The asynchronous contract of Batch.run and MixedBatch.run (include/audiomod_pv.h: "enqueue all work on hip_stream and
return without synchronising"): a run is ordered behind whatever its stream holds when it is enqueued, and whatever is
enqueued behind it on that stream sees its whole output -- although inside, pv_batch_run forks to a high-priority chain
stream (and, with AUDIOMOD_PV_RES_STREAM=1, to a resampling stream), joins through rotating events and restarts its
state with memsets on the caller's stream.

Every comparison is bit for bit against the SAME object's synchronous result: input uploaded synchronously, run on the
current stream, torch.cuda.synchronize() before and after.

The delay.  The late-input tests put a spinning kernel (torch.cuda._sleep) in front of the copy that produces the
input, so that run() returns while its input is not there yet.  The spin has to outlast the host time of run(); that
time is measured once per module (`delay` fixture: the slowest of the configurations' run() calls), the spin is sized
to DELAY_FACTOR times it, at least DELAY_MIN_MS and at most DELAY_MAX_MS, and its cycle count comes from a calibration
of _sleep against HIP events.  Each test asserts that the producer's event has NOT completed when run() returns -- a
producer that had already finished would have tested nothing.  The negative control issues the same run on a stream
that does not wait for the producer and must NOT match: it shows that the delay makes a broken order visible.  (The
stale content of the input buffer is valid audio on purpose: a broken order gives a wrong answer, never non-finite
input to the rotation chain.)

Measured on an MI355X (the `delay` fixture prints it under -s), two sessions: run() takes 2.9 and 5.8 ms of host time
at most (152 launches, fft512_cm1), so the floor decides: a spin of 100 ms = 240 821 793 and 240 427 007 cycles of
torch.cuda._sleep (2.4 million per ms), 17 to 34 times the host time; the negative control fails to match, as designed."""
import functools
import time

import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals
from tests.test_mbatch_gpu import STREAMS
from tests.test_mbatch_redraw_gpu import B as REDRAWN

pytestmark = pytest.mark.gpu

S, F = 3, 60000          # 3 stereo streams x 60 000 frames ...
CHUNK = "8"              # ... in launches of 8 slices: more than 10 launches, many chunks in the pipeline
DELAY_FACTOR = 8.0       # the spin against the measured host time of run()
DELAY_MIN_MS = 100.0     # (host jitter: a run() that is descheduled for a few milliseconds must not void the test)
DELAY_MAX_MS = 1000.0

# name: (configuration, flush, environment at creation, pipelined as pv_batch_pipelined must report; None: as it does)
CONFIGS = {
    # pipelined three-stage path with the look-ahead order (PV_ARITH_FAST: fused kernels; PV_ARITH_EXACT: tile path)
    "fft2048_cm1": (dict(semitones=4.0, coremode=1, fftsize=2048), True, {}, True),
    # ... with the resampling kernel on a stream of its own and the join at the end of the run
    "fft2048_cm1_res_stream": (dict(semitones=4.0, coremode=1, fftsize=2048), True, {"AUDIOMOD_PV_RES_STREAM": "1"}, True),
    # no resampling stage.  (Core::pipeline_wanted: frames above 2048 points do not take the second stream, so this
    # one runs on the caller's stream alone; the 2048-point case below is the pipelined one without a resampling stage)
    "stretch_fft4096": (dict(mode="time_stretch", time_ratio=1.5, fftsize=4096), False, {}, None),
    "stretch_fft2048": (dict(mode="time_stretch", time_ratio=1.5, fftsize=2048), False, {}, True),
    # not pipelined: the control
    "fft2048_cm0": (dict(semitones=4.0, coremode=0, fftsize=2048), True, {}, False),
    # generic kernels.  (74 slices: ten launches of 8, so this one runs in launches of 4 -- nineteen of them)
    "fft8192_cm1": (dict(semitones=4.0, coremode=1, fftsize=8192), True, {"AUDIOMOD_PV_CHUNK_SLICES": "4"}, None),
    # four-waves-per-block kernels
    "fft512_cm1": (dict(semitones=4.0, coremode=1, fftsize=512), True, {}, True),
}
DEFAULT = "fft2048_cm1"


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


@functools.lru_cache(maxsize=None)
def _host_batch(seed):
    x = np.stack([signals.voice(F, 2, seed=seed, stream=s) for s in range(S)])
    x.setflags(write=False)
    return x


def _inputs():
    """x_a, x_b: two different voice batches, on the device, complete"""
    xs = [torch.from_numpy(_host_batch(seed).copy()).cuda() for seed in (70, 170)]
    torch.cuda.synchronize()
    return xs


def _sync_run(b, x):
    """the synchronous result: nothing in flight before, nothing after"""
    torch.cuda.synchronize()
    out = b.run(x)
    torch.cuda.synchronize()
    return out.clone()


def _same(got, want):
    return got.shape == want.shape and torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


class Ctx:
    """one configuration under one arithmetic setting: the engine, a twin, the inputs and the synchronous results"""

    def __init__(self, name, setenv, delenv):
        kw, flush, env, pipelined = CONFIGS[name]
        env = dict({"AUDIOMOD_PV_CHUNK_SLICES": CHUNK}, **env)
        for k, v in env.items():
            setenv(k, v)
        try:
            self.b = E.Batch(S, F, channels=2, flush=flush, **kw)
            self.twin = E.Batch(S, F, channels=2, flush=flush, **kw)
        finally:
            for k in env:
                delenv(k)
        assert self.b.launches > 10, self.b.launches
        if pipelined is not None:
            assert self.b.pipelined == pipelined
        self.x_a, self.x_b = _inputs()
        self.want_a, self.want_b = _sync_run(self.b, self.x_a), _sync_run(self.b, self.x_b)
        assert not _same(self.want_a, self.want_b)
        # the twin's solo results (the same configuration: the same bits, but it is the twin's own run that says so)
        self.twin_a, self.twin_b = _sync_run(self.twin, self.x_a), _sync_run(self.twin, self.x_b)
        assert _same(self.twin_a, self.want_a) and _same(self.twin_b, self.want_b)

    def close(self):
        self.b.close(), self.twin.close()


_CTX = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    torch.cuda.synchronize()
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def _ctx(name, arith, monkeypatch):
    """created once per (configuration, arithmetic) and shared: the tests leave the references unchanged"""
    assert E.get_arithmetic() == arith
    if (name, arith) not in _CTX:
        _CTX[(name, arith)] = Ctx(name, monkeypatch.setenv, monkeypatch.delenv)
    return _CTX[(name, arith)]


@pytest.fixture(params=sorted(CONFIGS))
def ctx(request, arith, monkeypatch):
    return _ctx(request.param, arith, monkeypatch)


# ---- the delay --------------------------------------------------------------------------------------------------------
def _spin(cycles):
    """a kernel on the current stream that does nothing for `cycles`"""
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(cycles))
    else:  # a chain of large matrix products: `cycles` counts products
        a = torch.ones((4096, 4096), device="cuda")
        for _ in range(int(cycles)):
            a = (a @ a).clamp_(0.0, 1.0)


def _spin_ms(cycles):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    _spin(cycles)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


@pytest.fixture(scope="module")
def delay():
    """cycles of _spin that outlast run()'s host time DELAY_FACTOR times over (module docstring).  The host time is that
    of the configuration with the most launches per run -- fft512_cm1 -- and of the default one, whichever is larger,
    each the slowest of five warm calls."""
    prev = E.set_arithmetic(E.ARITH_FAST)
    host_ms, launches = 0.0, 0
    try:
        for name in ("fft512_cm1", DEFAULT):
            kw, flush, _, _ = CONFIGS[name]
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("AUDIOMOD_PV_CHUNK_SLICES", CHUNK)
                b = E.Batch(S, F, channels=2, flush=flush, **kw)
            x = _inputs()[0]
            out = b.alloc_out()
            _sync_run(b, x)  # warm: code objects loaded
            for _ in range(5):
                torch.cuda.synchronize()
                t = time.perf_counter()
                b.run(x, out)
                host_ms = max(host_ms, (time.perf_counter() - t) * 1e3)
            torch.cuda.synchronize()
            launches = max(launches, b.launches)
            b.close()
    finally:
        E.set_arithmetic(prev)
    want_ms = min(max(DELAY_FACTOR * host_ms, DELAY_MIN_MS), DELAY_MAX_MS)
    # calibrate: grow the probe until it is long enough to time, then scale
    probe = 100_000 if hasattr(torch.cuda, "_sleep") else 4
    ms = _spin_ms(probe)
    while ms < 5.0 and probe < (1 << 40):
        probe *= 4
        ms = _spin_ms(probe)
    cycles = max(int(probe * want_ms / ms), 1)
    got_ms = _spin_ms(cycles)
    print(f"\n[test_async_gpu] run() host time {host_ms:.3f} ms at most (up to {launches} launches); spin of "
          f"{want_ms:.0f} ms = {cycles} cycles ({probe / ms:.0f} per ms), measured {got_ms:.1f} ms")
    assert got_ms >= 0.5 * want_ms, "the calibrated spin is shorter than asked for"
    assert host_ms * 2.0 <= got_ms, "the spin does not outlast run()'s host time"
    return cycles


def _late_input(run, x_a, x_b, d_in, producer, consumer, cycles):
    """d_in holds x_b; on `producer`: spin, d_in <- x_a, event; on `consumer`: run(d_in), snapshot of the output.  Returns
    the snapshot (complete).  consumer is producer: stream order alone must make the run see x_a."""
    d_in.copy_(x_b)
    torch.cuda.synchronize()
    ev = torch.cuda.Event()
    with torch.cuda.stream(producer):
        _spin(cycles)
        d_in.copy_(x_a, non_blocking=True)
        ev.record(producer)
    with torch.cuda.stream(consumer):
        d_out = run(d_in, consumer)
        pending = not ev.query()
        snap = d_out.clone()
    # (only now)
    consumer.synchronize()
    producer.synchronize()
    assert pending, "the producer had finished when run() returned: the delay is too short to test anything"
    return snap


# ---- Batch ------------------------------------------------------------------------------------------------------------
def _batch_run(b):
    return lambda d_in, stream: b.run(d_in, b.alloc_out(), stream=stream)


@pytest.mark.parametrize("null", [False, True], ids=["side_stream", "null_stream"])
def test_late_input(ctx, null, delay):
    """run() behind a producer that is still spinning, on a side stream and on the null stream (hip_stream = NULL: the
    internal streams are hipStreamNonBlocking, so nothing is implicit there either)"""
    s = torch.cuda.default_stream() if null else torch.cuda.Stream()
    assert (s.cuda_stream == 0) == null
    snap = _late_input(_batch_run(ctx.b), ctx.x_a, ctx.x_b, torch.empty_like(ctx.x_a), s, s, delay)
    assert _same(snap, ctx.want_a), "the run did not wait for its input"


def test_negative_control_a_run_that_does_not_wait_is_seen(monkeypatch, delay):
    """the same set-up with the run on a second stream that does not wait for the producer: it reads the stale (valid)
    input and must NOT give x_a's result -- the delay makes a broken order observable here.  Once per module, on the
    pipelined default configuration, under the process's arithmetic setting."""
    c = _ctx(DEFAULT, E.get_arithmetic(), monkeypatch)
    snap = _late_input(_batch_run(c.b), c.x_a, c.x_b, torch.empty_like(c.x_a), torch.cuda.Stream(), torch.cuda.Stream(), delay)
    assert not _same(snap, c.want_a)
    assert _same(snap, c.want_b)  # what it read was the stale batch, whole


@pytest.mark.parametrize("null", [False, True], ids=["side_stream", "null_stream"])
def test_back_to_back_without_a_sync(ctx, null):
    """three runs on one stream, one synchronisation: the state reset of a run (memsets on the caller's stream) must not
    overtake the previous run's tail on the internal streams, nor a rotating event be taken for the previous run's"""
    s = torch.cuda.default_stream() if null else torch.cuda.Stream()
    b = ctx.b
    o1, o2, o3 = b.alloc_out(), b.alloc_out(), b.alloc_out()
    torch.cuda.synchronize()
    b.run(ctx.x_a, o1, stream=s)
    b.run(ctx.x_b, o2, stream=s)
    b.run(ctx.x_a, o3, stream=s)
    s.synchronize()
    assert _same(o1, ctx.want_a), "first run"
    assert _same(o2, ctx.want_b), "second run"
    assert _same(o3, ctx.want_a), "third run"


def test_one_output_buffer_reused(ctx):
    """run, copy, run into the same buffer, copy: work enqueued behind a run sees its whole output, and the next run does
    not write before that work has read"""
    s = torch.cuda.Stream()
    b = ctx.b
    o = b.alloc_out()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        b.run(ctx.x_a, o, stream=s)
        c1 = o.clone()
        b.run(ctx.x_b, o, stream=s)
        c2 = o.clone()
    s.synchronize()
    assert _same(c1, ctx.want_a), "copy behind the first run"
    assert _same(c2, ctx.want_b), "copy behind the second run"


@pytest.mark.parametrize("null", [False, True], ids=["two_side_streams", "one_on_the_null_stream"])
def test_two_engines_at_once(ctx, null):
    """two engines of one configuration, different inputs, interleaved on two streams: each equals its solo result"""
    s1 = torch.cuda.default_stream() if null else torch.cuda.Stream()
    s2 = torch.cuda.Stream()
    b1, b2 = ctx.b, ctx.twin
    o = [b1.alloc_out() for _ in range(4)]
    torch.cuda.synchronize()
    b1.run(ctx.x_a, o[0], stream=s1)
    b2.run(ctx.x_b, o[1], stream=s2)
    b1.run(ctx.x_b, o[2], stream=s1)
    b2.run(ctx.x_a, o[3], stream=s2)
    torch.cuda.synchronize()
    assert _same(o[0], ctx.want_a) and _same(o[2], ctx.want_b), "first engine"
    assert _same(o[1], ctx.twin_b) and _same(o[3], ctx.twin_a), "second engine"


def test_timing_on_changes_no_bit(ctx):
    """enable_timing puts event records on the caller's and on the internal streams"""
    b = ctx.b
    try:
        b.enable_timing(1)
        got = _sync_run(b, ctx.x_a)
        assert _same(got, ctx.want_a), "with timing on"
        ms, n = b.kernel_times()["pv_analyze_kernel"]
        assert n == b.launches and ms > 0.0
    finally:
        b.enable_timing(0)
    assert _same(_sync_run(b, ctx.x_a), ctx.want_a), "with timing off again"
    # (and timed runs back to back: the records of two runs interleave on the internal streams)
    s = torch.cuda.Stream()
    try:
        b.enable_timing(1)
        o1, o2 = b.alloc_out(), b.alloc_out()
        torch.cuda.synchronize()
        b.run(ctx.x_a, o1, stream=s)
        b.run(ctx.x_b, o2, stream=s)
        s.synchronize()
        assert _same(o1, ctx.want_a) and _same(o2, ctx.want_b), "timed runs back to back"
        assert b.kernel_times()["pv_analyze_kernel"][1] == 2 * b.launches
    finally:
        b.enable_timing(0)


# ---- MixedBatch -------------------------------------------------------------------------------------------------------
MIXED = {"fft512_cm1": dict(fftsize=512, coremode=1), "fft2048_cm1": dict(fftsize=2048, coremode=1)}
MB_CHUNK = "16"  # as tests/test_mbatch_gpu.py has it: at least 8 launch groups


@functools.lru_cache(maxsize=None)
def _clip(frames, seed):
    x = signals.voice(frames, 2, seed=seed)
    x.setflags(write=False)
    return x


def _clips(streams, seed0):
    return [_clip(f, seed0 + i) for i, (f, _, _) in enumerate(streams)]


def _mb_sync_run(mb, x):
    torch.cuda.synchronize()
    out = mb.run(x)
    torch.cuda.synchronize()
    return out.clone()


class MixedCtx:
    def __init__(self, name, setenv, delenv):
        self.kw = MIXED[name]
        setenv("AUDIOMOD_PV_CHUNK_SLICES", MB_CHUNK)
        try:
            self.mb = E.MixedBatch(STREAMS, channels=2, **self.kw)
        finally:
            delenv("AUDIOMOD_PV_CHUNK_SLICES")
        assert self.mb.launches >= 8
        self.x_a, self.x_b = self.mb.pack(_clips(STREAMS, 300)), self.mb.pack(_clips(STREAMS, 700))
        torch.cuda.synchronize()
        self.want_a, self.want_b = _mb_sync_run(self.mb, self.x_a), _mb_sync_run(self.mb, self.x_b)
        assert not _same(self.want_a, self.want_b)

    def close(self):
        self.mb.close()


@pytest.fixture(params=sorted(MIXED))
def mctx(request, arith, monkeypatch):
    key = ("mixed", request.param, arith)
    if key not in _CTX:
        _CTX[key] = MixedCtx(request.param, monkeypatch.setenv, monkeypatch.delenv)
    return _CTX[key]


def test_mixed_late_input(mctx, delay):
    s = torch.cuda.Stream()
    mb = mctx.mb
    snap = _late_input(lambda d_in, stream: mb.run(d_in, mb.alloc_out(), stream=stream), mctx.x_a, mctx.x_b,
                       torch.empty_like(mctx.x_a), s, s, delay)
    assert _same(snap, mctx.want_a), "the run did not wait for its input"


def test_mixed_back_to_back_without_a_sync(mctx):
    s = torch.cuda.Stream()
    mb = mctx.mb
    o1, o2, o3 = mb.alloc_out(), mb.alloc_out(), mb.alloc_out()
    torch.cuda.synchronize()
    mb.run(mctx.x_a, o1, stream=s)
    mb.run(mctx.x_b, o2, stream=s)
    mb.run(mctx.x_a, o3, stream=s)
    s.synchronize()
    assert _same(o1, mctx.want_a) and _same(o2, mctx.want_b) and _same(o3, mctx.want_a)


def test_mixed_one_output_buffer_reused(mctx):
    s = torch.cuda.Stream()
    mb = mctx.mb
    o = mb.alloc_out()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        mb.run(mctx.x_a, o, stream=s)
        c1 = o.clone()
        mb.run(mctx.x_b, o, stream=s)
        c2 = o.clone()
    s.synchronize()
    assert _same(c1, mctx.want_a) and _same(c2, mctx.want_b)


@pytest.mark.parametrize("name", sorted(MIXED))
def test_mixed_run_redraw_run(name, arith, monkeypatch):
    """run, redraw, run on one stream with no synchronisation of the caller's in between (the redraw waits for the
    device itself before it writes anything resident): both outputs are what fresh objects of the two draws give"""
    kw = MIXED[name]
    monkeypatch.setenv("AUDIOMOD_PV_CHUNK_SLICES", MB_CHUNK)
    mb = E.MixedBatch(STREAMS, channels=2, **kw)
    fresh = [E.MixedBatch(d, channels=2, **kw) for d in (STREAMS, REDRAWN)]
    monkeypatch.delenv("AUDIOMOD_PV_CHUNK_SLICES")
    x = [f.pack(_clips(d, 300)) for f, d in zip(fresh, (STREAMS, REDRAWN))]
    want = [_mb_sync_run(f, xi) for f, xi in zip(fresh, x)]
    o1 = mb.alloc_out()
    o2 = fresh[1].alloc_out()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    mb.run(x[0], o1, stream=s)
    mb.redraw(REDRAWN)
    assert mb.out_floats == fresh[1].out_floats and mb.in_floats == fresh[1].in_floats
    mb.run(x[1], o2, stream=s)
    s.synchronize()
    assert _same(o1, want[0]), "the run before the redraw"
    assert _same(o2, want[1]), "the run after the redraw"
    mb.close(), fresh[0].close(), fresh[1].close()
