"""The phase-locked stage in every form it exists in, on inputs that fill its peak lists and place its step patterns.

tests/test_phase_forms_host.py holds the cases and proves on the oracle's trace that each reaches its situation.  Here
they run through the forms of the stage (engine.phase_census_read names them):
    batch ring 8 / ring 4   pv_match_kernel + pv_seq_ring_kernel<8 | 4>       ("batch", "ring", 8 | 4)
    batch one step ahead    pv_seq_kernel<1>  (AUDIOMOD_PV_SEQ_RING=0; always at fft 8192)   ("batch", "step", 1)
    batch narrow            pv_seq_kernel<3>  (AUDIOMOD_PV_SEQ_NARROW=1)       ("batch", "step", 3)
    engine                  pv_phase_kernel<8>, or the two kernels with AUDIOMOD_PV_STREAM_FUSE_PHASE=0
                                                                               ("batch", "fused", 8) / ("batch", "ring", 8)
    single launch           pv_stream_kernel  (AUDIOMOD_PV_STREAM_LAUNCHES=single)           ("batch", "stream", 1)
    pool / mixed pool       pv_pool_phase_kernel<8> / pv_pmix_phase_kernel<8>  ("pool" | "pmix", "fused", 8)
    mixed batch             pv_mb_match_kernel + pv_mb_seq_kernel<4>           ("mb", "ring", 4)
Each run is held to three things: (i) the census shows the expected form and no other; (ii) every stream against the
oracle -- per-call counts where there are calls, RMS <= 1e-4 and the error-shape bar of tests/helpers.py; (iii) the same
bits as the other forms under the same arithmetic setting: batch forms and mixed-batch streams against Batch(1, frames)
of the stream, pool slots against the single-stream engine fed the same blocks, the engine's two routes against each
other.  Forms chosen by a variable that is read once per process run in child processes, one at a time.

At fft 8192 (1368 list slots, more than a workgroup has lanes) the batch and the engine take the one-step form;
StreamPool and MixedBatch refuse the configuration at creation (PvError), as they did before this file."""
import contextlib
import functools
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from audiomod_amd import engine as E
from oracle import oracle_py as O
from tests.helpers import assert_shape, bits_equal, oracle_floor, parity_shape
from tests import test_phase_forms_host as H
from tests.test_phase_forms_host import BLOCK, HOP1, N1, SHIFT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RMS_TOL = 1e-4   # BASELINE's contract (tests/test_gpu_parity.py RMS_TOL)
FAST, EXACT = 0, 1   # engine.ARITH_FAST / ARITH_EXACT
ARITHS = [pytest.param(FAST, id="fast"), pytest.param(EXACT, id="exact")]
WAVE_COMBS = [c.name for c in H.COMB_CASES if c.fft <= 4096]
BIG_COMBS = [c.name for c in H.COMB_CASES if c.fft == 8192]
EDGES = [c.name for c in H.EDGE_CASES]


def _cfg(name):
    return dict(fftsize=H.BY_NAME[name].fft, **SHIFT)


# ---- inputs and references: a case gives two streams, the signal and (stereo) the signal with its channels swapped ----
@functools.lru_cache(maxsize=None)
def _signal(name, variant):
    x = H.signal(name)
    if variant:
        x = np.ascontiguousarray(x[::-1]) if x.shape[0] == 2 else np.ascontiguousarray(-x)
        x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _oracle(name, variant):
    if not variant:
        want, counts, _ = H.oracle(name)
        return want, counts
    want, counts, _ = O.run_offline(_signal(name, variant), block=BLOCK, **_cfg(name))
    want.setflags(write=False)
    return want, tuple(counts)


@functools.lru_cache(maxsize=None)
def _floor(name, variant, arith):
    return oracle_floor(O.run_offline, _signal(name, variant), arith, want=_oracle(name, variant)[0], block=BLOCK,
                        **_cfg(name))


def _against_oracle(label, got, name, variant, arith, counts=None):
    want, wc = _oracle(name, variant)
    if counts is not None:
        assert list(counts) == list(wc), label
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert want.shape[1] > 0 and float(np.abs(want).max()) > 0.01, label   # there is audio to compare
    shape = parity_shape(got, want)
    print(f"{label}: rms {shape['rms']:.3e} max_abs {shape['max_abs']:.3e} win_rms {shape['win_rms']:.3e}")
    assert shape["rms"] <= RMS_TOL, (label, shape)
    assert_shape(label, got, want, _floor(name, variant, arith), arith)


@contextlib.contextmanager
def _env(**kv):
    """environment variables the library reads when an object is created"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module", autouse=True)
def census():
    """On for the module.  Where AUDIOMOD_PV_CHAIN_CENSUS already switched it on for the process it is left alone (the
    counts are written out at exit); the tests read differences only."""
    if not os.environ.get("AUDIOMOD_PV_CHAIN_CENSUS"):
        E.chain_census(True)
        yield
        E.chain_census(False)
    else:
        yield


@contextlib.contextmanager
def _forms(want):
    """the forms of the phase stage launched inside the block: exactly `want`"""
    before = E.phase_census_read()
    yield
    after = E.phase_census_read()
    got = {k for k, v in after.items() if v - before.get(k, 0) > 0}
    print("phase census:", sorted(got))
    assert got == set(want), (got, want)


@pytest.fixture
def arithmetic():
    prev = E.get_arithmetic()
    yield E.set_arithmetic
    E.set_arithmetic(prev)


# ---- the runners -------------------------------------------------------------------------------------------------
def run_batch(xs, cfg, chunk=None):
    """the streams `xs` ([channels, frames] each, same shape) as one Batch; a list of outputs"""
    import torch
    env = {} if chunk is None else dict(AUDIOMOD_PV_CHUNK_SLICES=str(chunk))
    with _env(**env):
        b = E.Batch(len(xs), xs[0].shape[1], channels=xs[0].shape[0], block=BLOCK, **cfg)
    out = b.run(torch.from_numpy(np.stack(xs)).cuda(),
                d_out=torch.full((len(xs), xs[0].shape[0], b.out_frames), float("nan"), device="cuda"))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    launches, slices = b.launches, b.slices
    b.close()
    return [out[i] for i in range(len(xs))], launches, slices


def run_mb(xs, cfg, chunk=None):
    import torch
    env = {} if chunk is None else dict(AUDIOMOD_PV_CHUNK_SLICES=str(chunk))
    streams = [(x.shape[1], cfg["semitones"], 1.0) for x in xs]
    with _env(**env):
        mb = E.MixedBatch(streams, channels=xs[0].shape[0], block=BLOCK, **cfg)
    y = mb.run(mb.pack(list(xs)))
    torch.cuda.synchronize()
    outs = [v.cpu().numpy() for v in mb.split(y)]
    mb.close()
    return outs


def _sizes(frames, schedule):
    """the calls of one run: `schedule` cycled over the input, then on through the flush"""
    it = itertools.cycle(schedule)
    pos = 0
    while True:
        n = next(it)
        yield pos, n
        pos += n


def drive(process, xs, schedule=(BLOCK,)):
    """The reference CLI's offline loop (engine.run_offline's) on several streams at once, with the sizes of the calls
    taken from `schedule`.  process(blocks) feeds one block per stream and returns what each then has, as a list of
    arrays.  Returns (outputs, per-call counts)."""
    n, frames, ch = len(xs), xs[0].shape[1], xs[0].shape[0]
    outs, counts, produced = [[] for _ in xs], [[] for _ in xs], [0] * n
    for pos, size in _sizes(frames, schedule):
        if pos < frames:
            blocks = [x[:, pos:pos + size] for x in xs]
        elif all(p >= frames for p in produced):
            break
        else:
            blocks = [np.zeros((ch, size), np.float32) for _ in xs]
        for j, y in enumerate(process(blocks)):
            counts[j].append(y.shape[1])
            w = y.shape[1] if pos < frames else max(min(y.shape[1], frames - produced[j]), 0)
            outs[j].append(y[:, :w])
            produced[j] += w
    return [np.concatenate(o, axis=1) for o in outs], counts


def run_pool(xs, cfg, mixed=False, schedule=(BLOCK,), steps=None):
    """`steps`: a list that receives the steps (slices) each feed's launch held for slot 0"""
    kw = dict(pitch_range=(-12.0, 12.0)) if mixed else {}
    pool = E.StreamPool(len(xs), channels=xs[0].shape[0], **kw, **cfg)
    slots = [pool.open(semitones=cfg["semitones"]) if mixed else pool.open() for _ in xs]

    def process(blocks):
        before = pool.info(slots[0])["slices"]
        pool.feed({s: b for s, b in zip(slots, blocks)})
        if steps is not None:
            steps.append(pool.info(slots[0])["slices"] - before)
        return [pool.retrieve(s, pool.available(s)) for s in slots]
    out = drive(process, xs, schedule)
    pool.close_pool()
    return out


def run_engine(x, cfg, schedule=(BLOCK,), fuse=True):
    c = E.make_config(x.shape[0], **cfg)
    with _env(AUDIOMOD_PV_STREAM_FUSE_PHASE="1" if fuse else "0"):
        pv = E.PhaseVocoder(c.sample_rate, x.shape[0], c.time_ratio, c.pitch_semitones, c.mode, c.coremode, c.fftsize,
                            c.hopsize, 0)

    def process(blocks):
        pv.processInData(blocks[0])
        return [pv.getOutData(pv.getOutSamples())]
    outs, counts = drive(process, [x], schedule)
    pv.close()
    return outs[0], counts[0]


def run_oracle(x, cfg, schedule):
    o = O.Oracle(x.shape[0], **cfg)

    def process(blocks):
        return [o.retrieve(o.process(blocks[0]))]
    outs, counts = drive(process, [x], schedule)
    o.close()
    return outs[0], counts[0]


def test_the_drive_loop_is_the_offline_loop():
    """drive() with the constant schedule on the oracle gives oracle_py.run_offline's output and counts (no GPU work:
    it pins the helper the pool and engine runs below are fed through)"""
    x = _signal("gap_single", 0)
    got, counts = run_oracle(x, _cfg("gap_single"), (BLOCK,))
    want, wc = _oracle("gap_single", 0)
    assert bits_equal(got, want) and list(counts) == list(wc)


def _batch_form(name):
    return ("batch", "step", 1) if H.BY_NAME[name].fft == 8192 else ("batch", "ring", 8)


# ---- references of the GPU's own: computed once per (signal, arithmetic) ---------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_of_one(name, variant, arith):
    assert E.get_arithmetic() == arith
    with _forms({_batch_form(name)}):
        y = run_batch([_signal(name, variant)], _cfg(name))[0][0]
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def _engine(name, variant, arith):
    assert E.get_arithmetic() == arith
    # (at fft 8192 the fused kernel does not fit: the two kernels, one step ahead)
    with _forms({("batch", "step", 1) if H.BY_NAME[name].fft == 8192 else ("batch", "fused", 8)}):
        y, counts = run_engine(_signal(name, variant), _cfg(name))
    y.setflags(write=False)
    return y, tuple(counts)


# ---- a. full lists in every form -------------------------------------------------------------------------------------
def check_batch(name, arith, label, form, **kw):
    xs = [_signal(name, v) for v in (0, 1)]
    with _forms({form}):
        outs, _, _ = run_batch(xs, _cfg(name), **kw)
    for v, got in enumerate(outs):
        _against_oracle(f"{label} {name} stream {v}", got, name, v, arith)
    return outs


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", WAVE_COMBS + BIG_COMBS)
def test_full_lists_batch(name, arith, arithmetic):
    arithmetic(arith)
    outs = check_batch(name, arith, "batch", _batch_form(name))
    for v in (0, 1):
        assert bits_equal(outs[v], _batch_of_one(name, v, arith)), (name, v)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", WAVE_COMBS + BIG_COMBS)
def test_full_lists_engine_both_routes(name, arith, arithmetic):
    arithmetic(arith)
    big = H.BY_NAME[name].fft == 8192
    x = _signal(name, 0)
    got, counts = _engine(name, 0, arith)
    _against_oracle(f"engine {name}", got, name, 0, arith, counts)
    with _forms({("batch", "step", 1) if big else ("batch", "ring", 8)}):
        two, counts2 = run_engine(x, _cfg(name), fuse=False)
    assert list(counts2) == list(counts) and bits_equal(two, got), name


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", WAVE_COMBS)
@pytest.mark.parametrize("set_", ["pool", "pmix"])
def test_full_lists_pool(set_, name, arith, arithmetic):
    arithmetic(arith)
    xs = [_signal(name, v) for v in (0, 1)]
    with _forms({(set_, "fused", 8)}):
        outs, counts = run_pool(xs, _cfg(name), mixed=set_ == "pmix")
    for v in (0, 1):
        _against_oracle(f"{set_} {name} slot {v}", outs[v], name, v, arith, counts[v])
        ref, rc = _engine(name, v, arith)
        assert list(counts[v]) == list(rc) and bits_equal(outs[v], ref), (set_, name, v)


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("name", WAVE_COMBS)
def test_full_lists_mixed_batch(name, arith, arithmetic):
    arithmetic(arith)
    xs = [_signal(name, v) for v in (0, 1)]
    with _forms({("mb", "ring", 4)}):
        outs = run_mb(xs, _cfg(name))
    for v in (0, 1):
        _against_oracle(f"mb {name} stream {v}", outs[v], name, v, arith)
        assert bits_equal(outs[v], _batch_of_one(name, v, arith)), (name, v)


@pytest.mark.parametrize("name", BIG_COMBS)
def test_fft_8192_is_refused_by_pool_and_mixed_batch(name):
    c = H.BY_NAME[name]
    with _forms(set()):
        with pytest.raises(E.PvError):
            E.StreamPool(2, channels=c.channels, **_cfg(name))
        with pytest.raises(E.PvError):
            E.StreamPool(2, channels=c.channels, pitch_range=(-12.0, 12.0), **_cfg(name))
        with pytest.raises(E.PvError):
            E.MixedBatch([(c.frames, 4.0, 1.0)] * 2, channels=c.channels, block=BLOCK, **_cfg(name))


@pytest.mark.parametrize("arith", ARITHS)
def test_full_lists_ring_4_by_row_count(arith, arithmetic):
    """49 stereo streams are 98 rows: the batch launcher takes the ring of depth 4 by itself"""
    arithmetic(arith)
    kinds = [("comb_1024", 0), ("comb_1024", 1), ("gap_single", 0), ("gap_single", 1)]
    xs = [_signal(*kinds[j % 4]) for j in range(49)]
    with _forms({("batch", "ring", 4)}):
        outs, _, _ = run_batch(xs, _cfg("comb_1024"))
    for j in (0, 1, 2, 3, 48):
        name, v = kinds[j % 4]
        _against_oracle(f"batch of 49 stream {j}", outs[j], name, v, arith)
    for j in range(49):
        name, v = kinds[j % 4]
        assert bits_equal(outs[j], _batch_of_one(name, v, arith)), j


# forms that a variable read once per process selects: child processes, one at a time
CHILD_FORMS = {
    "ring4": (dict(AUDIOMOD_PV_SEQ_DEPTH="4"), ("batch", "ring", 4)),
    "step": (dict(AUDIOMOD_PV_SEQ_RING="0"), ("batch", "step", 1)),
    "narrow": (dict(AUDIOMOD_PV_SEQ_NARROW="1"), ("batch", "step", 3)),
}
CHILD_VARS = ("AUDIOMOD_PV_SEQ_DEPTH", "AUDIOMOD_PV_SEQ_RING", "AUDIOMOD_PV_SEQ_NARROW", "AUDIOMOD_PV_STREAM_LAUNCHES",
              "AUDIOMOD_PV_EXACT", "AUDIOMOD_PV_CHAIN_CENSUS", "AUDIOMOD_PV_CHUNK_SLICES")


def child_main():
    """argv: what, output file.  Saves the outputs of every run with the census of each."""
    what, path = sys.argv[1], sys.argv[2]
    E.chain_census(True)
    arrays, forms = {}, {}

    def census_of(key, before):
        after = E.phase_census_read()
        forms[key] = sorted(k for k, v in after.items() if v - before.get(k, 0) > 0)
    if what == "batch":        # the comb cases as batches of two, under both arithmetic settings
        for arith in (FAST, EXACT):
            E.set_arithmetic(arith)
            for name in WAVE_COMBS:
                before = E.phase_census_read()
                outs, _, _ = run_batch([_signal(name, v) for v in (0, 1)], _cfg(name))
                census_of(f"{arith}/{name}", before)
                for v in (0, 1):
                    arrays[f"{arith}/{name}/{v}"] = outs[v]
    elif what == "sweep":      # the placement sweep's chunkings for the ring of depth 4
        for chunk in H.SWEEP_CHUNKS[4]:
            before = E.phase_census_read()
            outs, launches, slices = run_batch(_sweep_signals(), _sweep_cfg(), chunk=chunk)
            census_of(f"{chunk}", before)
            arrays[f"{chunk}/launches"] = np.array([launches, slices])
            for j, y in enumerate(outs):
                arrays[f"{chunk}/{j}"] = y
    elif what == "single":     # the single-launch kernel of the streaming path
        for arith in (FAST, EXACT):
            E.set_arithmetic(arith)
            for name in ("comb_2048", "comb_4096"):
                before = E.phase_census_read()
                y, counts = run_engine(_signal(name, 0), _cfg(name))
                census_of(f"{arith}/{name}", before)
                arrays[f"{arith}/{name}/0"] = y
                arrays[f"{arith}/{name}/counts"] = np.array(counts)
    np.savez(path, forms=np.array(json.dumps(forms)), **arrays)
    print("phase-child ok", len(arrays))


def _child(what, path, **env):
    code = "import sys; sys.path.insert(0, %r); from tests import test_phase_forms_gpu as T; T.child_main()" % (ROOT,)
    environ = {k: v for k, v in os.environ.items() if k not in CHILD_VARS}
    r = subprocess.run([sys.executable, "-c", code, what, path], capture_output=True, text=True,
                       env=dict(environ, **env), timeout=300)
    assert r.returncode == 0 and "phase-child ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    z = np.load(path)
    return z, {k: {tuple(f) for f in v} for k, v in json.loads(str(z["forms"])).items()}


@pytest.mark.parametrize("form", sorted(CHILD_FORMS))
def test_full_lists_batch_forms_by_variable(form, tmp_path, arithmetic):
    env, key = CHILD_FORMS[form]
    z, forms = _child("batch", str(tmp_path / "out.npz"), **env)
    for arith in (FAST, EXACT):
        arithmetic(arith)
        for name in WAVE_COMBS:
            assert forms[f"{arith}/{name}"] == {key}, (form, arith, name, forms)
            for v in (0, 1):
                got = z[f"{arith}/{name}/{v}"]
                _against_oracle(f"batch {form} {name} stream {v}", got, name, v, arith)
                assert bits_equal(got, _batch_of_one(name, v, arith)), (form, arith, name, v)


def test_full_lists_single_launch_kernel(tmp_path, arithmetic):
    """pv_stream_kernel: seq_role<1> on 512 threads, so 682 peaks at fft 4096 take the second trip of its LOCK loop.
    (i) and (ii) under both settings; (iii) under PV_ARITH_EXACT, where it writes the staged engine's bits.  (Under
    PV_ARITH_FAST the staged engine synthesises with the free-form fused kernel, which this kernel does not contain.)"""
    z, forms = _child("single", str(tmp_path / "out.npz"), AUDIOMOD_PV_STREAM_LAUNCHES="single")
    for arith in (FAST, EXACT):
        for name in ("comb_2048", "comb_4096"):
            assert forms[f"{arith}/{name}"] == {("batch", "stream", 1)}, forms
            _against_oracle(f"single launch {name}", z[f"{arith}/{name}/0"], name, 0, arith,
                            [int(c) for c in z[f"{arith}/{name}/counts"]])
            if arith == EXACT:
                arithmetic(arith)
                assert bits_equal(z[f"{arith}/{name}/0"], _engine(name, 0, arith)[0]), name


# ---- b. the placement sweep ------------------------------------------------------------------------------------------
def _sweep_cfg():
    return dict(fftsize=N1, **SHIFT)


def _sweep_signals():
    return [H.sweep_signal(j) for j in range(H.SWEEP_STREAMS)]


@functools.lru_cache(maxsize=None)
def _sweep_floor(j, arith):
    return oracle_floor(O.run_offline, H.sweep_signal(j), arith, want=H.sweep_oracle(j)[0], block=BLOCK, **_sweep_cfg())


@functools.lru_cache(maxsize=None)
def _sweep_batch_of_one(j):
    assert E.get_arithmetic() == FAST   # (b) and (c) run under the default
    y = run_batch([H.sweep_signal(j)], _sweep_cfg())[0][0]
    y.setflags(write=False)
    return y


def _check_sweep(label, outs, launches=None, slices=None, chunk=None):
    arith = E.get_arithmetic()
    if chunk is not None:
        assert slices == H.sweep_oracle(0)[2]["slices"] and launches == -(-slices // chunk), (label, launches, slices)
    for j, got in enumerate(outs):
        want = H.sweep_oracle(j)[0]
        assert got.shape == want.shape, (label, j)
        shape = parity_shape(got, want)
        assert shape["rms"] <= RMS_TOL, (label, j, shape)
        assert_shape(f"{label} stream {j}", got, want, _sweep_floor(j, arith), arith)
        assert bits_equal(got, _sweep_batch_of_one(j)), (label, j)


@pytest.mark.parametrize("chunk", H.SWEEP_CHUNKS[8])
def test_sweep_batch_ring_8(chunk):
    with _forms({("batch", "ring", 8)}):
        outs, launches, slices = run_batch(_sweep_signals(), _sweep_cfg(), chunk=chunk)
    _check_sweep(f"sweep chunk {chunk}", outs, launches, slices, chunk)


def test_sweep_batch_ring_4(tmp_path):
    z, forms = _child("sweep", str(tmp_path / "out.npz"), AUDIOMOD_PV_SEQ_DEPTH="4")
    for chunk in H.SWEEP_CHUNKS[4]:
        assert forms[f"{chunk}"] == {("batch", "ring", 4)}, forms
        launches, slices = (int(v) for v in z[f"{chunk}/launches"])
        _check_sweep(f"sweep depth 4 chunk {chunk}", [z[f"{chunk}/{j}"] for j in range(H.SWEEP_STREAMS)], launches,
                     slices, chunk)


@pytest.mark.parametrize("chunk", [4, 5])
def test_sweep_mixed_batch(chunk):
    with _forms({("mb", "ring", 4)}):
        outs = run_mb(_sweep_signals(), _sweep_cfg(), chunk=chunk)
    _check_sweep(f"sweep mb chunk {chunk}", outs)


POOL_SCHEDULE = tuple(k * HOP1 for k in range(1, 11))   # launches of 1 ... 10 steps at depth 8


def test_sweep_pool():
    """feeds of k hops, k cycling 1 ... 10: launches of that many steps.  Against the oracle and the single-stream engine
    fed the same blocks (counts and bits); the feeds do not change what a stream computes, so also Batch(1, frames)."""
    arith = E.get_arithmetic()
    xs = _sweep_signals()
    steps = []
    with _forms({("pool", "fused", 8)}):
        outs, counts = run_pool(xs, _sweep_cfg(), schedule=POOL_SCHEDULE, steps=steps)
    print("steps per feed:", steps)
    assert set(range(1, 11)) <= set(steps), steps   # launches of 1 ... 10 steps: shorter than, as long as and longer
    #                                                 than the ring of 8
    for j in (0, 7, 15):
        want, wc = run_oracle(xs[j], _sweep_cfg(), POOL_SCHEDULE)
        assert list(counts[j]) == list(wc), j
        assert max(wc) > 0 and bits_equal(want, H.sweep_oracle(j)[0])   # (the same stream, in other calls)
        with _forms({("batch", "fused", 8)}):
            ref, rc = run_engine(xs[j], _sweep_cfg(), POOL_SCHEDULE)
        assert list(counts[j]) == list(rc) and bits_equal(outs[j], ref), j
    _check_sweep("sweep pool", outs)
    assert arith == E.get_arithmetic()


# ---- c. edge states --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EDGES)
@pytest.mark.parametrize("set_", ["batch", "engine", "pool", "mb"])
def test_edge_states(set_, name):
    arith = E.get_arithmetic()
    xs = [_signal(name, v) for v in (0, 1)]
    cfg = _cfg(name)
    if set_ == "batch":
        outs = check_batch(name, arith, "batch", ("batch", "ring", 8))
    elif set_ == "mb":
        with _forms({("mb", "ring", 4)}):
            outs = run_mb(xs, cfg)
    elif set_ == "pool":
        with _forms({("pool", "fused", 8)}):
            outs, counts = run_pool(xs, cfg)
    else:
        got = [_engine(name, v, arith) for v in (0, 1)]
        outs, counts = [g[0] for g in got], [g[1] for g in got]
    for v in (0, 1):
        _against_oracle(f"{set_} {name} stream {v}", outs[v], name, v, arith, counts[v] if set_ in ("pool", "engine") else None)
        if set_ in ("batch", "mb"):
            assert bits_equal(outs[v], _batch_of_one(name, v, arith)), (set_, name, v)
        elif set_ == "pool":
            ref, rc = _engine(name, v, arith)
            assert list(counts[v]) == list(rc) and bits_equal(outs[v], ref), (name, v)
