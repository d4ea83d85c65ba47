"""Every analysis kernel's planes, and the phase stage's, against the oracle's plane trace: bit for bit.

tests/analysis_signals.py makes the inputs and tests/test_analysis_planes_host.py proves on the CPU what each of them does
to the oracle.  Here the same streams run through the batch, the single-stream engine, the stream pool (uniform and mixed)
and the mixed batch, and every slice the plane tap can read (engine.*.planes, include/audiomod_pv.h pv_debug_*_planes) is
compared with the oracle's trace of that stream: magnitudes, analysis phases, peak count, peak list, step mode, a locked
step's rotations, any other step's output phases.  tests/helpers.py bits_equal and equal integers; there is no tolerance
in this file.  The census' sixth kind (engine.analysis_census_read) must show exactly the analysis kernel the form is
expected to take:
    Batch fft 256 / 8192                       pv_analyze_kernel                      ("batch", "generic", 128 / 4096)
    Batch fft 512 / 1024 / 2048                pv_analyze_wave_kernel<256 / 512 / 1024> ("batch", "wave", nc)
    Batch fft 4096                             pv_analyze_split_kernel                ("batch", "split", 2048)
      ... with AUDIOMOD_PV_SPLIT_ANALYSIS=0    pv_analyze_wave_kernel<2048>           ("batch", "wave", 2048)
    PhaseVocoder                               the batch set's, per call
      ... AUDIOMOD_PV_STREAM_LAUNCHES=single   pv_stream_kernel                       ("batch", "stream", nc)
    StreamPool / mixed                         pv_pool_* / pv_pmix_*                  ("pool" | "pmix", "wave" | "split", nc)
    MixedBatch                                 pv_mb_*                                ("mb", "wave" | "split", nc)
Forms chosen by a variable that is read once per process run in child processes, one at a time, each under a timeout;
the child compares and reports, the parent asserts on the report."""
import contextlib
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from audiomod_amd import engine as E
from oracle import oracle_py as O
from tests import analysis_signals as A
from tests.helpers import bits_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST, EXACT = 0, 1   # engine.ARITH_FAST / ARITH_EXACT
BLOCK = A.BLOCK
# the cases every form but the batch runs: ordinary and mixed level, holes, and the peak search's corners
FORM_KINDS = ("ordinary", "mixed", "holes", "corners", "outer", "dcnyq", "single")


def batch_kernel(fft, split=True):
    nc = fft // 2
    if fft in (256, 8192):
        return ("batch", "generic", nc)
    return ("batch", "split" if fft == 4096 and split else "wave", nc)


def slot_kernel(set_, fft):
    return (set_, "split" if fft == 4096 else "wave", fft // 2)


# ---- comparing ---------------------------------------------------------------------------------------------------------
def _same(label, what, got, want):
    """bit equality of two float32 arrays, with the first difference in the message"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if not bits_equal(got, want):
        assert got.shape == want.shape, (label, what, got.shape, want.shape)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        i = int(bad[0])
        raise AssertionError(f"{label}: {what}[{i}] is {got[i]!r} ({got.view(np.uint32)[i]:#010x}), the oracle's "
                             f"{want[i]!r} ({want.view(np.uint32)[i]:#010x}); {bad.size} of {got.size} differ")


def compare_slice(label, got, want, t):
    """one slice of one row from the plane tap against step t of the oracle's plane trace"""
    label = f"{label} slice {t}"
    _same(label, "mag", got["mag"], want["mag"][t])
    _same(label, "phase", got["phase"], want["phase"][t])
    n, mode = int(want["npk"][t]), int(want["mode"][t])
    assert got["npk"] == n, (label, "npk", got["npk"], n)
    assert np.array_equal(got["peaks"], want["peaks"][t, :n]), (label, "peaks", list(got["peaks"]), list(want["peaks"][t, :n]))
    assert got["mode"] == mode, (label, "mode", got["mode"], mode)
    if mode == E.STEP_LOCK:
        assert got["outphase"] is None
        _same(label, "rot", got["rot"], want["rot"][t, :n])
    else:
        assert got["rot"] is None
        _same(label, "outphase", got["outphase"], want["outphase"][t])


def compare_readable(label, info, read, want, seen=None):
    """every readable slice (info: a plane_info dict; read(t): the tap) against the trace; `seen`: a set of the slices
    compared in earlier calls, which are skipped and added to.  Returns the number compared."""
    assert info["has_peaks"] and info["has_chain"], info
    n = 0
    for t in range(info["slice_begin"], info["slice_end"]):
        if seen is not None:
            if t in seen:
                continue
            seen.add(t)
        compare_slice(label, read(t), want, t)
        n += 1
    return n


@functools.lru_cache(maxsize=256)
def _trace(name, j, frames=None, semitones=None, time_ratio=None):
    """the oracle's planes of stream j of a case; with `frames` etc.: of its first `frames` frames under another pitch
    and time ratio (the mixed forms)"""
    if frames is None:
        info = A.oracle(name, j)[2]
        return info["planes"], info["slices"]
    c = A.BY_NAME[name]
    cfg = dict(c.cfg, semitones=semitones, time_ratio=time_ratio)
    _, _, info = O.run_offline(A.streams(name)[j][:, :frames], block=BLOCK, planes=True, fftsize=c.fft, **cfg)
    return info["planes"], info["slices"]


@contextlib.contextmanager
def _env(**kv):
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
    """On for the module.  Where AUDIOMOD_PV_CHAIN_CENSUS already switched it on for the process it is left alone; the
    tests read differences only."""
    if not os.environ.get("AUDIOMOD_PV_CHAIN_CENSUS"):
        E.chain_census(True)
        yield
        E.chain_census(False)
    else:
        yield


@contextlib.contextmanager
def _kernels(want):
    """the analysis kernels launched inside the block: exactly `want`"""
    before = E.analysis_census_read()
    yield
    after = E.analysis_census_read()
    got = {k for k, v in after.items() if v - before.get(k, 0) > 0}
    assert got == set(want), (got, want)


@pytest.fixture
def arithmetic():
    prev = E.get_arithmetic()
    yield E.set_arithmetic
    E.set_arithmetic(prev)


def _report(form, case, arith, kernels, slices):
    print(f"analysis-planes: form={form} case={case} arith={'exact' if arith == EXACT else 'fast'} "
          f"kernels={sorted(kernels)} slices={slices}")


# ---- the batch ---------------------------------------------------------------------------------------------------------
def batch_planes(name, chunk=None):
    """The case's streams as one Batch; every readable slice of every row compared.  Returns (slices compared, the
    plane_info, the planes read as {(stream, slice): dict}, the batch's launches)."""
    import torch
    c = A.BY_NAME[name]
    xs = A.streams(name)
    with _env(**({} if chunk is None else dict(AUDIOMOD_PV_CHUNK_SLICES=str(chunk)))):
        b = E.Batch(len(xs), xs[0].shape[1], channels=1, block=BLOCK, fftsize=c.fft, **c.cfg)
    try:
        assert b.plane_info()["slice_end"] == 0   # nothing to read before a run
        with pytest.raises(E.PvError, match="not held"):
            b.planes(0, 0, 0)
        b.run(torch.from_numpy(np.stack(xs)).cuda())
        info = b.plane_info()
        assert info["slice_end"] == b.slices and info["hs"] == c.fft // 2
        read, n = {}, 0
        for j in range(len(xs)):
            want, slices = _trace(name, j)
            assert slices == b.slices
            n += compare_readable(f"batch {name} stream {j}", info,
                                  lambda t: read.setdefault((j, t), b.planes(j, 0, t)), want)
        for t in (info["slice_begin"] - 1, info["slice_end"]):   # what is not held is an error, never stale data
            with pytest.raises(E.PvError, match="not held"):
                b.planes(0, 0, t)
        return n, info, read, b.launches
    finally:
        b.close()


BATCH_CASES = [c.name for c in A.CASES]


@pytest.mark.parametrize("name", BATCH_CASES)
def test_batch_planes(name, arithmetic):
    """every case under both arithmetic settings: the oracle's bits, and therefore the same bits under both"""
    c = A.BY_NAME[name]
    got = {}
    for arith in (FAST, EXACT):
        arithmetic(arith)
        with _kernels({batch_kernel(c.fft)}):
            n, info, got[arith], launches = batch_planes(name)
        # every slice the ring still holds, of every row; a stream that fits one launch is compared whole
        assert n == (info["slice_end"] - info["slice_begin"]) * len(A.streams(name)) and n >= 60
        assert launches > 1 or info["slice_begin"] == 0
        _report("batch", name, arith, {batch_kernel(c.fft)}, f"{n} of {info['slice_end'] * len(A.streams(name))} in {launches} launches")
    for key, a in got[FAST].items():
        b = got[EXACT][key]
        for k in ("mag", "phase", "rot", "outphase"):
            assert (a[k] is None) == (b[k] is None) and (a[k] is None or bits_equal(a[k], b[k])), (name, key, k)
        assert a["npk"] == b["npk"] and a["mode"] == b["mode"] and np.array_equal(a["peaks"], b["peaks"]), (name, key)


# ---- the single-stream engine ------------------------------------------------------------------------------------------
def engine_planes(name, j=0):
    """stream j through PhaseVocoder in BLOCK-frame calls (the offline loop, flush included); after every call the
    slices it launched are compared, each once.  Returns the number compared: all of the stream's."""
    c = A.BY_NAME[name]
    x = A.streams(name)[j]
    want, slices = _trace(name, j)
    cfg = E.make_config(1, fftsize=c.fft, **c.cfg)
    pv = E.PhaseVocoder(cfg.sample_rate, 1, cfg.time_ratio, cfg.pitch_semitones, cfg.mode, cfg.coremode, cfg.fftsize,
                        cfg.hopsize, 0)
    try:
        seen, frames, produced, pos, wrapped = set(), x.shape[1], 0, 0, False
        assert pv.plane_info()["slice_end"] == 0
        while pos < frames or produced < frames:
            blk = x[:, pos:pos + BLOCK] if pos < frames else np.zeros((1, BLOCK), np.float32)
            pv.processInData(blk)
            got = pv.getOutData(pv.getOutSamples()).shape[1]
            produced += got if pos < frames else min(got, max(frames - produced, 0))
            pos += BLOCK
            info = pv.plane_info()
            compare_readable(f"engine {name} stream {j}", info, lambda t: pv.planes(0, t), want, seen)
            wrapped = wrapped or info["slice_end"] > 17   # (the ring of the streaming path holds 17 slices)
        assert seen == set(range(slices)) and wrapped, (len(seen), slices)
        with pytest.raises(E.PvError, match="not held"):
            pv.planes(0, slices)
        return len(seen)
    finally:
        pv.close()


@pytest.mark.parametrize("fft", [1024, 4096])
@pytest.mark.parametrize("kind", FORM_KINDS)
def test_engine_planes(kind, fft, arithmetic):
    name = f"{kind}_{fft}"
    ariths = (FAST, EXACT) if fft == 1024 else (FAST,)
    for arith in ariths:
        arithmetic(arith)
        with _kernels({batch_kernel(fft)}):
            n = engine_planes(name, j=1 if kind == "ordinary" else 0)
        assert n >= 60
        _report("engine", name, arith, {batch_kernel(fft)}, n)


# ---- the stream pool ---------------------------------------------------------------------------------------------------
def pool_planes(name, mixed):
    """the case's streams in one pool, fed BLOCK frames per slot and call; after every feed each slot's new slices"""
    c = A.BY_NAME[name]
    xs = A.streams(name)
    kw = dict(pitch_range=(-12.0, 12.0)) if mixed else {}
    pool = E.StreamPool(len(xs), channels=1, fftsize=c.fft, **kw, **c.cfg)
    try:
        slots = [pool.open(semitones=c.cfg["semitones"]) if mixed else pool.open() for _ in xs]
        traces = [_trace(name, j) for j in range(len(xs))]
        seen = [set() for _ in xs]
        frames, produced, pos = xs[0].shape[1], [0] * len(xs), 0
        assert all(pool.plane_info(s)["slice_end"] == 0 for s in slots)
        while pos < frames or any(p < frames for p in produced):
            blocks = [x[:, pos:pos + BLOCK] if pos < frames else np.zeros((1, BLOCK), np.float32) for x in xs]
            pool.feed({s: b for s, b in zip(slots, blocks)})
            for j, s in enumerate(slots):
                got = pool.retrieve(s, pool.available(s)).shape[1]
                produced[j] += got if pos < frames else min(got, max(frames - produced[j], 0))
                compare_readable(f"{'pmix' if mixed else 'pool'} {name} slot {j}", pool.plane_info(s),
                                 lambda t: pool.planes(s, 0, t), traces[j][0], seen[j])
            pos += BLOCK
        for j in range(len(xs)):
            assert seen[j] == set(range(traces[j][1])), (j, len(seen[j]), traces[j][1])
        return sum(len(s) for s in seen)
    finally:
        pool.close_pool()


@pytest.mark.parametrize("fft", [1024, 4096])
@pytest.mark.parametrize("kind", FORM_KINDS + ("rows3",))
@pytest.mark.parametrize("set_", ["pool", "pmix"])
def test_pool_planes(set_, kind, fft, arithmetic):
    name = f"{kind}_{fft}"
    ariths = (FAST, EXACT) if fft == 1024 else (FAST,)
    for arith in ariths:
        arithmetic(arith)
        with _kernels({slot_kernel(set_, fft)}):
            n = pool_planes(name, mixed=set_ == "pmix")
        assert n >= 120
        _report(set_, name, arith, {slot_kernel(set_, fft)}, n)


# ---- the mixed batch ---------------------------------------------------------------------------------------------------
# per stream: (case kind, stream of the case, share of its frames, semitones, time ratio)
MB_DRAW = [("ordinary", 0, 1.0, 4.0, 1.0), ("mixed", 1, 0.8, -3.0, 1.0), ("holes", 0, 0.9, 7.0, 1.25),
           ("corners", 1, 1.0, 2.0, 0.8), ("outer", 0, 0.7, -5.0, 1.0), ("dcnyq", 0, 0.85, 4.0, 1.0),
           ("single", 0, 1.0, 4.0, 1.5)]


def mb_planes(fft, chunk=None):
    import torch
    draw = [(f"{kind}_{fft}", j, int(A.frames_of(fft) * share) // 4 * 4, semis, ratio)
            for kind, j, share, semis, ratio in MB_DRAW]
    clips = [A.streams(name)[j][:, :frames] for name, j, frames, _, _ in draw]
    with _env(**({} if chunk is None else dict(AUDIOMOD_PV_CHUNK_SLICES=str(chunk)))):
        mb = E.MixedBatch([(frames, semis, ratio) for _, _, frames, semis, ratio in draw], channels=1, block=BLOCK,
                          fftsize=fft, **A.SHIFT)
    try:
        assert all(mb.plane_info(i)["slice_end"] == 0 for i in range(len(draw)))
        mb.run(mb.pack(clips))
        torch.cuda.synchronize()
        n, hops = 0, set()
        for i, (name, j, frames, semis, ratio) in enumerate(draw):
            want, slices = _trace(name, j, frames, semis, ratio)
            info = mb.plane_info(i)
            assert info["slice_end"] == slices == mb.info(i)["slices"]
            hops.add(mb.info(i)["hop_in"])
            n += compare_readable(f"mb {fft} stream {i} ({name})", info, lambda t: mb.planes(i, 0, t), want)
            assert chunk is not None or info["slice_begin"] == 0
        assert len(hops) >= 3, hops   # streams with hops of their own in one launch
        return n
    finally:
        mb.close()


@pytest.mark.parametrize("fft", [512, 1024, 2048, 4096])
def test_mixed_batch_planes(fft, arithmetic):
    ariths = (FAST, EXACT) if fft == 1024 else (FAST,)
    for arith in ariths:
        arithmetic(arith)
        with _kernels({slot_kernel("mb", fft)}):
            n = mb_planes(fft)
        assert n >= 300
        _report("mb", f"draw_{fft}", arith, {slot_kernel("mb", fft)}, n)


# ---- forms that a variable read once per process selects: child processes ---------------------------------------------
CHILD_VARS = ("AUDIOMOD_PV_SPLIT_ANALYSIS", "AUDIOMOD_PV_CHUNK_SLICES", "AUDIOMOD_PV_STREAM_LAUNCHES", "AUDIOMOD_PV_EXACT",
              "AUDIOMOD_PV_CHAIN_CENSUS", "AUDIOMOD_PV_RESAMPLE_CENSUS")
CHILD_KINDS = ("ordinary", "mixed", "holes", "corners")


def child_main():
    """argv: what.  Runs the form's cases, compares, and prints one JSON line: per run the kernels the census saw and
    the slices compared.  A mismatch ends the child with the assertion's message."""
    what = sys.argv[1]
    E.chain_census(True)
    report = {}

    def run(key, f):
        before = E.analysis_census_read()
        n = f()
        after = E.analysis_census_read()
        report[key] = dict(kernels=sorted(k for k, v in after.items() if v - before.get(k, 0) > 0), slices=n)
    for arith in (FAST, EXACT):
        E.set_arithmetic(arith)
        if what == "nosplit":      # AUDIOMOD_PV_SPLIT_ANALYSIS=0: 4096-point frames on one wave
            for kind in A.LEVELS + A.CORNERS:
                run(f"{arith}/{kind}_4096", lambda: batch_planes(f"{kind}_4096")[0])
        elif what == "chunks":     # AUDIOMOD_PV_CHUNK_SLICES=8: many launches; what the ring still holds at the end
            for fft in (256, 1024, 4096, 8192):
                for kind in CHILD_KINDS:
                    def f(name=f"{kind}_{fft}"):
                        n, info, _, launches = batch_planes(name)
                        assert launches == -(-info["slice_end"] // 8) and launches >= 6
                        assert info["slice_end"] - info["slice_begin"] >= min(8, info["slice_end"] % 8 or 8)
                        assert info["slice_begin"] > 0 and n == 2 * (info["slice_end"] - info["slice_begin"])
                        return n
                    run(f"{arith}/{kind}_{fft}", f)
        elif what == "single":     # AUDIOMOD_PV_STREAM_LAUNCHES=single: pv_stream_kernel, at the sizes it serves
            for fft in (2048, 4096):
                for kind in CHILD_KINDS:
                    run(f"{arith}/{kind}_{fft}", lambda: engine_planes(f"{kind}_{fft}"))
    print("planes-child " + json.dumps(report))


def _child(what, **env):
    code = "import sys; sys.path.insert(0, %r); from tests import test_analysis_planes_gpu as T; T.child_main()" % (ROOT,)
    environ = {k: v for k, v in os.environ.items() if k not in CHILD_VARS}
    r = subprocess.run([sys.executable, "-c", code, what], capture_output=True, text=True, env=dict(environ, **env),
                       timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("planes-child ")]
    assert r.returncode == 0 and lines, (r.stdout + r.stderr)[-3000:]
    return {k: (set(map(tuple, v["kernels"])), v["slices"]) for k, v in json.loads(lines[-1][len("planes-child "):]).items()}


def test_batch_planes_4096_on_one_wave():
    rep = _child("nosplit", AUDIOMOD_PV_SPLIT_ANALYSIS="0")
    assert len(rep) == 2 * len(A.LEVELS + A.CORNERS)
    for key, (kernels, n) in rep.items():
        assert kernels == {batch_kernel(4096, split=False)} and n >= 100, (key, kernels, n)
        _report("batch-nosplit", key, int(key[0]), kernels, n)


def test_batch_planes_many_launches():
    rep = _child("chunks", AUDIOMOD_PV_CHUNK_SLICES="8")
    assert len(rep) == 2 * 4 * len(CHILD_KINDS)
    for key, (kernels, n) in rep.items():
        fft = int(key.rsplit("_", 1)[1])
        assert kernels == {batch_kernel(fft)} and n >= 2, (key, kernels, n)
        _report("batch-chunk8", key, int(key[0]), kernels, n)


def test_engine_planes_single_launch_kernel():
    rep = _child("single", AUDIOMOD_PV_STREAM_LAUNCHES="single")
    assert len(rep) == 2 * 2 * len(CHILD_KINDS)
    for key, (kernels, n) in rep.items():
        fft = int(key.rsplit("_", 1)[1])
        assert kernels == {("batch", "stream", fft // 2)} and n >= 40, (key, kernels, n)
        _report("engine-single", key, int(key[0]), kernels, n)
