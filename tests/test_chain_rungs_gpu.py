"""Every instantiation of the fused synthesis + overlap-add kernel, in all four sets, on the GPU.

tests/test_chain_rungs_host.py holds the table: one entry per rung of the ladder (60) plus second routes into the
all-modes kernel.  Each entry runs here through each set -- Batch (pv_synth_chain_kernel), StreamPool
(pv_pool_synth_chain_kernel), a mixed StreamPool (pv_pmix_*) and MixedBatch (pv_mb_*) -- at the smallest shapes that
still carry state: 2 channels, 24 000 frames, 3 streams with their own signals, 4 slices per launch for the batches and
480-frame calls for the pools.  Per case:
  1. the library's census (engine.chain_census_read) shows that exactly the entry's instantiation of this set was
     launched, no other set's, and the slot-table analysis / resampler kernels that go with it;
  2. every stream against the oracle: counts, RMS <= 1e-4 and the error-shape bar of tests/helpers.py; robotic entries
     under PV_ARITH_EXACT bit for bit;
  3. the contract between the sets, bit for bit: pool and pmix slots against the single-stream engine fed the same
     blocks, batch and mb streams against Batch(1, frames) of the stream.
The specialisation tests run the plain entries once more in child processes, with and without AUDIOMOD_PV_SYNTH_GENERIC:
the specialised kernels and the all-modes kernel of every set must write the same bits under PV_ARITH_EXACT."""
import contextlib
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import assert_shape, bits_equal, oracle_floor, parity_shape
from tests.test_chain_rungs_host import (BLOCK, BY_NAME, CASES, CHUNK_SLICES, EXACT, FAST, FRAMES, MB_FRAMES, PLAIN,
                                         case_id, config)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RMS_TOL = 1e-4   # BASELINE's contract (tests/test_gpu_parity.py RMS_TOL)
SETS = E.CENSUS_SETS
SEED = 4100


@functools.lru_cache(maxsize=None)
def _signal(frames, stream):
    x = signals.voice(frames, 2, seed=SEED, stream=stream)
    x.setflags(write=False)
    return x


def _key(cfg):
    return tuple(sorted(cfg.items()))


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


# ---- one entry through one set: a list of (frames, stream index, configuration, output, per-call counts or None)
def _batch_env(entry):
    env = dict(AUDIOMOD_PV_CHUNK_SLICES=str(CHUNK_SLICES))
    if not entry.rung[3]:   # without a free-form kernel few rows take the tile path: the fused one, whatever the rows
        env["AUDIOMOD_PV_FUSED"] = "2"
    return env


def run_batch(entry):
    import torch
    cfg = config(entry)
    xs = np.stack([_signal(FRAMES, s) for s in range(3)])
    with _env(**_batch_env(entry)):
        b = E.Batch(3, FRAMES, channels=2, block=BLOCK, **cfg)
    assert b.launches >= 3 and b.slices >= 16, (b.launches, b.slices)
    out = b.run(torch.from_numpy(xs).cuda(), d_out=torch.full((3, 2, b.out_frames), float("nan"), device="cuda"))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    b.close()
    return [(FRAMES, s, cfg, out[s], None) for s in range(3)]


def _drive_pool(pool, slots, xs):
    """engine.run_offline's loop (the reference CLI's) on every slot at once"""
    n = len(slots)
    outs, counts, produced = [[] for _ in slots], [[] for _ in slots], [0] * n
    for i in range(0, FRAMES, BLOCK):
        pool.feed({s: xs[j][:, i:i + BLOCK] for j, s in enumerate(slots)})
        for j, s in enumerate(slots):
            got = pool.available(s)
            outs[j].append(pool.retrieve(s, got))
            counts[j].append(got)
            produced[j] += got
    z = np.zeros((2, BLOCK), np.float32)
    while any(p < FRAMES for p in produced):
        live = [j for j in range(n) if produced[j] < FRAMES]
        pool.feed({slots[j]: z for j in live})
        for j in live:
            got = pool.available(slots[j])
            y = pool.retrieve(slots[j], got)
            counts[j].append(got)
            w = min(got, FRAMES - produced[j])
            outs[j].append(y[:, :w])
            produced[j] += w
    return [np.concatenate(o, axis=1) for o in outs], counts


def run_pool(entry):
    cfg = config(entry)
    pool = E.StreamPool(3, channels=2, **cfg)
    slots = [pool.open() for _ in range(3)]
    outs, counts = _drive_pool(pool, slots, [_signal(FRAMES, s) for s in range(3)])
    pool.close_pool()
    return [(FRAMES, s, cfg, outs[s], counts[s]) for s in range(3)]


def run_pmix(entry):
    ratios = [r for _, r in entry.values]
    if max(ratios) != min(ratios):
        ranges = dict(ratio_range=(min(ratios), max(ratios)))
    else:
        ranges = dict(pitch_range=(-12.0, 12.0))
    pool = E.StreamPool(3, channels=2, **ranges, **config(entry))
    slots = [pool.open(semitones=s, time_ratio=r) for s, r in entry.values]
    outs, counts = _drive_pool(pool, slots, [_signal(FRAMES, s) for s in range(3)])
    pool.close_pool()
    return [(FRAMES, s, config(entry, entry.values[s]), outs[s], counts[s]) for s in range(3)]


def run_mb(entry):
    import torch
    streams = [(f, s, r) for f, (s, r) in zip(MB_FRAMES, entry.values)]
    with _env(AUDIOMOD_PV_CHUNK_SLICES=str(CHUNK_SLICES)):
        mb = E.MixedBatch(streams, channels=2, block=BLOCK, **entry.kw)
    assert mb.launches >= 3, mb.launches
    y = mb.run(mb.pack([_signal(f, i) for i, f in enumerate(MB_FRAMES)]))
    torch.cuda.synchronize()
    outs = [v.cpu().numpy() for v in mb.split(y)]
    mb.close()
    return [(f, i, config(entry, entry.values[i]), outs[i], None) for i, f in enumerate(MB_FRAMES)]


RUN = dict(batch=run_batch, pool=run_pool, pmix=run_pmix, mb=run_mb)


# ---- references, computed once per (signal, configuration[, arithmetic]) and shared by the sets
@functools.lru_cache(maxsize=None)
def _oracle(frames, stream, cfg):
    want, counts, _ = O.run_offline(_signal(frames, stream), block=BLOCK, **dict(cfg))
    want.setflags(write=False)
    return want, tuple(counts)


@functools.lru_cache(maxsize=None)
def _floor(frames, stream, cfg, arith):
    want = _oracle(frames, stream, cfg)[0]
    return oracle_floor(O.run_offline, _signal(frames, stream), arith, want=want, block=BLOCK, **dict(cfg))


@functools.lru_cache(maxsize=None)
def _single_stream(frames, stream, cfg, arith):
    assert E.get_arithmetic() == arith
    y, counts = E.run_offline(_signal(frames, stream), block=BLOCK, **dict(cfg))
    y.setflags(write=False)
    return y, tuple(counts)


@functools.lru_cache(maxsize=None)
def _batch_of_one(frames, stream, cfg, arith):
    import torch
    assert E.get_arithmetic() == arith
    b = E.Batch(1, frames, channels=2, block=BLOCK, **dict(cfg))
    y = b.run(torch.from_numpy(np.array(_signal(frames, stream)[None])).cuda())
    torch.cuda.synchronize()
    y = y.cpu().numpy()[0]
    b.close()
    y.setflags(write=False)
    return y


# ---- the census
@pytest.fixture(scope="module", autouse=True)
def census():
    """On for the module.  Where AUDIOMOD_PV_CHAIN_CENSUS already switched it on for the process it is left alone (the
    counts are written out at exit); the tests below read differences only."""
    if not os.environ.get("AUDIOMOD_PV_CHAIN_CENSUS"):
        E.chain_census(True)
        yield
        E.chain_census(False)
    else:
        yield


def _delta(after, before):
    return [{k: v - b.get(k, 0) for k, v in a.items() if v - b.get(k, 0) > 0} for a, b in zip(after, before)]


def expected_census(set_, entry):
    nc, _, res, fast = entry.rung
    chain = {(set_,) + tuple(entry.rung)}
    if set_ == "batch":   # the batch path has its own analysis and resampling launchers
        return chain, set(), set()
    ana = {(set_, nc, 1 if nc == 2048 else 0)}   # 4096 points: the two-wave kernel
    if not res:
        return chain, set(), ana
    interp = 0 if entry.values[0][0] in (12.0, -12.0) else 1
    # the mixed batch has a resampling kernel of its own for the free-form arithmetic only; in the reference's order it
    # launches the mixed pool's
    res_set = "pmix" if set_ == "mb" and not fast else set_
    return chain, {(res_set, fast, interp)}, ana


@pytest.fixture
def arithmetic():
    prev = E.get_arithmetic()
    yield E.set_arithmetic
    E.set_arithmetic(prev)


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("set_", SETS)
def test_rung(set_, case, arithmetic):
    name, arith = case
    entry = BY_NAME[name]
    arithmetic(arith)
    before = E.chain_census_read()
    streams = RUN[set_](entry)
    chain, res, ana = _delta(E.chain_census_read(), before)
    want_chain, want_res, want_ana = expected_census(set_, entry)
    # 1. the instantiation that ran: this one, of this set, and nothing else
    assert set(chain) == want_chain, (chain, want_chain)
    assert set(res) == want_res, (res, want_res)
    assert set(ana) == want_ana, (ana, want_ana)
    for frames, i, cfg, got, counts in streams:
        label = f"{set_} {case_id(case)} stream {i}"
        k = _key(cfg)
        # 2. the oracle
        want, wc = _oracle(frames, i, k)
        if counts is not None:
            assert list(counts) == list(wc), label
        assert got.shape == want.shape, (label, got.shape, want.shape)
        assert want.shape[1] > 0 and float(np.abs(want).max()) > 0.01, label   # there is audio to compare
        if cfg["mode"] == "robotic" and arith == EXACT:
            assert bits_equal(got, want), label
        shape = parity_shape(got, want)
        print(f"{label}: rms {shape['rms']:.3e} max_abs {shape['max_abs']:.3e} win_rms {shape['win_rms']:.3e}")
        assert shape["rms"] <= RMS_TOL, (label, shape)
        assert_shape(label, got, want, _floor(frames, i, k, arith), arith)
        # 3. the other engines of the same stream, bit for bit
        if set_ in ("pool", "pmix"):
            ref, rc = _single_stream(frames, i, k, arith)
            assert list(counts) == list(rc), label
        else:
            ref = _batch_of_one(frames, i, k, arith)
        assert bits_equal(got, ref), (label, got.shape, ref.shape)


# ---- specialisations against the all-modes kernel: the variable is read once per process, hence child processes
def child_main():
    """argv: set, output file.  Every plain entry under PV_ARITH_EXACT through one set; saves outputs and census."""
    set_, path = sys.argv[1], sys.argv[2]
    assert E.get_arithmetic() == EXACT   # AUDIOMOD_PV_EXACT=1
    E.chain_census(True)
    arrays = {}
    for entry in PLAIN:
        for _, i, _, got, _ in RUN[set_](entry):
            arrays[f"{entry.name}/{i}"] = got
    chain = E.chain_census_read()[0]
    np.savez(path, census=np.array(json.dumps(sorted(chain))), **arrays)
    print("chain-child ok", len(arrays))


def _child(set_, path, **env):
    code = "import sys; sys.path.insert(0, %r); from tests import test_chain_rungs_gpu as T; T.child_main()" % (ROOT,)
    environ = {k: v for k, v in os.environ.items() if k != "AUDIOMOD_PV_SYNTH_GENERIC"}
    r = subprocess.run([sys.executable, "-c", code, set_, path], capture_output=True, text=True,
                       env=dict(environ, AUDIOMOD_PV_EXACT="1", **env), timeout=300)
    assert r.returncode == 0 and f"chain-child ok {3 * len(PLAIN)}" in r.stdout, (r.stdout + r.stderr)[-3000:]
    z = np.load(path)
    return z, {tuple(k) for k in json.loads(str(z["census"]))}


@pytest.mark.parametrize("set_", SETS)
def test_specialisations_are_bit_identical_to_the_all_modes_kernel(set_, tmp_path):
    spec, spec_census = _child(set_, str(tmp_path / "spec.npz"))
    assert spec_census == {(set_,) + tuple(e.rung) for e in PLAIN}, spec_census
    gen, gen_census = _child(set_, str(tmp_path / "generic.npz"), AUDIOMOD_PV_SYNTH_GENERIC="1")
    assert gen_census == {(set_, e.rung[0], -1, e.rung[2], 0) for e in PLAIN}, gen_census
    pairs = 0
    for entry in PLAIN:
        for i in range(3):
            a, b = spec[f"{entry.name}/{i}"], gen[f"{entry.name}/{i}"]
            assert a.shape[1] > 0 and bits_equal(a, b), (set_, entry.name, i)
        pairs += 1
    assert pairs == 24   # 4 sizes x 3 core modes x with / without resampling, per set


def test_the_census_file_receives_a_process_counts_at_exit(tmp_path):
    """AUDIOMOD_PV_CHAIN_CENSUS: on from the start, appended to when the process ends, one line per key"""
    path = tmp_path / "census.txt"
    path.write_text("kept\n")
    code = ("import sys; sys.path.insert(0, %r); from tests import test_chain_rungs_gpu as T; "
            "T.run_pool(T.BY_NAME['shift_2048_c1_fast']); print('census-child ok')" % (ROOT,))
    environ = {k: v for k, v in os.environ.items() if k not in ("AUDIOMOD_PV_EXACT", "AUDIOMOD_PV_SYNTH_GENERIC")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       env=dict(environ, AUDIOMOD_PV_CHAIN_CENSUS=str(path)), timeout=300)
    assert r.returncode == 0 and "census-child ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    lines = path.read_text().splitlines()
    assert lines[0] == "kept"
    keys = sorted(l.rsplit(" ", 1)[0] for l in lines[1:])
    assert keys == ["analyze set=pool nc=1024 split=0", "chain set=pool nc=1024 core=1 res=1 fast=1",
                    "phase set=pool form=fused b=8", "resample set=pool fast=1 interp=1"], lines
    assert all(int(l.rsplit("count=", 1)[1]) > 0 for l in lines[1:]), lines
