"""Every overlap-add advance from 1 to the FFT size, on the GPU, in every engine form, against the oracle: the rows of
tests/ola_advance_signals.py (tests/test_ola_advance_host.py proves each row's regime on the oracle's record).

Forms: the single-stream engine in the row's blocks and in ragged calls; a Batch of 3 streams with distinct inputs and a
NaN-prefilled output -- as it comes (six rows stay on the tile path in most configurations) and on the fused path
(AUDIOMOD_PV_FUSED=2) with the default run count, AUDIOMOD_PV_CHAIN_RUNS=1 and =8 and a small
AUDIOMOD_PV_CHUNK_SLICES --; a StreamPool slot; a mixed-pool slot beside a slot of another pitch (time ratio, for the
time-stretch rows); a MixedBatch stream beside a clip of another length.  The pool and the mixed batch take fft 512 ...
4096.  Everything runs under both arithmetic settings.

Bars.  ROBOTIC rows: the oracle's per-call counts and its bits, no tolerance; where the oracle's output has non-finite
samples (an advance of N: the window sum under a frame's first sample is 0) the non-finite positions are identical and
the finite samples bit-equal.  Plain rows: the oracle's counts, whole-output RMS <= 1e-4, the error-shape bar of
tests/helpers.py against the oracle's own floor, and every form bit-equal to the single engine.  Undefined rows: every
form refuses with PV_ERR_UNSUPPORTED.  With AUDIOMOD_PARITY_SHAPE_LOG set, the comparisons made, the run lists' counts
and the census of the tile path's boundary are appended to that file (profiles/r20/ola_advance.txt)."""
import functools
import os

import numpy as np
import pytest

from audiomod_amd import engine as E
from oracle import oracle_py as O
from tests import ola_advance_signals as S
from tests.helpers import assert_shape, oracle_floor, parity_shape

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4
ARITHS = [E.ARITH_FAST, E.ARITH_EXACT]
ARITH_IDS = ["fast", "exact"]
RAGGED = [1, 479, 1100, 13, 480, 7, 333]   # then the rest of the clip in calls of 1000, then zero blocks
NBATCH = 3
CHUNK_SLICES = "5"
POOL_FFTS = (512, 1024, 2048, 4096)
UNSUPPORTED = "unsupported configuration"   # pv_strerror(PV_ERR_UNSUPPORTED)
# Batch of 3 on the fused path with AUDIOMOD_PV_CHAIN_RUNS=8: (the largest run count of a launch, any warm-up entry), as
# ChainBuilder::end_launch cuts the row's launches (a run needs two slices, and a warm-up of at most half a run)
MULTI_RUN = {
    "rob512_h63": (8, True), "rob512_h64": (8, True), "rob512_h65": (8, True), "rob512_h255": (4, True),
    "rob512_h256": (8, True), "rob512_h257": (8, True), "rob512_h507": (8, True), "rob512_h508": (8, True),
    "rob512_h509": (8, True), "rob512_h511": (8, True), "rob512_h512": (8, False), "rob1024_h253": (4, True),
    "rob1024_h509": (4, True), "rob1024_h512": (8, True), "rob1024_h515": (8, True), "rob1024_h765": (8, True),
    "rob1024_h769": (8, True), "rob1024_h1021": (4, True), "rob1024_h1023": (4, True), "rob1024_h1024": (4, False),
    "rob2048_h2045": (8, True), "rob2048_h2047": (8, True), "rob2048_h2048": (8, False), "rob4096_h4093": (4, True),
    "rob256_h255": (4, True), "rob256_h256": (4, False), "rob8192_h8189": (4, True), "p1024_+7_h340": (8, True),
    "p2048_+7_h1020": (8, True), "p2048_+4_h1621": (4, True), "p1024_+12_h511": (8, True),
    "p1024_+12_h512": (8, False), "p512_+4_h406": (8, True), "s512_1.5_h341_core2": (4, True),
    "s512_1.5_h340_core0": (4, True), "g512_-7_h300": (4, True), "s2048_1.5_h1360": (4, True),
}


@pytest.fixture(autouse=True)
def census_off_afterwards():
    yield
    E.chain_census(False)


def log(text):
    path = os.environ.get("AUDIOMOD_PARITY_SHAPE_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(text + "\n")


def tag(arith):
    return "exact" if arith else "fast"


def same_where_finite(got, want):
    """the same shape, the same non-finite positions, and the same bits wherever the samples are finite (all of them,
    in most rows: then this is helpers.bits_equal)"""
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    fin = np.isfinite(want)
    return bool(np.array_equal(np.isfinite(got), fin) and np.array_equal(got.view(np.uint32)[fin], want.view(np.uint32)[fin]))


def where(got, want):
    if got.shape != want.shape:
        return f"shapes {got.shape} {want.shape}"
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = (np.isfinite(g) != np.isfinite(w)) | (np.isfinite(w) & (g.view(np.uint32) != w.view(np.uint32)))
    m = np.argwhere(bad)
    return f"{len(m)} differ, first {m[:6].tolist()}: " + str([(float(g[tuple(i)]), float(w[tuple(i)])) for i in m[:6]])


@functools.lru_cache(maxsize=None)
def floor(name, arith, stream):
    row = S.BY_NAME[name]
    return oracle_floor(O.run_offline, S.clip(name, stream), arith, want=S.oracle(name, stream).y, block=row.block,
                        flush=True, **row.cfg)


def held(label, name, got, arith, stream=0):
    """one output against the oracle under the row's bar; writes the comparison to the log"""
    row = S.BY_NAME[name]
    want = S.oracle(name, stream).y
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = int(np.count_nonzero(~np.isfinite(want)))
    if row.kind == "robotic":
        ok = same_where_finite(got, want)
        log(f"{label} [{tag(arith)}] bits vs oracle{f' ({bad} non-finite in place)' if bad else ''}: "
            f"{'equal' if ok else 'DIFFER'}")
        assert ok, (label, where(got, want))
        return
    s = parity_shape(got, want)   # (inf where the non-finite positions do not coincide)
    print(f"{label}: rms {s['rms']:.3e} max_abs {s['max_abs']:.3e} win_rms {s['win_rms']:.3e}")
    assert s["rms"] <= RMS_TOL, (label, s)
    assert_shape(label + (f" ({bad} non-finite in place)" if bad else ""), got, want, floor(name, arith, stream), arith)


# ---- the forms
def run_engine(name):
    row = S.BY_NAME[name]
    return E.run_offline(S.clip(name), block=row.block, flush=True, **row.cfg)


def run_ragged(name, want_len):
    """ragged calls, the rest of the clip in calls of 1000, then zero blocks until want_len frames have come out: the
    stream does not depend on how the calls cut it"""
    row = S.BY_NAME[name]
    x = S.clip(name)
    cfg = E.make_config(row.channels, **row.cfg)
    pv = E.PhaseVocoder(cfg.sample_rate, row.channels, cfg.time_ratio, cfg.pitch_semitones, cfg.mode, cfg.coremode,
                        cfg.fftsize, cfg.hopsize)
    calls = list(RAGGED)
    while sum(calls) < row.frames:
        calls.append(min(1000, row.frames - sum(calls)))
    pos, outs, produced = 0, [], 0
    for n in calls:
        pv.processInData(x[:, pos:pos + n])
        pos += n
        outs.append(pv.getOutData(pv.getOutSamples()))
        produced += outs[-1].shape[1]
    assert pos == row.frames
    zeros = np.zeros((row.channels, S.BLOCK), np.float32)
    for _ in range(400):
        if produced >= want_len:
            break
        pv.processInData(zeros)
        outs.append(pv.getOutData(pv.getOutSamples()))
        produced += outs[-1].shape[1]
    pv.close()
    return np.concatenate(outs, axis=1)[:, :want_len]


def run_batch(name, streams=tuple(range(NBATCH))):
    import torch
    row = S.BY_NAME[name]
    x = np.stack([S.clip(name, s) for s in streams])
    b = E.Batch(len(streams), row.frames, channels=row.channels, block=row.block, flush=True, **row.cfg)
    out = b.run(torch.from_numpy(x).cuda(), d_out=torch.full((len(streams), row.channels, b.out_frames), float("nan"),
                                                               device="cuda"))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    runs = [b.chain_runs(i) for i in range(b.launches)]
    b.close()
    return out, runs


def other_setting(name):
    """the neighbour of a row's slot in a mixed pool: another time ratio for the time-stretch rows, else another pitch;
    never one with larger advances than the row's own.  (key, own value, the neighbour's)"""
    cfg = S.config(name)
    if cfg["mode"] == "time_stretch":
        return "time_ratio", cfg["time_ratio"], cfg["time_ratio"] * 0.75
    return "semitones", cfg.get("semitones", 0.0), cfg.get("semitones", 0.0) - 3.0


def make_pool(name, mixed):
    row = S.BY_NAME[name]
    if not mixed:
        pool = E.StreamPool(3, channels=row.channels, **row.cfg)
        pool.open()
        return pool, pool.open()
    key, own, other = other_setting(name)
    rng = {"pitch_range" if key == "semitones" else "ratio_range": (min(own, other), max(own, other))}
    pool = E.StreamPool(3, channels=row.channels, **rng, **row.cfg)
    pool.open(**{key: other})
    return pool, pool.open(**{key: own})


def run_pool(name, mixed):
    """the offline loop on one slot: the row's blocks, then zero blocks until the clip's length has come out"""
    row = S.BY_NAME[name]
    pool, slot = make_pool(name, mixed)
    x, got, counts, produced = S.clip(name), [], [], 0

    def call(blk):
        nonlocal produced
        pool.feed({slot: blk})
        n = pool.available(slot)
        counts.append(n)
        y = pool.retrieve(slot, n)
        assert y.shape[1] == n
        return y

    for i in range(0, row.frames, row.block):
        got.append(call(x[:, i:i + row.block]))
        produced += got[-1].shape[1]
    zeros = np.zeros((row.channels, row.block), np.float32)
    while produced < row.frames:
        y = call(zeros)
        w = min(y.shape[1], row.frames - produced)
        got.append(y[:, :w])
        produced += w
        assert len(counts) < 4000
    pool.close_pool()
    return np.concatenate(got, axis=1), counts


def mixed_batch_streams(name):
    row = S.BY_NAME[name]
    cfg = S.config(name)
    st, tr = cfg.pop("semitones", 0.0), cfg.pop("time_ratio", 1.0)
    return [(row.frames, st, tr), (row.frames - 1234, st, tr)], cfg


def run_mixed_batch(name):
    import torch
    row = S.BY_NAME[name]
    streams, cfg = mixed_batch_streams(name)
    mb = E.MixedBatch(streams, channels=row.channels, block=row.block, flush=True, **cfg)
    out = mb.run(mb.pack([S.clip(name), S.clip(name, 1)[:, :row.frames - 1234]]))
    torch.cuda.synchronize()
    y = mb.split(out)[0].cpu().numpy()
    mb.close()
    return y


CASES = [(n, a) for n in S.SERVED for a in ARITHS]


def case_id(case):
    return f"{case[0]}-{tag(case[1])}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_single_stream_forms(case):
    """the single engine (the row's blocks; ragged calls), a pool slot, a mixed-pool slot, a mixed-batch stream"""
    name, arith = case
    run = S.oracle(name)
    prev = E.set_arithmetic(arith)
    try:
        got, counts = run_engine(name)
        assert list(counts) == list(run.counts), (name, counts[:12], run.counts[:12])
        held(f"{name} engine", name, got, arith)
        forms = {}
        if name not in S.OVERRUN:   # (where slices are dropped the stream depends on the calls)
            forms["ragged"] = run_ragged(name, got.shape[1])
        if S.fft_of(name) in POOL_FFTS:
            for mixed in (False, True):
                y, pc = run_pool(name, mixed)
                assert pc == list(run.counts), (name, mixed, pc[:12], run.counts[:12])
                forms["mixed_pool" if mixed else "pool"] = y
            forms["mixed_batch"] = run_mixed_batch(name)
        for form, y in forms.items():
            ok = same_where_finite(y, got)
            log(f"{name} {form} [{tag(arith)}] bits vs the single engine: {'equal' if ok else 'DIFFER'}")
            assert ok, (name, form, where(y, got))
        assert len(forms) == (3 if S.fft_of(name) in POOL_FFTS else 0) + (0 if name in S.OVERRUN else 1), sorted(forms)
    finally:
        E.set_arithmetic(prev)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_batch_forms(case, monkeypatch):
    """Batch of 3 distinct streams, NaN-prefilled output.  Six rows are too few for the fused kernel by default (Core::init:
    below 192 rows a batch stays on the frame ring and the overlap-add tiles unless the configuration has a free-form
    kernel, drops slices or exceeds the tiles' frame limit), so the batch runs as it comes and then on the fused path
    (AUDIOMOD_PV_FUSED=2, a non-empty chain census) with the default run count, one run, eight runs wanted and launches
    of five slices.  Eight runs wanted must really split the rows of MULTI_RUN, with warm-up copies where frames
    overlap."""
    name, arith = case
    row = S.BY_NAME[name]
    prev = E.set_arithmetic(arith)
    try:
        first = None
        fused = {"AUDIOMOD_PV_FUSED": "2"}
        for label, env in (("as it comes", {}), ("fused", fused), ("fused runs=1", dict(fused, AUDIOMOD_PV_CHAIN_RUNS="1")),
                           ("fused runs=8", dict(fused, AUDIOMOD_PV_CHAIN_RUNS="8")),
                           ("fused chunk=5", dict(fused, AUDIOMOD_PV_CHUNK_SLICES=CHUNK_SLICES))):
            with monkeypatch.context() as m:
                for k, v in env.items():
                    m.setenv(k, v)
                E.chain_census(True)
                out, runs = run_batch(name)
                census = E.chain_census_read()[0]
            log(f"{name} batch{NBATCH} {label} [{tag(arith)}] fused launches {sum(census.values())} launches {len(runs)} "
                f"runs {sorted({r for r, _ in runs})} warm-up entries {sum(w for _, w in runs)}")
            if env and S.fft_of(name) in POOL_FFTS:   # (the census keys the wave-FFT kernels; 256 and 8192 run the generic one)
                assert census and all(k[0] == "batch" for k in census), (name, label, census)
            if label == "fused runs=1":
                assert {r for r, _ in runs} == {1} and sum(w for _, w in runs) == 0, runs
            if label == "fused runs=8" and name in MULTI_RUN:
                want_runs, warm = MULTI_RUN[name]
                assert max(r for r, _ in runs) == want_runs, (name, runs)
                assert (sum(w for _, w in runs) > 0) == warm, (name, runs)
            for s in range(NBATCH):
                held(f"{name} batch{NBATCH} {label} stream {s}", name, out[s], arith, stream=s)
            if first is None:
                first = out
            else:   # the run lists and the launches' cut change nothing
                assert same_where_finite(out, first), (name, label, where(out, first))
        if row.kind == "plain":   # ... and stream 0 is the single engine's output, bit for bit (Batch(1) == engine)
            got, _ = run_engine(name)
            assert same_where_finite(first[0], got), (name, where(first[0], got))
    finally:
        E.set_arithmetic(prev)


# ---- the run lists (ChainBuilder::end_launch) through pv_debug_batch_chain_runs
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_run_lists(arith, monkeypatch):
    prev = E.set_arithmetic(arith)
    try:
        monkeypatch.setenv("AUDIOMOD_PV_CHAIN_RUNS", "8")
        monkeypatch.setenv("AUDIOMOD_PV_FUSED", "2")   # (the fused path whatever the row count)
        got = {}
        for name in ("rob512_h1", "rob512_h512", "rob512_h64", "rob1024_h253"):
            row = S.BY_NAME[name]
            b = E.Batch(NBATCH, row.frames, channels=row.channels, **row.cfg)
            got[name] = [b.chain_runs(i) for i in range(b.launches)]
            with pytest.raises(E.PvError):
                b.chain_runs(b.launches)
            with pytest.raises(E.PvError):
                b.chain_runs(-1)
            b.close()
            log(f"{name} run lists, 8 runs wanted [{tag(arith)}]: (runs, warm-up entries) per launch {got[name]}")
        # hop 1: 512 frames reach into every sample; no cut of a launch has a warm-up of at most half a run
        assert all(r < 8 for r, _ in got["rob512_h1"]), got["rob512_h1"]
        assert any(r == 1 for r, _ in got["rob512_h1"]), got["rob512_h1"]   # ... and falls back to one run
        # hop = N: frames do not overlap, nothing to warm up
        assert any(r > 1 for r, _ in got["rob512_h512"]) and all(w == 0 for _, w in got["rob512_h512"]), got["rob512_h512"]
        for name in ("rob512_h64", "rob1024_h253"):   # ordinary: several runs, each later one with its warm-up
            assert any(r > 1 and w >= r - 1 for r, w in got[name]), (name, got[name])
    finally:
        E.set_arithmetic(prev)


# ---- the tile path (frame ring + overlap-add tiles) and its limit of frames per tile
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
def test_tile_path_limit_between_hop_7_and_hop_6(arith, monkeypatch):
    """Core::init, kMaxTileFrames: ROBOTIC at fft 512 fits the tile path's 128 frames per tile at hop 7, not at hop 6.  A
    batch of three streams takes the tile path by default where it has the choice (reference-order arithmetic, or no
    free-form fused kernel for the configuration): then no fused launch at hop 7, fused launches at hop 6; both are the
    oracle's bits.  Under AUDIOMOD_PV_FUSED=0 hop 6 is the named refusal."""
    prev = E.set_arithmetic(arith)
    try:
        census = {}
        for name in ("rob512_h7", "rob512_h6"):
            E.chain_census(True)
            out, _ = run_batch(name)
            census[name] = E.chain_census_read()[0]
            log(f"{name} batch{NBATCH} [{tag(arith)}] fused launches {sorted(census[name].items())}")
            for s in range(NBATCH):
                held(f"{name} batch{NBATCH} boundary stream {s}", name, out[s], arith, stream=s)
        assert census["rob512_h7"] == {}, census   # (ROBOTIC has no free-form kernel: the same under either setting)
        assert census["rob512_h6"] and all(k[0] == "batch" and k[1] == 256 for k in census["rob512_h6"]), census
        monkeypatch.setenv("AUDIOMOD_PV_FUSED", "0")
        E.chain_census(True)
        out, _ = run_batch("rob512_h7")
        assert E.chain_census_read()[0] == {}
        for s in range(NBATCH):
            held(f"rob512_h7 batch{NBATCH} tile path stream {s}", "rob512_h7", out[s], arith, stream=s)
        row = S.BY_NAME["rob512_h6"]
        with pytest.raises(E.PvError) as e:
            E.Batch(NBATCH, row.frames, channels=2, **row.cfg)
        assert UNSUPPORTED in str(e.value) and "hop too small relative to the FFT size for the OLA tile" in str(e.value)
        assert E.chain_census_read()[0] == {}
    finally:
        E.set_arithmetic(prev)


TILE_ROWS = [r.name for r in S.ROBOTIC_ROWS if r.cfg["hopsize"] >= 63]


@pytest.mark.parametrize("name", TILE_ROWS)
def test_larger_hops_on_the_tile_path_equal_the_fused_result(name, monkeypatch):
    """AUDIOMOD_PV_FUSED=0 (the frame ring and the overlap-add tiles: an empty chain census) against AUDIOMOD_PV_FUSED=2
    (the fused kernel: a non-empty one), bit for bit"""
    for arith in ARITHS:
        prev = E.set_arithmetic(arith)
        try:
            with monkeypatch.context() as m:
                m.setenv("AUDIOMOD_PV_FUSED", "2")
                E.chain_census(True)
                fused, fused_runs = run_batch(name)
                if S.fft_of(name) in POOL_FFTS:
                    assert E.chain_census_read()[0], name
                else:   # (the census keys the wave-FFT kernels; 256 and 8192 run the generic one: only it splits into runs)
                    assert any(r > 1 for r, _ in fused_runs), (name, fused_runs)
            with monkeypatch.context() as m:
                m.setenv("AUDIOMOD_PV_FUSED", "0")
                E.chain_census(True)
                tiles, _ = run_batch(name)
                assert E.chain_census_read()[0] == {}
            ok = same_where_finite(tiles, fused)
            log(f"{name} batch{NBATCH} tile path [{tag(arith)}] bits vs the fused path: {'equal' if ok else 'DIFFER'}")
            assert ok, (name, where(tiles, fused))
            held(f"{name} batch{NBATCH} tile path stream 0", name, tiles[0], arith)
        finally:
            E.set_arithmetic(prev)


# ---- above N: undefined in the reference, refused by every form
@pytest.mark.parametrize("arith", ARITHS, ids=ARITH_IDS)
@pytest.mark.parametrize("name", [r.name for r in S.ROWS if r.kind == S.UNDEFINED])
def test_undefined_rows_are_refused_by_every_form(name, arith):
    row = S.BY_NAME[name]
    x = S.clip(name)
    prev = E.set_arithmetic(arith)

    def pool(mixed):
        p, slot = make_pool(name, mixed)
        try:
            for i in range(0, row.frames, row.block):
                p.feed({slot: x[:, i:i + row.block]})
                p.retrieve(slot, p.available(slot))
        finally:
            p.close_pool()

    try:
        streams, cfg = mixed_batch_streams(name)
        forms = {"engine": lambda: run_engine(name),
                 "ragged": lambda: run_ragged(name, row.frames),
                 "batch": lambda: E.Batch(NBATCH, row.frames, channels=row.channels, **row.cfg),
                 "pool": lambda: pool(False),
                 "mixed_pool": lambda: pool(True),
                 "mixed_batch": lambda: E.MixedBatch(streams, channels=row.channels, **cfg)}
        for form, run in forms.items():
            with pytest.raises(E.PvError) as e:
                run()
            log(f"{name} {form} [{tag(arith)}] refused: {e.value}")
            assert UNSUPPORTED in str(e.value), (form, str(e.value))
    finally:
        E.set_arithmetic(prev)
