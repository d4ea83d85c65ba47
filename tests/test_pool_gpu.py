"""Stream pool on the GPU: every slot must behave bit for bit like a single-stream engine (PhaseVocoder / pv_engine)
of the same configuration fed the same blocks, whatever the other slots do."""
import numpy as np
import pytest

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import bits_equal

pytestmark = pytest.mark.gpu

SPECIAL = (0, 1, 13, 479, 4097, 9000)


def _cfg_args(kw):
    cfg = E.make_config(2, **kw)
    return (cfg.sample_rate, 2, cfg.time_ratio, cfg.pitch_semitones, cfg.mode, cfg.coremode, cfg.fftsize, cfg.hopsize)


def _sizes(rng, ncalls):
    n = [int(v) for v in rng.integers(200, 900, ncalls)]
    for j, v in enumerate(rng.permutation(SPECIAL)):
        n[(3 * j + 1) % ncalls] = int(v)
    return n


class _Stream:
    """One logical stream: its input, its call sizes and the single-stream engine it must match."""

    def __init__(self, kw, seed, ncalls, rng):
        self.sizes = _sizes(rng, ncalls)
        self.x = signals.voice(sum(self.sizes) + 1, 2, seed=seed)
        self.pos = 0
        self.k = 0
        self.ref = E.PhaseVocoder(*_cfg_args(kw))
        self.out, self.ref_out = [], []

    def next_block(self):
        n = self.sizes[self.k % len(self.sizes)]
        self.k += 1
        blk = self.x[:, self.pos:self.pos + n]
        if blk.shape[1] < n:
            blk = np.zeros((2, n), np.float32)
        self.pos += n
        return np.ascontiguousarray(blk)


def _check_identity(kw, nslots=6, ncalls=30, seed=11, reopen=True, refuse_at=None):
    rng = np.random.default_rng(seed)
    pool = E.StreamPool(nslots, channels=2, **kw)
    live = {}  # slot -> _Stream
    sid = 0
    for call in range(ncalls):
        if call % 2 == 0 and len(live) < nslots:  # staggered joins
            s = pool.open()
            assert s not in live
            live[s] = _Stream(kw, 100 + sid, ncalls, rng)
            sid += 1
        if reopen and call == ncalls // 2:  # one slot closes and comes back as a fresh stream
            victim = sorted(live)[1]
            pool.close(victim)
            del live[victim]
            s = pool.open()
            assert s == victim
            live[s] = _Stream(kw, 100 + sid, ncalls, rng)
            sid += 1
        if refuse_at is not None and call == refuse_at:
            # a call that lists a closed slot beside open ones is refused whole: nothing changes for any slot
            before = {s: (pool.available(s), pool.info(s)["slices"]) for s in live}
            free = next(s for s in range(nslots) if s not in live) if len(live) < nslots else None
            if free is not None:
                blocks = {s: np.zeros((2, 4800), np.float32) for s in live}
                blocks[free] = np.zeros((2, 480), np.float32)
                with pytest.raises(E.PvError, match=f"slot {free}"):
                    pool.feed(blocks)
                assert {s: (pool.available(s), pool.info(s)["slices"]) for s in live} == before
        blocks = {}
        for s, stm in live.items():
            if rng.random() < 0.8:  # some slots sit out some calls
                blocks[s] = stm.next_block()
        pool.feed(blocks)
        for s, blk in blocks.items():
            live[s].ref.processInData(blk)
        for s, stm in live.items():
            got_n, want_n = pool.available(s), stm.ref.getOutSamples()
            assert got_n == want_n, (call, s)
            stm.out.append(pool.retrieve(s, got_n))
            stm.ref_out.append(stm.ref.getOutData(want_n))
            stm.ref.num_res_ = 0
    for s, stm in live.items():
        a, b = np.concatenate(stm.out, axis=1), np.concatenate(stm.ref_out, axis=1)
        assert b.shape[1] > 0
        assert bits_equal(a, b), (s, a.shape, b.shape)
    return pool, live


CASES = {
    "ps4_cm1_2048": dict(semitones=4.0, coremode=1, fftsize=2048),
    "ps12_cm0": dict(semitones=12.0, coremode=0),
    "ps12_cm2": dict(semitones=12.0, coremode=2),
    "stretch1.5_4096": dict(mode="time_stretch", time_ratio=1.5, fftsize=4096),
    "gender-7": dict(mode="gender_change", semitones=-7.0),
    "formant+7": dict(mode="formant_pitchshift", semitones=7.0),
    "robotic": dict(mode="robotic"),
    "ps4_512": dict(semitones=4.0, fftsize=512),
    "ps4_1024": dict(semitones=4.0, fftsize=1024),
}


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


@pytest.mark.parametrize("name", list(CASES))
def test_slots_match_single_stream_engine(name, arith):
    _check_identity(CASES[name])


def test_against_oracle():
    kw = CASES["ps4_cm1_2048"]
    pool = E.StreamPool(2, channels=2, **kw)
    slots = [pool.open(), pool.open()]
    xs = [signals.voice(48000, 2, seed=7), signals.voice(48000, 2, seed=8)]
    orc = [O.Oracle(2, **kw) for _ in slots]
    got, want = [[], []], [[], []]
    for i in range(0, 48000, 480):
        pool.feed({s: xs[j][:, i:i + 480] for j, s in enumerate(slots)})
        for j, s in enumerate(slots):
            orc[j].process(xs[j][:, i:i + 480])
            assert pool.available(s) == orc[j].available()
            got[j].append(pool.retrieve(s, pool.available(s)))
            want[j].append(orc[j].retrieve(orc[j].available()))
    for j in range(2):
        a, b = np.concatenate(got[j], axis=1).astype(np.float64), np.concatenate(want[j], axis=1)
        assert a.shape == b.shape and a.shape[1] > 40000
        assert float(np.sqrt(np.mean((a - b) ** 2))) <= 1e-4


def test_robotic_bit_exact_vs_oracle(arith):
    pool = E.StreamPool(3, channels=2, mode="robotic")
    slots = [pool.open() for _ in range(3)]
    xs = [signals.voice(20000, 2, seed=20 + j) for j in range(3)]
    orc = [O.Oracle(2, mode="robotic") for _ in slots]
    got, want = [[] for _ in slots], [[] for _ in slots]
    for i in range(0, 20000, 480):
        pool.feed({s: xs[j][:, i:i + 480] for j, s in enumerate(slots)})
        for j, s in enumerate(slots):
            orc[j].process(xs[j][:, i:i + 480])
            got[j].append(pool.retrieve(s, pool.available(s)))
            want[j].append(orc[j].retrieve(orc[j].available()))
    for j in range(3):
        assert bits_equal(np.concatenate(got[j], axis=1), np.concatenate(want[j], axis=1))


def test_overrun_drops_like_engine():
    kw = CASES["ps4_cm1_2048"]
    pool = E.StreamPool(2, channels=2, **kw)
    hog, busy = pool.open(), pool.open()
    ref_hog, ref_busy = E.PhaseVocoder(*_cfg_args(kw)), E.PhaseVocoder(*_cfg_args(kw))
    x, y = signals.voice(60000, 2, seed=5), signals.voice(60000, 2, seed=6)
    got, want = [], []
    for i in range(0, 60000, 480):
        pool.feed({hog: x[:, i:i + 480], busy: y[:, i:i + 480]})
        ref_hog.processInData(x[:, i:i + 480])
        ref_busy.processInData(y[:, i:i + 480])
        assert pool.available(hog) == ref_hog.getOutSamples()  # the hog never retrieves
        n = pool.available(busy)
        assert n == ref_busy.getOutSamples()
        assert bits_equal(pool.retrieve(busy, n), ref_busy.getOutData(n))
    info = pool.info(hog)
    assert info["slices"] == ref_hog.info()["slices"]
    n = pool.available(hog)
    assert n > 0 and n == ref_hog.getOutSamples()
    assert bits_equal(pool.retrieve(hog, n), ref_hog.getOutData(n))


def test_refused_call_changes_nothing():
    _check_identity(CASES["ps4_cm1_2048"], ncalls=24, seed=3, reopen=False, refuse_at=12)


def test_bad_slots_and_full_pool():
    pool = E.StreamPool(2, channels=2, semitones=4.0)
    a, b = pool.open(), pool.open()
    assert (a, b) == (0, 1)
    with pytest.raises(E.PvError, match="invalid argument"):
        pool.open()
    blk = np.zeros((2, 480), np.float32)
    L = E.lib()
    for slots in ([5], [-1], [a, a]):
        arr = np.array(slots, np.int32)
        n = np.full(len(slots), 480, np.int32)
        rows = E._pp([blk[c] for _ in slots for c in range(2)])
        assert L.pv_pool_feed(pool.h, len(slots), arr.ctypes.data, rows, n.ctypes.data) == 1
    pool.close(b)
    with pytest.raises(E.PvError, match="invalid argument"):
        pool.feed({b: blk})
    with pytest.raises(E.PvError, match="invalid argument"):
        pool.close(b)
    assert pool.available(b) == -1
    pool.feed({a: blk})
    assert pool.open() == b


def test_scale_128_slots():
    kw = CASES["ps4_cm1_2048"]
    S, calls = 128, 200  # 480-frame calls: 2 s of audio
    pool = E.StreamPool(S, channels=2, **kw)
    xs = [signals.voice(calls * 480, 2, seed=1000 + j) for j in range(S)]
    refs = {}  # sampled slots: their single-stream engines
    outs, want = {}, {}
    pos = {}
    for k in range(calls):
        while len(pos) < S and len(pos) < (k + 1) * S // 20:  # joins staggered over the first 20 calls
            s = pool.open()
            pos[s] = 0
            if s in (0, 37, 90, 127):
                refs[s] = E.PhaseVocoder(*_cfg_args(kw))
                outs[s], want[s] = [], []
        blocks = {s: xs[s][:, p:p + 480] for s, p in pos.items()}
        pool.feed(blocks)
        for s in pos:
            pos[s] += 480
            n = pool.available(s)
            y = pool.retrieve(s, n)
            assert np.isfinite(y).all()
            if s in refs:
                refs[s].processInData(blocks[s])
                assert refs[s].getOutSamples() == n
                outs[s].append(y)
                want[s].append(refs[s].getOutData(n))
    assert sorted(refs) == [0, 37, 90, 127]
    for s in refs:
        assert bits_equal(np.concatenate(outs[s], axis=1), np.concatenate(want[s], axis=1)), s


def test_planner_refusal_names_the_slot_and_changes_nothing():
    # A hop this large for the stretch makes the first slice's shift increment exceed the frame, so the planner refuses
    # a slot as soon as it has the input for a slice.  (In the pool's scope a planner refusal depends only on the
    # configuration and the slot's own slice count.)  `quiet` is listed first: its planner has taken the refused call's
    # block before `loud` is refused, and must be put back -- afterwards it reaches its own refusal at exactly the call
    # a single-stream engine fed the same accepted blocks reaches it.
    kw = dict(mode="time_stretch", time_ratio=2.5, fftsize=2048, hopsize=1024)
    pool = E.StreamPool(2, channels=2, **kw)
    quiet, loud = pool.open(), pool.open()
    ref = E.PhaseVocoder(*_cfg_args(kw))
    blk = signals.voice(100, 2, seed=9)
    pool.feed({quiet: blk})
    ref.processInData(blk)
    before = (pool.available(quiet), pool.info(quiet)["slices"])
    with pytest.raises(E.PvError, match=f"slot {loud}"):
        pool.feed({quiet: blk, loud: np.zeros((2, 8192), np.float32)})
    assert (pool.available(quiet), pool.info(quiet)["slices"]) == before
    assert pool.info(loud)["slices"] == 0
    for call in range(100):
        try:
            ref.processInData(blk)
            ref_ok = True
        except E.PvError:
            ref_ok = False
        try:
            pool.feed({quiet: blk})
            pool_ok = True
        except E.PvError:
            pool_ok = False
        assert pool_ok == ref_ok, call
        if not ref_ok:
            break
        assert pool.available(quiet) == ref.getOutSamples()
    assert not ref_ok
