"""Mixed stream pool on the GPU: slots of one pool at different pitches / time ratios, each bit for bit like a
single-stream engine (PhaseVocoder / pv_engine) created with that slot's own values and fed the same blocks."""
import math

import numpy as np
import pytest

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import bits_equal

pytestmark = pytest.mark.gpu

SPECIAL = (0, 1, 4097)
PITCHES = (-12.0, -7.0, -0.5, 0.0, 3.7, 4.0, 12.0)


def _cfg_args(kw, semitones, time_ratio):
    cfg = E.make_config(2, **kw)
    return (cfg.sample_rate, 2, float(time_ratio), float(semitones), cfg.mode, cfg.coremode, cfg.fftsize, cfg.hopsize)


def _sizes(rng, ncalls):
    n = [int(v) for v in rng.integers(200, 900, ncalls)]
    for j, v in enumerate(rng.permutation(SPECIAL)):
        n[(3 * j + 1) % ncalls] = int(v)
    return n


class _Stream:
    def __init__(self, kw, st, tr, seed, ncalls, rng):
        self.sizes = _sizes(rng, ncalls)
        self.x = signals.voice(sum(self.sizes) + 1, 2, seed=seed)
        self.pos = self.k = 0
        self.ref = E.PhaseVocoder(*_cfg_args(kw, st, tr))
        self.out, self.ref_out = [], []

    def next_block(self):
        n = self.sizes[self.k % len(self.sizes)]
        self.k += 1
        blk = self.x[:, self.pos:self.pos + n]
        if blk.shape[1] < n:
            blk = np.zeros((2, n), np.float32)
        self.pos += n
        return np.ascontiguousarray(blk)


def _check_mixed(kw, values, pitch_range=(-12, 12), ratio_range=None, ncalls=30, seed=11):
    """values: (semitones, time_ratio) of each stream in joining order; the last one is the stream that takes over a
    closed slot halfway through."""
    rng = np.random.default_rng(seed)
    pool = E.StreamPool(len(values), channels=2, pitch_range=pitch_range, ratio_range=ratio_range, **kw)
    live = {}
    todo = list(values[:-1])
    for call in range(ncalls):
        if call % 2 == 0 and todo:  # staggered joins
            st, tr = todo.pop(0)
            s = pool.open(semitones=st, time_ratio=tr)
            live[s] = _Stream(kw, st, tr, 100 + len(live), ncalls, rng)
            info = pool.info(s)
            want = live[s].ref.info()
            for k in ("hop_in", "pitch_scale", "hs_ratio", "resample", "res_num", "res_den", "res_filt_len", "res_interp"):
                assert info[k] == want[k], (k, st, tr)
        if call == ncalls // 2:  # a slot closes and comes back as a fresh stream at another value
            victim = sorted(live)[1]
            pool.close(victim)
            del live[victim]
            st, tr = values[-1]
            s = pool.open(semitones=st, time_ratio=tr)
            assert s == victim
            live[s] = _Stream(kw, st, tr, 200, ncalls, rng)
        blocks = {s: stm.next_block() for s, stm in live.items() if rng.random() < 0.8}
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
    return pool


def _pitches(last=-3.0):
    return [(p, 1.0) for p in PITCHES] + [(last, 1.0)]


CASES = {
    "cm1_2048": (dict(semitones=4.0, coremode=1, fftsize=2048), _pitches()),
    "cm0_2048": (dict(semitones=4.0, coremode=0, fftsize=2048), _pitches()),
    "cm2_2048": (dict(semitones=4.0, coremode=2, fftsize=2048), _pitches()),
    "fft512": (dict(semitones=4.0, fftsize=512), _pitches()),
    "fft1024": (dict(semitones=4.0, fftsize=1024), _pitches()),
    "fft4096": (dict(semitones=4.0, fftsize=4096), _pitches()),
    "gender": (dict(mode="gender_change", semitones=0.0), _pitches(5.0)),
    "formant": (dict(mode="formant_pitchshift", semitones=0.0), _pitches(-5.0)),
    "robotic": (dict(mode="robotic", semitones=0.0), _pitches()),
}


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


@pytest.mark.parametrize("name", list(CASES))
def test_slots_at_different_pitches_match_their_engines(name, arith):
    kw, values = CASES[name]
    _check_mixed(kw, values)


def test_time_ratios_match_their_engines(arith):
    kw = dict(mode="time_stretch", time_ratio=1.0, fftsize=4096)
    values = [(0.0, r) for r in (0.8, 1.0, 1.5, 2.0)] + [(0.0, 1.25)]
    _check_mixed(kw, values, pitch_range=None, ratio_range=(0.8, 2.0))


def test_against_oracle():
    kw = dict(semitones=4.0, coremode=1, fftsize=2048)
    pool = E.StreamPool(2, channels=2, pitch_range=(-12, 12), **kw)
    pitch = (-7.0, 3.7)
    slots = [pool.open(semitones=p) for p in pitch]
    xs = [signals.voice(48000, 2, seed=7), signals.voice(48000, 2, seed=8)]
    orc = [O.Oracle(2, **dict(kw, semitones=p)) for p in pitch]
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
        assert a.shape == b.shape and a.shape[1] > 30000
        assert float(np.sqrt(np.mean((a - b) ** 2))) <= 1e-4


def test_overrun_drops_per_slot():
    kw = dict(semitones=4.0, coremode=1, fftsize=2048)
    pool = E.StreamPool(3, channels=2, pitch_range=(-12, 12), **kw)
    vals = (12.0, -12.0, 3.7)  # two hogs that never retrieve, one busy slot
    slots = [pool.open(semitones=v) for v in vals]
    refs = [E.PhaseVocoder(*_cfg_args(kw, v, 1.0)) for v in vals]
    xs = [signals.voice(60000, 2, seed=5 + j) for j in range(3)]
    for i in range(0, 60000, 480):
        pool.feed({s: xs[j][:, i:i + 480] for j, s in enumerate(slots)})
        for j, s in enumerate(slots):
            refs[j].processInData(xs[j][:, i:i + 480])
            assert pool.available(s) == refs[j].getOutSamples(), (i, j)
        n = pool.available(slots[2])
        assert bits_equal(pool.retrieve(slots[2], n), refs[2].getOutData(n))
    for j in range(2):
        assert pool.info(slots[j])["slices"] == refs[j].info()["slices"]
        n = pool.available(slots[j])
        assert n > 0
        assert bits_equal(pool.retrieve(slots[j], n), refs[j].getOutData(n))


def test_reopen_at_another_pitch_is_a_fresh_stream():
    kw = dict(semitones=4.0, coremode=1, fftsize=2048)
    pool = E.StreamPool(2, channels=2, pitch_range=(-12, 12), **kw)
    x = signals.voice(24000, 2, seed=3)
    s = pool.open(semitones=-7.0)
    for i in range(0, 12000, 480):
        pool.feed({s: x[:, i:i + 480]})
    pool.close(s)
    assert pool.open(semitones=5.5) == s
    ref = E.PhaseVocoder(*_cfg_args(kw, 5.5, 1.0))
    assert pool.info(s)["slices"] == 0 and pool.info(s)["pitch_scale"] == ref.info()["pitch_scale"]
    got, want = [], []
    for i in range(0, 24000, 480):
        pool.feed({s: x[:, i:i + 480]})
        ref.processInData(x[:, i:i + 480])
        assert pool.available(s) == ref.getOutSamples()
        got.append(pool.retrieve(s, pool.available(s)))
        want.append(ref.getOutData(ref.getOutSamples()))
    assert bits_equal(np.concatenate(got, axis=1), np.concatenate(want, axis=1))


def test_open_with_sweeps_the_range_and_refuses_outside():
    kw = dict(semitones=0.0, coremode=1, fftsize=2048)
    pool = E.StreamPool(2, channels=2, pitch_range=(-12, 12), **kw)
    keep = pool.open(semitones=4.0)
    pool.feed({keep: signals.voice(4800, 2, seed=1)})
    before = (pool.available(keep), pool.info(keep))
    for v in np.arange(-12.0, 12.0 + 1e-9, 0.5):
        s = pool.open(semitones=float(v))
        assert s == 1
        assert pool.info(s)["pitch_scale"] == E.PhaseVocoder(*_cfg_args(kw, float(v), 1.0)).info()["pitch_scale"]
        pool.close(s)
    for st, tr in ((-12.5, 1.0), (12.01, 1.0), (math.nan, 1.0), (4.0, 1.1), (4.0, math.nan)):
        with pytest.raises(E.PvError, match="invalid argument"):
            pool.open(semitones=st, time_ratio=tr)
        assert (pool.available(keep), pool.info(keep)) == before
        assert pool.available(1) == -1
    assert pool.open() == 1  # cfg's own value
    # a uniform pool takes only its configuration's values
    uni = E.StreamPool(2, channels=2, **dict(kw, semitones=4.0))
    with pytest.raises(E.PvError, match="invalid argument"):
        uni.open(semitones=3.0)
    assert uni.open(semitones=4.0) == 0


def test_128_distinct_pitches_match_and_launch_like_one():
    kw = dict(semitones=4.0, coremode=1, fftsize=2048)
    S, calls = 128, 60
    pitches = [float(np.float32(v)) for v in np.linspace(-11.9, 11.9, S)]
    mixed = E.StreamPool(S, channels=2, pitch_range=(-12, 12), **kw)
    same = E.StreamPool(S, channels=2, pitch_range=(-12, 12), **kw)
    xs = [signals.voice(calls * 480, 2, seed=2000 + j) for j in range(S)]
    ms = [mixed.open(semitones=p) for p in pitches]
    us = [same.open(semitones=4.0) for _ in range(S)]
    assert all(mixed.info(s)["res_interp"] == 1 for s in ms) and same.info(us[0])["res_interp"] == 1
    sample = (0, 37, 64, 90, 127)
    refs = {j: E.PhaseVocoder(*_cfg_args(kw, pitches[j], 1.0)) for j in sample}
    got, want = {j: [] for j in sample}, {j: [] for j in sample}
    lm, lu = [], []
    for k in range(calls):
        blocks = {ms[j]: xs[j][:, 480 * k:480 * (k + 1)] for j in range(S)}
        mixed.feed(blocks)
        lm.append(mixed.last_launches())
        same.feed({us[j]: xs[j][:, 480 * k:480 * (k + 1)] for j in range(S)})
        lu.append(same.last_launches())
        for j in range(S):
            n = mixed.available(ms[j])
            y = mixed.retrieve(ms[j], n)
            same.retrieve(us[j], same.available(us[j]))
            if j in refs:
                refs[j].processInData(blocks[ms[j]])
                assert refs[j].getOutSamples() == n
                got[j].append(y)
                want[j].append(refs[j].getOutData(n))
    for j in sample:
        assert bits_equal(np.concatenate(got[j], axis=1), np.concatenate(want[j], axis=1)), j
    # one variant class either way: the same launches per feed, however many pitches
    assert max(lm[10:]) == max(lu[10:]) and 0 < max(lm[10:]) <= 8, (lm, lu)
