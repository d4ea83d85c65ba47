"""The stream pool's device-resident feed (include/audiomod_pv.h pv_pool_feed_device; StreamPool.feed_device) on the
GPU.  Every comparison is bit for bit against a TWIN pool of the same configuration and arithmetic setting driven by
feed() + retrieve()-all with the same blocks: a device feed is defined as that pair.

Sizes.  A call's block sizes come from {0, 1, 7, 480, 960}, different per slot and call.  The pool's input ring is
next_pow2(3 * fftsize + 16 * max_hop + 16) frames (pv_engine.cc pool_create): 4096 at fftsize 512 and 16384 at fftsize
2048 for every configuration below (hops of 170 ... 512 frames).  The identity tests feed every slot NCALLS = 30 calls of
at least 16 400 frames in total (asserted), so every slot's ring wraps at least once (four times at fftsize 512)."""
import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals
from tests.test_async_gpu import _late_input, _spin, delay  # noqa: F401 (delay: the fixture that sizes the spin)

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 7, 480, 960)
NCALLS = 30
RING_MAX = 16384
NSLOTS = 3
POISON_F32 = 12345.0
POISON_I16 = 0x5A5A

# name: (pool arguments, per-slot (semitones, time_ratio) or None for a plain pool)
CONFIGS = {
    "fft512_cm1_ps4": (dict(semitones=4.0, coremode=1, fftsize=512), None),
    "fft2048_cm1_ps4": (dict(semitones=4.0, coremode=1, fftsize=2048), None),
    "fft2048_cm0_ps-5": (dict(semitones=-5.0, coremode=0, fftsize=2048), None),
    "stretch1.5_fft2048": (dict(mode="time_stretch", time_ratio=1.5, fftsize=2048), None),
    # no resampler, interpolated table, direct table: three kernel variants per call
    "mixed_0_+4_-7": (dict(semitones=0.0, coremode=1, fftsize=2048, pitch_range=(-7.0, 4.0)),
                      ((0.0, 1.0), (4.0, 1.0), (-7.0, 1.0))),
}
DEFAULT = "fft2048_cm1_ps4"


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


def _call_sizes(seed):
    """[NCALLS][NSLOTS] block sizes from SIZES, every slot's total above the largest ring"""
    rng = np.random.default_rng(seed)
    n = rng.choice(SIZES, size=(NCALLS, NSLOTS), p=(0.05, 0.05, 0.05, 0.15, 0.7))
    for j, v in enumerate(SIZES):  # every size at least once per slot, in different calls
        for s in range(NSLOTS):
            n[(5 * j + 2 * s + 1) % NCALLS, s] = v
    assert (n.sum(axis=0) >= RING_MAX + 16).all(), n.sum(axis=0)
    assert all((n[:, a] != n[:, b]).sum() > NCALLS // 4 for a in range(NSLOTS) for b in range(a))
    return n


def _to_i16(y):
    """the WAV writer's rule (pv_wire.h) in numpy: saturate(x * 32768, -32768, 32767), truncated toward zero"""
    v = np.asarray(y, np.float32) * np.float32(32768.0)
    return np.trunc(np.clip(v, np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)


class Pair:
    """a pool driven through feed_device and its twin driven through feed + retrieve, slot for slot"""

    def __init__(self, name, wire="f32"):
        kw, values = CONFIGS[name]
        self.pool, self.twin = E.StreamPool(NSLOTS, channels=2, **kw), E.StreamPool(NSLOTS, channels=2, **kw)
        self.values = values
        self.i16 = wire == "i16"
        self.slots = [self.open(i) for i in range(NSLOTS)]
        self.pending = []  # (what, device tensor, frames, expected arrays, pitch)

    def open(self, i):
        kw = {} if self.values is None else dict(semitones=self.values[i][0], time_ratio=self.values[i][1])
        s, t = self.pool.open(**kw), self.twin.open(**kw)
        assert s == t
        return s

    def twin_all(self, blocks):
        """the twin's side of a device feed: feed, then retrieve everything; {slot: [2, got] float32}"""
        self.twin.feed({s: (b.astype(np.float32) * np.float32(1.0 / 32768.0) if self.i16 else b) for s, b in blocks.items()})
        return {s: self.twin.retrieve(s, self.twin.available(s)) for s in blocks}

    def device(self, blocks, what="", stream=None, pad_in=3, pad_out=5):
        """one feed_device of {slot: [2, n]} (float32 or int16 as the pair's wire) and the twin's pair of calls; counts
        are checked at once, samples in check()"""
        slots = list(blocks)
        n = np.array([blocks[s].shape[1] for s in slots], np.int32)
        dt = np.int16 if self.i16 else np.float32
        poison = POISON_I16 if self.i16 else POISON_F32
        x = np.full((len(slots), 2, int(n.max()) + pad_in), 1234 if self.i16 else 0.25, dt)  # (past n[i]: never read)
        for i, s in enumerate(slots):
            assert blocks[s].dtype == dt
            x[i, :, :n[i]] = blocks[s]
        plan = self.pool.plan_feed(slots, n)
        out = torch.full((len(slots), 2, int(plan.max()) + pad_out), poison, dtype=torch.int16 if self.i16 else torch.float32,
                         device="cuda")
        d_x = torch.from_numpy(x).cuda()
        got_out, frames = self.pool.feed_device(slots, d_x, n=n, out=out, stream=stream)
        assert got_out is out
        want = self.twin_all(blocks)
        assert [int(v) for v in plan] == [want[s].shape[1] for s in slots], (what, "plan_feed")
        assert [int(v) for v in frames] == [want[s].shape[1] for s in slots], (what, "out_frames")
        assert all(self.pool.available(s) == 0 for s in slots), what
        self.pending.append((what, out, frames, [want[s] for s in slots], d_x))
        return frames

    def check(self):
        torch.cuda.synchronize()
        total = 0
        for what, out, frames, want, _ in self.pending:
            got = out.cpu().numpy()
            for i, w in enumerate(want):
                k = int(frames[i])
                if self.i16:
                    assert np.array_equal(got[i, :, :k], _to_i16(w)), (what, i)
                    assert (got[i, :, k:] == POISON_I16).all(), (what, i, "tail written")
                else:
                    assert np.array_equal(got[i, :, :k].view(np.uint32), w.view(np.uint32)), (what, i)
                    assert (got[i, :, k:] == np.float32(POISON_F32)).all(), (what, i, "tail written")
                total += k
        self.pending = []
        return total

    def close(self):
        torch.cuda.synchronize()
        self.pool.close_pool(), self.twin.close_pool()


def _voice(n, seed, i16=False, gain=1.0):
    x = signals.voice(n, 2, seed=seed) * np.float32(gain)
    if not i16:
        return np.ascontiguousarray(x, np.float32)
    return np.clip(np.rint(x.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def _drive(pair, sizes, gain=1.0):
    """NCALLS device feeds of all slots (several in flight: one synchronisation at the end); returns the frames compared"""
    xs = [_voice(int(sizes[:, j].sum()) + 1, 40 + j, pair.i16, gain) for j in range(NSLOTS)]
    pos = [0] * NSLOTS
    for c in range(len(sizes)):
        blocks = {}
        for j, s in enumerate(pair.slots):
            n = int(sizes[c, j])
            blocks[s] = np.ascontiguousarray(xs[j][:, pos[j]:pos[j] + n])
            pos[j] += n
        pair.device(blocks, what=f"call {c}")
    return pair.check()


# ---- 1. twin identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_twin_identity(name, arith):
    """30 calls of sizes from {0, 1, 7, 480, 960}, at least 16 400 frames per slot (every input ring wraps), an out_pitch
    five above the need with a poisoned tail, an in_pitch three above the largest block"""
    pair = Pair(name)
    try:
        assert _drive(pair, _call_sizes(7)) > 3 * 10000
    finally:
        pair.close()


# ---- 2. int16 wire ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,gain", [(DEFAULT, 0.5), ("mixed_0_+4_-7", 0.5), (DEFAULT, 200.0)],
                         ids=["plain", "mixed", "loud"])
def test_int16_wire(name, gain, arith):
    """int16 in and out against the twin fed the reader's float conversion, its output converted by the writer's rule in
    numpy.  The block sizes and so the counts are no multiples of 4 (1, 7 and what 480 / 960 frames give at +4 st).
    `loud`: the voice 200 times over, clipped to the int16 range on the way in -- a full-scale square-like wave whose
    phase-vocoded output overshoots full scale; that both rails are hit is asserted from the twin's float output."""
    pair = Pair(name, wire="i16")
    try:
        sizes = _call_sizes(8)
        xs = [_voice(int(sizes[:, j].sum()) + 1, 40 + j, True, gain) for j in range(NSLOTS)]
        pos = [0] * NSLOTS
        lo, hi, odd = 0.0, 0.0, 0
        for c in range(NCALLS):
            blocks = {}
            for j, s in enumerate(pair.slots):
                n = int(sizes[c, j])
                blocks[s] = np.ascontiguousarray(xs[j][:, pos[j]:pos[j] + n])
                pos[j] += n
            frames = pair.device(blocks, what=f"call {c}")
            odd += sum(1 for v in frames if v % 4)
            for w in pair.pending[-1][3]:
                if w.size:
                    lo, hi = min(lo, float(w.min())), max(hi, float(w.max()))
        assert odd > 0
        if gain > 1.0:
            assert hi * 32768.0 > 32767.0 and lo * 32768.0 < -32768.0, (lo, hi)
        else:
            assert hi > 0.01 and lo < -0.01, (lo, hi)
        assert pair.check() > 3 * 10000
    finally:
        pair.close()


# ---- 3. order -----------------------------------------------------------------------------------------------------------
PRIME = 4800  # frames that bring every slot past its first slices, so that a 480-frame call returns output
# A call's output trails its input by about 1875 frames at fft 2048, +4 st (the reference on the CPU, fed 4800 + 480 frames
# and then n frames of two different voices: the two outputs are equal for n = 480 and 960, and differ from frame 1872
# on for n = 1920 ... 4800 -- in 510 of 2438 frames for n = 2400).  The order tests therefore feed LATE = 2400 frames per
# call, so that a call's result shows which input it read; each asserts that the two candidate results differ.
LATE = 2400


def _primed(name=DEFAULT, late=False):
    """late: also four device feeds of LATE frames, one through each descriptor block of the ring, so that no call of the
    test itself has to grow a block (growing frees the old buffer, which waits for the device, and so for a spinning
    producer)"""
    pair = Pair(name)
    pair.device({s: _voice(PRIME, 60 + s) for s in pair.slots}, what="prime")
    pair.device({s: _voice(480, 70 + s) for s in pair.slots}, what="prime 2")
    for k in range(4 if late else 0):
        pair.device({s: _voice(LATE, 400 + 10 * k + s) for s in pair.slots}, what=f"prime, block {k}")
    assert pair.check() > 0
    return pair


def _block3(seed, n=480):
    return np.stack([_voice(n, seed + j) for j in range(NSLOTS)])


def _differ(a, b):
    """two lists of per-slot results that differ for every slot"""
    return all(x.shape == y.shape and not np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def _twin_result(pair, x):
    want = pair.twin_all({s: x[i] for i, s in enumerate(pair.slots)})
    return [want[s] for s in pair.slots]


def _matches(snap, frames, want):
    got = snap.cpu().numpy()
    return all(int(frames[i]) == w.shape[1] and np.array_equal(got[i, :, :w.shape[1]].view(np.uint32), w.view(np.uint32))
               for i, w in enumerate(want))


def _late(pair, x_a, x_b, producer, consumer, cycles):
    got = {}

    def run(d_in, stream):
        out, got["frames"] = pair.pool.feed_device(pair.slots, d_in, stream=stream)
        return out

    d_a, d_b = torch.from_numpy(x_a).cuda(), torch.from_numpy(x_b).cuda()
    snap = _late_input(run, d_a, d_b, torch.empty_like(d_a), producer, consumer, cycles)
    return snap, got["frames"]


@pytest.mark.parametrize("null", [False, True], ids=["side_stream", "null_stream"])
def test_late_input(null, delay):
    """feed_device behind a producer that is still spinning (tests/test_async_gpu.py's construction and delay): the call
    returns before its input exists, and the result is the synchronous one of the late input, not of the stale one"""
    pair, other = _primed(late=True), _primed(late=True)
    try:
        s = torch.cuda.default_stream() if null else torch.cuda.Stream()
        x_a, x_b = _block3(80, LATE), _block3(90, LATE)
        snap, frames = _late(pair, x_a, x_b, s, s, delay)
        want_a, want_b = _twin_result(pair, x_a), _twin_result(other, x_b)
        assert _differ(want_a, want_b)
        assert _matches(snap, frames, want_a), "the feed did not wait for its input"
    finally:
        pair.close(), other.close()


def test_negative_control_a_feed_that_does_not_wait_is_seen(delay):
    """the same call on a stream that does not wait for the producer reads the stale (valid) input and must NOT give
    x_a's result: the delay makes a broken order observable"""
    pair, other = _primed(late=True), _primed(late=True)
    try:
        x_a, x_b = _block3(80, LATE), _block3(90, LATE)
        snap, frames = _late(pair, x_a, x_b, torch.cuda.Stream(), torch.cuda.Stream(), delay)
        want_a, want_b = _twin_result(other, x_a), _twin_result(pair, x_b)
        assert _differ(want_a, want_b)
        assert not _matches(snap, frames, want_a)
        assert _matches(snap, frames, want_b)  # what it read was the stale block, whole
    finally:
        pair.close(), other.close()


def test_eight_calls_behind_one_spin(delay):
    """more calls than the descriptor ring is deep behind one spin: the later ones wait on the host for the oldest block
    (bounded by the spin), and all eight equal the twin's.  Every call's input is produced behind the spin too, over a
    stale block whose result differs."""
    pair, other = _primed(late=True), _primed(late=True)
    try:
        s = torch.cuda.Stream()
        xs = [_block3(100 + 10 * k, LATE) for k in range(8)]
        stale = _block3(300, LATE)
        src = [torch.from_numpy(x).cuda() for x in xs]
        ds = [torch.from_numpy(stale).cuda() for _ in xs]
        torch.cuda.synchronize()
        ev = torch.cuda.Event()
        res = []
        with torch.cuda.stream(s):
            _spin(delay)
            ev.record(s)
            for k, d in enumerate(ds):
                d.copy_(src[k], non_blocking=True)
                res.append(pair.pool.feed_device(pair.slots, d, stream=s))
                if k == 0:
                    pending = not ev.query()
        s.synchronize()
        assert pending, "the spin had finished when the first call returned"
        # (that calls 4 to 7 waited for their descriptor blocks is not observed directly: a call that had written a busy
        # block would have replaced descriptors that queued launches still read, and the results below would differ)
        for k, (out, frames) in enumerate(res):
            want = _twin_result(pair, xs[k])
            if k == 0:
                assert _differ(want, _twin_result(other, stale))
            assert _matches(out, frames, want), f"call {k}"
    finally:
        pair.close(), other.close()


# ---- 4. interleaving ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [DEFAULT, "mixed_0_+4_-7"])
def test_interleaved_with_the_synchronous_calls(name):
    """device feeds, feed + partial retrieve, close and open with device feeds in flight, device feeds of everything"""
    pair = _primed(name)
    pool, twin = pair.pool, pair.twin
    s0, s1, s2 = pair.slots
    try:
        pair.device({s0: _voice(480, 200)}, what="device feed, slot 0")
        blk = _voice(960, 201)
        pool.feed({s1: blk}), twin.feed({s1: blk})
        assert pool.available(s1) == twin.available(s1) > 100
        assert np.array_equal(pool.retrieve(s1, 100).view(np.uint32), twin.retrieve(s1, 100).view(np.uint32))
        assert pool.available(s1) == twin.available(s1) > 0
        pair.device({s2: _voice(7, 202)}, what="device feed, slot 2")
        for k in range(3):  # in flight while slot 1 closes and reopens
            pair.device({s0: _voice(960, 210 + k), s2: _voice(480, 220 + k)}, what=f"in flight {k}")
        pool.close(s1), twin.close(s1)
        assert pair.open(1) == s1
        assert pool.available(s1) == 0
        for k in range(3):  # the reopened slot is a fresh stream: the twin's is
            pair.device({s: _voice(PRIME if s == s1 and k == 0 else 480, 230 + 10 * k + s) for s in pair.slots},
                        what=f"all slots {k}")
        # ... and the synchronous path behind device feeds in flight
        blocks = {s: _voice(480, 260 + s) for s in pair.slots}
        pool.feed(blocks), twin.feed(blocks)
        for s in pair.slots:
            n = twin.available(s)
            assert pool.available(s) == n > 0
            assert np.array_equal(pool.retrieve(s, n).view(np.uint32), twin.retrieve(s, n).view(np.uint32)), s
        pair.device({s: _voice(480, 270 + s) for s in pair.slots}, what="after the FIFOs are empty")
        assert pair.check() > 0
    finally:
        pair.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_are_transactional():
    pair = _primed()
    pool, twin = pair.pool, pair.twin
    slots = pair.slots
    L = pool.L

    def state():
        return [(pool.available(s), pool.info(s)["slices"], [int(v) for v in pool.plan_feed([s] * 3, [0, 480, 960])])
                for s in slots]

    def valid(what):
        pair.device({s: _voice(480, 300 + s) for s in slots}, what=what)
        assert pair.check() > 0

    def refused(what, *args, **kw):
        before = state()
        with pytest.raises(E.PvError, match="invalid argument"):
            pool.feed_device(*args, **kw)
        assert state() == before, what
        valid(what)

    try:
        x = torch.from_numpy(_block3(310)).cuda()
        plan = pool.plan_feed(slots, [480] * 3)
        assert plan.min() > 1
        # out_pitch one below the planned count (of the slot that needs the most)
        short = torch.zeros((3, 2, int(plan.max()) - 1), device="cuda")
        refused("out_pitch", slots, x, out=short)
        # a slot with pending host output
        blk = _voice(960, 320)
        pool.feed({slots[1]: blk}), twin.feed({slots[1]: blk})
        before = state()
        with pytest.raises(E.PvError, match=f"slot {slots[1]}"):
            pool.feed_device(slots, x)
        assert state() == before
        n = twin.available(slots[1])
        assert pool.available(slots[1]) == n > 0
        assert np.array_equal(pool.retrieve(slots[1], n).view(np.uint32), twin.retrieve(slots[1], n).view(np.uint32))
        valid("pending host output")
        # wire 7
        before = state()
        sl, nn = np.array(slots, np.int32), np.full(3, 480, np.int32)
        out, frames = torch.zeros((3, 2, 2048), device="cuda"), np.zeros(3, np.int32)
        st = L.pv_pool_feed_device(pool.h, 3, sl.ctypes.data, nn.ctypes.data, x.data_ptr(), 480, out.data_ptr(), 2048, 7,
                                   frames.ctypes.data, None)
        assert st == 1 and b"wire" in L.pv_last_error()
        assert state() == before
        valid("wire 7")
        # a duplicate slot
        before = state()
        with pytest.raises(E.PvError, match=f"slot {slots[0]} is listed twice"):
            pool.feed_device([slots[0], slots[0]], x[:2].contiguous())
        assert state() == before
        valid("duplicate slot")
        # n[i] > in_pitch
        refused("n above in_pitch", slots, x, n=[480, 481, 480])
    finally:
        pair.close()
