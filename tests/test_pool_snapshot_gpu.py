"""Stream-pool snapshots on the GPU (include/audiomod_pv.h pv_pool_save / pv_pool_restore; StreamPool.save / restore /
fork): a slot saved to a blob and restored elsewhere continues bit for bit as an uninterrupted single-stream engine
(PhaseVocoder / pv_engine) does -- every available value and every sample -- and a blob is a function of the stream's
history alone.

Shapes.  FFT size 512 unless a case is about another size; 16 calls (10 at fftsize 4096) of 200 ... 900 frames with the
sizes 0, 1, 13 and 479 mixed in, one call of 4097 frames (many slices in one call, and at the small sizes the reference's
overrun path), and a first call of two frames plus 37 so that output flows from the start.  One call's output is left
in the slot until after the next call, so that one save point has output pending.  The schedule is the same for every
save point: one engine run per configuration is the yardstick of all of them."""
import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals
from tests.helpers import bits_equal

pytestmark = pytest.mark.gpu

CASES = {
    "ps4_cm1": dict(semitones=4.0, coremode=1, fftsize=512),              # rotation chain state, resampler ring
    "ps12_cm0": dict(semitones=12.0, coremode=0, fftsize=512),            # st_pp, st_po
    "ps12_cm2": dict(semitones=12.0, coremode=2, fftsize=512),
    "stretch1.5_1024": dict(mode="time_stretch", time_ratio=1.5, fftsize=1024),  # output straight from the accumulator
    "gender-7": dict(mode="gender_change", semitones=-7.0, fftsize=512),  # frequency compensation
    "robotic": dict(mode="robotic", fftsize=512),                         # fixed hop, no phase stage
    "ps4_4096": dict(semitones=4.0, fftsize=4096),                        # two-wave analysis
}


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


def _engine(kw):
    cfg = E.make_config(2, **kw)
    return E.PhaseVocoder(cfg.sample_rate, 2, cfg.time_ratio, cfg.pitch_semitones, cfg.mode, cfg.coremode, cfg.fftsize,
                          cfg.hopsize)


class Schedule:
    """call sizes, the call whose output stays pending, and the save points (a save point k: after k calls)"""

    def __init__(self, fft, ncalls=16, seed=5):
        rng = np.random.default_rng(seed)
        n = [int(v) for v in rng.integers(200, 900, ncalls)]
        n[0] = 2 * fft + 37
        n[2] = 0
        n[4] = fft // 2 + 11  # at least one slice: its output is the pending one
        n[5], n[6] = 13, 1
        big = 9 if ncalls >= 16 else 7
        n[big], n[big + 1] = 4097, 479
        self.sizes, self.hold = n, 4
        self.points = {"after_open": 0, "after_zero_call": 3, "output_pending": 5, "after_4097": big + 1}


class Yardstick:
    """an uninterrupted engine over a schedule: per call the available count and what is retrieved"""

    def __init__(self, kw, x, sch, hold=True):
        ref = _engine(kw)
        self.avail, self.out = [], []
        pos = 0
        for i, n in enumerate(sch.sizes):
            ref.processInData(x[:, pos:pos + n])
            pos += n
            a = ref.L.pv_available(ref.h)
            self.avail.append(a)
            self.out.append(np.zeros((2, 0), np.float32) if (hold and i == sch.hold) else ref.getOutData(a))
        ref.close()


def _step(pool, slot, x, sch, i, yard, hold=True):
    """call i of the schedule on a pool's slot: feed, compare available, retrieve as the yardstick did"""
    pos = sum(sch.sizes[:i])
    pool.feed({slot: x[:, pos:pos + sch.sizes[i]]})
    assert pool.available(slot) == yard.avail[i], ("available", i)
    return np.zeros((2, 0), np.float32) if (hold and i == sch.hold) else pool.retrieve(slot, yard.avail[i])


def _cat(parts):
    return np.concatenate(parts, axis=1)


# 1. continuation equals the engine
@pytest.mark.parametrize("name", list(CASES))
def test_restored_slot_continues_like_the_engine(name, arith):
    kw = CASES[name]
    fft = kw.get("fftsize", 2048)
    sch = Schedule(fft, ncalls=10 if fft == 4096 else 16)
    ncalls = len(sch.sizes)
    x = signals.voice(sum(sch.sizes) + 1, 2, seed=31)
    y = signals.voice(sum(sch.sizes) + 1, 2, seed=32)
    yard_x = Yardstick(kw, x, sch)
    yard_y = Yardstick(kw, y, sch, hold=False)
    want = _cat(yard_x.out)
    assert want.shape[1] > 0
    # pool A: the stream in slot 0, saved at every save point and carried on to the end
    A = E.StreamPool(3, channels=2, **kw)
    src = A.open()
    blobs, got_a = {}, []
    for i in range(ncalls + 1):
        for label, k in sch.points.items():
            if k == i:
                blobs[label] = A.save(src)
                assert A.snapshot_bytes(src) == len(blobs[label])
                assert A.last_launches() == 1
        if i < ncalls:
            got_a.append(_step(A, src, x, sch, i, yard_x))
    assert bits_equal(_cat(got_a), want), "the source slot after its saves"
    info = E.blob_info(blobs["output_pending"])
    assert info["pending_frames"] == yard_x.avail[sch.hold] > 0
    assert info["slices"] > 0 and E.blob_info(blobs["after_open"])["slices"] == 0
    for label, k in sch.points.items():
        # pool B: another live slot first, fed in the same calls as the restored one from then on
        B = E.StreamPool(5, channels=2, **kw)
        other = B.open()
        got_y = [_step(B, other, y, sch, 0, yard_y, hold=False)]
        slot = B.restore(blobs[label])
        assert slot == 1 and B.last_launches() == 1
        assert B.available(slot) == (yard_x.avail[k - 1] if k == sch.hold + 1 else 0), label
        got_b = []
        for i in range(k, ncalls):
            j = 1 + i - k
            pos_x, pos_y = sum(sch.sizes[:i]), sum(sch.sizes[:j])
            blocks = {slot: x[:, pos_x:pos_x + sch.sizes[i]]}
            if j < ncalls:
                blocks[other] = y[:, pos_y:pos_y + sch.sizes[j]]
            B.feed(blocks)
            assert B.available(slot) == yard_x.avail[i], (label, "available", i)
            got_b.append(np.zeros((2, 0), np.float32) if i == sch.hold else B.retrieve(slot, yard_x.avail[i]))
            if j < ncalls:
                assert B.available(other) == yard_y.avail[j], (label, "other available", j)
                got_y.append(B.retrieve(other, yard_y.avail[j]))
        assert bits_equal(_cat(got_a[:k] + got_b), want), label
        assert bits_equal(_cat(got_y), _cat(yard_y.out[:len(got_y)])), (label, "the destination's other slot")
        assert B.info(slot)["slices"] == A.info(src)["slices"], label
        B.close_pool()
    A.close_pool()


# 2. fork
def test_fork_into_the_same_pool(arith):
    kw = CASES["ps4_cm1"]
    sch = Schedule(512)
    x = signals.voice(sum(sch.sizes) + 1, 2, seed=41)
    yard = Yardstick(kw, x, sch)
    pool = E.StreamPool(3, channels=2, **kw)
    src = pool.open()
    k = 6
    head = [_step(pool, src, x, sch, i, yard) for i in range(k)]
    copy = pool.fork(src)
    assert copy == 1 and pool.available(copy) == pool.available(src)
    a, b = [], []
    for i in range(k, len(sch.sizes)):
        pos = sum(sch.sizes[:i])
        blk = x[:, pos:pos + sch.sizes[i]]
        pool.feed({src: blk, copy: blk})
        assert pool.available(src) == pool.available(copy) == yard.avail[i]
        a.append(pool.retrieve(src, yard.avail[i]))
        b.append(pool.retrieve(copy, yard.avail[i]))
    assert bits_equal(_cat(a), _cat(b))
    assert bits_equal(_cat(head + a), _cat(yard.out)) and bits_equal(_cat(head + b), _cat(yard.out))


# 3. mixed pool
def _state(pool):
    return [(s, pool.available(s), pool.info(s)["slices"]) for s in range(pool.capacity) if pool.available(s) >= 0]


def test_mixed_pool_slot_moves_and_incompatible_pools_refuse():
    base = dict(semitones=0.0, time_ratio=1.0, coremode=1, fftsize=512)
    ranges = dict(pitch_range=(-5.0, 7.0), ratio_range=(0.8, 1.5))
    own = dict(semitones=-3.5, time_ratio=1.2)
    sch = Schedule(512)
    x = signals.voice(sum(sch.sizes) + 1, 2, seed=51)
    yard = Yardstick(dict(base, **own), x, sch)
    A = E.StreamPool(3, channels=2, **base, **ranges)
    A.open()  # (cfg's own values: the moved slot is not slot 0 here)
    src = A.open(**own)
    k = 7
    head = [_step(A, src, x, sch, i, yard) for i in range(k)]
    blob = A.save(src)
    info = E.blob_info(blob)
    assert (info["pitch_semitones"], info["time_ratio"]) == (-3.5, np.float32(1.2))
    assert info["arithmetic"] == E.get_arithmetic() and info["cfg"]["fftsize"] == 512
    B = E.StreamPool(2, channels=2, **base, **ranges)
    slot = B.restore(blob)
    assert slot == 0
    tail = [_step(B, slot, x, sch, i, yard) for i in range(k, len(sch.sizes))]
    assert bits_equal(_cat(head + tail), _cat(yard.out))
    # pools that cannot host it: each has a live slot, which a refusal must leave alone
    other = E.ARITH_EXACT if E.get_arithmetic() == E.ARITH_FAST else E.ARITH_FAST
    prev = E.set_arithmetic(other)
    try:
        wrong_arith = E.StreamPool(2, channels=2, **base, **ranges)
    finally:
        E.set_arithmetic(prev)
    bad = {
        "uniform pool of the base configuration": E.StreamPool(2, channels=2, **base),
        "range without the values": E.StreamPool(2, channels=2, **base, pitch_range=(-2.0, 7.0), ratio_range=(0.8, 1.5)),
        "another FFT size": E.StreamPool(2, channels=2, **dict(base, fftsize=1024), **ranges),
        "the other arithmetic setting": wrong_arith,
    }
    blk = signals.voice(1500, 2, seed=52)
    for what, pool in bad.items():
        s = pool.open()
        pool.feed({s: blk})
        before = _state(pool)
        assert len(before) == 1 and before[0][2] > 0
        with pytest.raises(E.PvError, match="invalid argument"):
            pool.restore(blob)
        assert _state(pool) == before, what
        pool.close_pool()


# 4. device feed
@pytest.mark.parametrize("wire", ["f32", "i16"])
def test_save_with_device_feeds_in_flight(wire):
    kw = CASES["ps4_cm1"]
    dt = np.int16 if wire == "i16" else np.float32
    sizes = [1061, 480, 0, 777, 13, 480, 900, 1, 4097, 479, 640, 333]
    k = 6
    x = signals.voice(sum(sizes) + 1, 2, seed=61)
    if wire == "i16":
        x = np.trunc(np.clip(x * 32768.0, -32768, 32767)).astype(np.int16)
    A, B, twin = (E.StreamPool(n, channels=2, **kw) for n in (3, 5, 2))
    src, ref = A.open(), twin.open()
    B.open()
    want, pending = [], []
    pos = 0
    pool, slot = A, src
    for i, n in enumerate(sizes):
        if i == k:  # device feeds of A are in flight: no synchronisation here
            blob = A.save(src)
            slot = B.restore(blob)
            assert slot == 1
            pool = B
        blk = np.ascontiguousarray(x[:, pos:pos + n])
        pos += n
        twin.feed({ref: blk.astype(np.float32) * np.float32(1.0 / 32768.0) if wire == "i16" else blk})
        want.append(twin.retrieve(ref, twin.available(ref)))
        buf = np.zeros((1, 2, max(n, 1)), dt)
        buf[0, :, :n] = blk
        d_x = torch.from_numpy(buf).cuda()
        out, frames = pool.feed_device([slot], d_x, n=np.array([n], np.int32))
        assert int(frames[0]) == want[-1].shape[1], i
        pending.append((out, int(frames[0]), d_x))
    torch.cuda.synchronize()
    total = 0
    for i, (out, f, _) in enumerate(pending):
        got = out.cpu().numpy()[0, :, :f]
        if wire == "i16":
            w = np.trunc(np.clip(want[i] * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)
            assert np.array_equal(got, w), i
        else:
            assert bits_equal(got, want[i]), i
        total += f if i >= k else 0
    assert total > 1000  # the destination delivered audio of its own


# 5. tenant independence and size
@pytest.mark.parametrize("name", ["ps4_cm1", "ps12_cm0"])
def test_blobs_depend_on_the_history_alone(name):
    kw = CASES[name]
    sch = Schedule(512)
    sch.sizes[:3] = [200, 250, 300]  # about five slices: the 17-slot plane rings have not wrapped at the first save
    x = signals.voice(sum(sch.sizes) + 1, 2, seed=71)
    fresh = E.StreamPool(2, channels=2, **kw)
    used = E.StreamPool(5, channels=2, **kw)
    a = fresh.open()
    used.open(), used.open(), used.open()
    noise = signals.voice(9000, 2, seed=72)
    for i in range(0, 9000, 3000):  # an unrelated stream fills every ring of slot 1 and leaves
        used.feed({1: noise[:, i:i + 3000], 2: noise[:, i:i + 500]})
        used.retrieve(1, used.available(1)), used.retrieve(2, used.available(2))
    used.close(1)
    b = used.open()
    assert (a, b) == (0, 1)
    pos = 0
    for i, n in enumerate(sch.sizes[:12]):
        blk = x[:, pos:pos + n]
        pos += n
        fresh.feed({a: blk})
        used.feed({b: blk, 2: noise[:, :n]})
        used.retrieve(2, used.available(2))
        if i != sch.hold:
            ya, yb = fresh.retrieve(a, fresh.available(a)), used.retrieve(b, used.available(b))
            assert bits_equal(ya, yb)
        if i + 1 in (3, 12):
            ba, bb = fresh.save(a), used.save(b)
            assert len(ba) == fresh.snapshot_bytes(a) == used.snapshot_bytes(b) == len(bb)
            if ba != bb:
                da, db = np.frombuffer(ba, np.uint8), np.frombuffer(bb, np.uint8)
                where = np.flatnonzero(da != db)
                raise AssertionError(f"after {i + 1} calls the blobs differ in {where.size} bytes, first at {where[0]}, last at {where[-1]}")
            assert fresh.save(a) == ba, "two saves with no feed between them"


# 6. many at once and refusals
def test_many_slots_at_once_and_refusals():
    kw = CASES["ps4_cm1"]
    A = E.StreamPool(4, channels=2, **kw)
    slots = [A.open() for _ in range(3)]
    xs = [signals.voice(6000, 2, seed=80 + j) for j in range(3)]
    refs = [_engine(kw) for _ in slots]
    for i in range(0, 3000, 750):
        A.feed({s: xs[j][:, i:i + 750] for j, s in enumerate(slots)})
        for j, s in enumerate(slots):
            refs[j].processInData(xs[j][:, i:i + 750])
            A.retrieve(s, A.available(s))
            refs[j].getOutData(refs[j].L.pv_available(refs[j].h))
    blobs = A.save(slots)
    assert A.last_launches() == 1 and len(blobs) == 3 and len(set(blobs)) == 3
    # two free slots: refused, nothing half-opened
    tight = E.StreamPool(3, channels=2, **kw)
    t0 = tight.open()
    tight.feed({t0: xs[0][:, :900]})
    before = _state(tight)
    with pytest.raises(E.PvError, match="free slots"):
        tight.restore(blobs)
    assert _state(tight) == before and tight.available(1) == tight.available(2) == -1
    # exactly three free slots
    B = E.StreamPool(4, channels=2, **kw)
    b0 = B.open()
    new = B.restore(blobs)
    assert new == [1, 2, 3] and B.last_launches() == 1
    got, want = [[] for _ in new], [[] for _ in new]
    for i in range(3000, 6000, 750):
        B.feed({s: xs[j][:, i:i + 750] for j, s in enumerate(new)})
        for j, s in enumerate(new):
            refs[j].processInData(xs[j][:, i:i + 750])
            n = refs[j].L.pv_available(refs[j].h)
            assert B.available(s) == n
            got[j].append(B.retrieve(s, n))
            want[j].append(refs[j].getOutData(n))
    for j in range(3):
        assert _cat(want[j]).shape[1] > 0 and bits_equal(_cat(got[j]), _cat(want[j])), j
    # damaged blobs: refused, and nothing is fed into the pool on their account
    blob = blobs[0]
    free = E.StreamPool(2, channels=2, **kw)
    damaged = [blob[:n] for n in (0, 7, 100, 224, len(blob) // 2, len(blob) - 8, len(blob) - 1)]
    for at in (9, 30, 70, 150, len(blob) - 4000, len(blob) - 3):  # header fields, the payload, the checksum
        m = bytearray(blob)
        m[at] ^= 0x10
        damaged.append(bytes(m))
    for d in damaged:
        with pytest.raises(E.PvError, match="invalid argument"):
            free.restore(d)
        with pytest.raises(E.PvError):
            E.blob_info(d)
        assert _state(free) == []
    # refusals of save: a bad slot, a slot twice, a blob too small -- nothing is written
    L = E.lib()
    import ctypes as C
    buf = np.full(len(blob), 0xAB, np.uint8)
    ptrs = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data)
    got = np.full(2, -7, np.int64)
    for sl, cap in (([9], [len(blob)]), ([b0, b0], [len(blob)] * 2), ([b0], [len(blob) // 2]), ([-1], [len(blob)])):
        arr, caps = np.array(sl, np.int32), np.array(cap, np.int64)
        assert L.pv_pool_save(B.h, len(sl), arr.ctypes.data, ptrs, caps.ctypes.data, got.ctypes.data) == 1
        assert (buf == 0xAB).all() and (got == -7).all()
    assert L.pv_pool_save(B.h, 1, np.array([b0], np.int32).ctypes.data, None, None, None) == 1
