"""The carrier setting on the GPU (include/audiomod_pv.h "Carrier setting"): a slot of a ROBOTIC pool or mixed pool that
is given carrier ROSENBERG or CHORD must be, bit for bit, the single-stream engine of mode vocoder / vocoder_chord with
the slot's own pitch and time ratio -- every available value, count and sample, the planner's slice dropping, the device
feed on both wires, snapshots -- whatever its robotic and whisper neighbours do; with the setting untouched a pool
launches what it always launched.  The carrier comes from the device generator (pv_carrier_kernel), which is checked on
its own first against the closed form on the host (tests/test_carrier_host.py holds that to the sequential generator).

NaN rule throughout: at 16 kHz the reference's carrier holds a NaN per period; there the output is NaN at the same
positions and NaN payloads are not compared."""
import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import bits_equal, load_e2e
from tests.test_gpu_parity import RMS_TOL, rms

pytestmark = pytest.mark.gpu

MODE_OF = {"rosenberg": "vocoder", "chord": "vocoder_chord"}
# per-call sizes (tests/test_pool_gpu.py SPECIAL and the usual block): a 0, a 1, odd ones, one of many slices
SIZES = (480, 0, 1, 37, 479, 480, 4097, 600, 13, 2500, 480, 900)


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


def same_bits_or_nan(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def _engine(channels, mode, **kw):
    cfg = E.make_config(channels, mode=mode, **kw)
    return E.PhaseVocoder(cfg.sample_rate, channels, cfg.time_ratio, cfg.pitch_semitones, cfg.mode, cfg.coremode,
                          cfg.fftsize, cfg.hopsize)


def _blocks(x, sizes, rot=0):
    """x cut into blocks of `sizes` (an int: that size throughout; a tuple: cycled from entry `rot`) up to its end"""
    out, pos, k = [], 0, rot
    while pos < x.shape[1]:
        n = sizes if isinstance(sizes, int) else sizes[k % len(sizes)]
        k += 1
        out.append(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n
    return out


def _engine_step(eng, b):
    eng.processInData(b)
    n = eng.getOutSamples()
    y = eng.getOutData(n)
    eng.num_res_ = 0
    return n, y


def _engine_run(eng, blocks):
    return [_engine_step(eng, b) for b in blocks]


def _pool_step(pool, feed):
    pool.feed(feed)
    return {s: (pool.available(s), pool.retrieve(s, pool.available(s))) for s in feed}


def _pool_run(pool, slot, blocks):
    return [_pool_step(pool, {slot: b})[slot] for b in blocks]


def _same(got, want, what=None):
    assert [n for n, _ in got] == [n for n, _ in want], what
    a, b = np.concatenate([y for _, y in got], axis=1), np.concatenate([y for _, y in want], axis=1)
    assert b.shape[1] > 0 and same_bits_or_nan(a, b), (what, a.shape, b.shape)


# ---- 1. the generator kernel alone
@pytest.mark.parametrize("rate", [48000, 16000])
@pytest.mark.parametrize("carrier", ["rosenberg", "chord"])
def test_generator_kernel_matches_the_closed_form(carrier, rate):
    """one launch of seven windows: every count around the workgroup size and the periods, firsts at the periods' ends
    and beyond 2^31 and 2^40"""
    firsts = [0, 109, 110, 378509, (1 << 31) + 12345, (1 << 40) + 777, 0]
    counts = [1, 63, 64, 65, 110, 111, 4097]
    got = E.carrier_device(rate, carrier, firsts, counts)
    assert got.shape == (sum(counts),)
    pos = 0
    for f, n in zip(firsts, counts):
        want = E.plan_carrier(rate, carrier, f, n)
        assert same_bits_or_nan(got[pos:pos + n], want), (f, n)
        pos += n
    assert bool(np.isnan(got).any()) == (rate == 16000)
    # windows in another order, an empty one among them; nothing at all
    got = E.carrier_device(rate, carrier, [378509, 5, 0], [4097, 0, 65])
    assert same_bits_or_nan(got[:4097], E.plan_carrier(rate, carrier, 378509, 4097))
    assert same_bits_or_nan(got[4097:], E.plan_carrier(rate, carrier, 0, 65))
    assert E.carrier_device(rate, carrier, [], []).shape == (0,)


# ---- 2. robotic, whisper and carrier slots of one pool, each against its engine
@pytest.mark.parametrize("fft", [512, 1024, 2048, 4096])
def test_pool_slots_are_their_engines(fft, arith):
    """band lengths 0 (the envelope branch is off), 1, 2 and 4; fft 4096 takes the two-wave analysis.  Slots open at
    different calls, so their carriers sit at different positions within one launch; unequal blocks per call."""
    kinds = ["rosenberg", "robotic", "chord", "whisper", "rosenberg"]
    ncalls, frames = 18, 14000
    pool = E.StreamPool(6, channels=2, mode="robotic", fftsize=fft)
    streams = {}  # slot -> [kind, engine, blocks, next block, got, want]
    for call in range(ncalls):
        if call % 2 == 0 and call // 2 < len(kinds):
            kind = kinds[call // 2]
            s = pool.open(carrier=kind) if kind in MODE_OF else pool.open(voice=kind)
            assert pool.get_carrier(s) == (kind if kind in MODE_OF else "none")
            x = signals.voice(frames, 2, seed=500 + s)
            streams[s] = [kind, _engine(2, MODE_OF.get(kind, kind), fftsize=fft), _blocks(x, SIZES, rot=3 * s), 0, [], []]
        feed = {s: st[2][st[3]] for s, st in streams.items() if st[3] < len(st[2])}
        got = _pool_step(pool, feed)
        for s in feed:
            st = streams[s]
            st[4].append(got[s])
            st[5].append(_engine_step(st[1], feed[s]))
            assert got[s][0] == st[5][-1][0], (call, s, st[0])
            st[3] += 1
    for s, st in streams.items():
        _same(st[4], st[5], (s, st[0]))
        assert pool.info(s) == st[1].info(), (s, st[0])
    assert pool.info(0)["resample"] == 0
    # more than one launch group's worth in all (at fft 4096, hop 1024, the calls hold about a dozen slices), and the
    # 4097-frame call is more than one group by itself at fft 512
    assert pool.info(0)["slices"] > (16 if fft < 4096 else 8 - 1)


# ---- 3. a mixed pool: the slot's own pitch and ratio move the vocoder's hop, and it never resamples
def test_mixed_pool_carrier_slots_beside_resampling_slots():
    x = signals.voice(12000, 2, seed=520)
    blocks = _blocks(x, SIZES)
    pool = E.StreamPool(5, channels=2, mode="robotic", fftsize=1024, pitch_range=(-8.0, 6.0), ratio_range=(0.8, 1.5))
    spec = [("rosenberg", 5.0, 1.0), ("robotic", 3.0, 1.0), ("chord", -7.0, 1.25), ("robotic", -4.0, 1.25), ("rosenberg", 0.0, 1.0)]
    slots, engines = [], []
    for kind, st, tr in spec:
        slots.append(pool.open(semitones=st, time_ratio=tr, carrier=kind if kind in MODE_OF else None))
        engines.append(_engine(2, MODE_OF.get(kind, kind), fftsize=1024, semitones=st, time_ratio=tr))
    got = {s: [] for s in slots}
    for b in blocks:
        step = _pool_step(pool, {s: b for s in slots})
        for s in slots:
            got[s].append(step[s])
    for s, eng, (kind, st, tr) in zip(slots, engines, spec):
        _same(got[s], _engine_run(eng, blocks), (kind, st, tr))
        assert pool.info(s) == eng.info(), (kind, st, tr)
        assert pool.info(s)["resample"] == (0 if kind in MODE_OF else 1), (kind, st, tr)
    assert len({pool.info(s)["hop_in"] for s in (slots[0], slots[2], slots[4])}) == 3  # (the pitch moved the hop)


# ---- 4. channels and sample rates (16 kHz: the NaN carrier)
@pytest.mark.parametrize("rate", [48000, 16000])
@pytest.mark.parametrize("channels", [1, 3])
def test_channels_and_sample_rates(channels, rate):
    x = signals.voice(9000, channels, seed=530 + channels)
    blocks = _blocks(x, SIZES)
    pool = E.StreamPool(3, channels=channels, mode="robotic", fftsize=1024, sample_rate=rate)
    r, a, c = pool.open(), pool.open(carrier="rosenberg"), pool.open(carrier="chord")
    got = {s: [] for s in (r, a, c)}
    for b in blocks:
        step = _pool_step(pool, {r: b, a: b, c: b})
        for s in got:
            got[s].append(step[s])
    for s, mode in ((r, "robotic"), (a, "vocoder"), (c, "vocoder_chord")):
        want = _engine_run(_engine(channels, mode, fftsize=1024, sample_rate=rate), blocks)
        _same(got[s], want, (mode, channels, rate))
        nan = np.isnan(np.concatenate([y for _, y in want], axis=1)).any()
        assert bool(nan) == (rate == 16000 and mode != "robotic"), (mode, rate)


# ---- 5. output piling up: the vocoder's guard is one hop (writeSliceCarrier), not ROBOTIC's
def test_overrun_drops_slices_like_the_engine():
    calls = [9000, 480, 9000]  # (tests/test_gpu_parity.py OVERRUN_GPU: the vocoder case), nothing retrieved in between
    x = signals.voice(sum(calls), 2, seed=55)
    blocks = _blocks(x, tuple(calls))
    pool = E.StreamPool(2, channels=2, mode="robotic", fftsize=512)
    s = pool.open(carrier="chord")
    eng = _engine(2, "vocoder_chord", fftsize=512)
    full = False
    for k, b in enumerate(blocks):
        planned = int(pool.plan_feed([s], [b.shape[1]])[0])
        pool.feed({s: b})
        eng.processInData(b)
        assert pool.available(s) == eng.getOutSamples() == planned, k
        full = full or pool.available(s) >= pool.info(s)["outbuf_capacity"] - 2 * 512
    assert full and pool.info(s) == eng.info()  # the case really drives the ring full
    n = pool.available(s)
    assert same_bits_or_nan(pool.retrieve(s, n), eng.getOutData(n))
    # ... and on from there
    tail = _blocks(signals.voice(2000, 2, seed=56), 480)
    eng.num_res_ = 0
    _same(_pool_run(pool, s, tail), _engine_run(eng, tail))


# ---- 6. the device feed, both wires
@pytest.mark.parametrize("wire", ["f32", "i16"])
def test_feed_device_equals_feed_and_retrieve(wire):
    i16 = wire == "i16"
    x = signals.voice(480 * 20, 2, seed=540)
    if i16:
        xi = np.round(x * 32767.0).astype(np.int16)
        xf = xi.astype(np.float32) * np.float32(1.0 / 32768.0)
    blocks_f = _blocks(xf if i16 else x, 480)
    blocks_w = _blocks(xi, 480) if i16 else blocks_f
    pool, twin = (E.StreamPool(3, channels=2, mode="robotic", fftsize=2048) for _ in range(2))
    slots = [pool.open(carrier="rosenberg"), pool.open(), pool.open(carrier="chord")]
    assert slots == [twin.open(carrier="rosenberg"), twin.open(), twin.open(carrier="chord")]
    want, pending, total = [], [], 0
    for k, (bw, bf) in enumerate(zip(blocks_w, blocks_f)):
        d_x = torch.from_numpy(np.stack([bw] * 3)).cuda()
        planned = pool.plan_feed(slots, [480] * 3)
        out, frames = pool.feed_device(slots, d_x)
        assert [int(f) for f in frames] == [int(f) for f in planned], k
        twin.feed({s: bf for s in slots})
        y = [twin.retrieve(s, twin.available(s)) for s in slots]
        assert [int(f) for f in frames] == [v.shape[1] for v in y], k
        want.append(y)
        pending.append((out, frames))
        if len(pending) == 4 or k == len(blocks_w) - 1:  # four calls in flight, then their results
            torch.cuda.synchronize()
            for (o, fr), ys in zip(pending, want[-len(pending):]):
                for i, v in enumerate(ys):
                    g = o[i, :, :int(fr[i])].cpu().numpy()
                    total += g.shape[1]
                    if i16:
                        v = np.trunc(np.clip(v * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)
                        assert np.array_equal(g, v)
                    else:
                        assert same_bits_or_nan(g, v)
            pending = []
    assert total > 0


# ---- 7. against the oracle: the existing 1e-4 bar with its NaN rule
def _offline_through_slot(x, block=480, **kw):
    """the reference CLI's offline loop (engine.run_offline) through a carrier slot"""
    mode = kw.pop("mode")
    carrier = {v: k for k, v in MODE_OF.items()}[mode]
    ch, frames = x.shape
    pool = E.StreamPool(1, channels=ch, mode="robotic", **kw)
    s = pool.open(carrier=carrier)
    outs, counts, produced = [], [], 0
    for b in _blocks(x, block):
        n, y = _pool_step(pool, {s: b})[s]
        outs.append(y), counts.append(n)
        produced += n
    z = np.zeros((ch, block), np.float32)
    while produced < frames:
        n, y = _pool_step(pool, {s: z})[s]
        counts.append(n), outs.append(y[:, :frames - produced])
        produced += outs[-1].shape[1]
    return np.concatenate(outs, axis=1), counts


@pytest.mark.parametrize("mode", ["vocoder", "vocoder_chord"])
def test_slot_against_the_oracle(mode):
    x = signals.voice(12000, 2, seed=41)
    want, wc, _ = O.run_offline(x, mode=mode, fftsize=2048)
    got, counts = _offline_through_slot(x, mode=mode, fftsize=2048)
    assert counts == wc and got.shape == want.shape
    err = rms(got, want)
    print(f"{mode} slot vs oracle: RMS {err:.3e}")
    assert err <= RMS_TOL


@pytest.mark.parametrize("name", ["vocoder_rosenberg", "vocoder_chord", "vocoder_16k_nan_carrier"])
def test_golden_fixtures_through_a_slot(name):
    x, y, counts, meta = load_e2e(name)
    got, cnt = _offline_through_slot(x, **meta)
    assert cnt == counts and got.shape == y.shape
    err = rms(got, y)
    print(f"{name} through a slot: RMS {err:.3e}")
    assert err <= RMS_TOL


# ---- 8. launch counts and census: K = 2 per launch group with a carrier slot (the generator and its analysis)
@pytest.mark.parametrize("mixed", [False, True], ids=["pool", "pmix"])
def test_launch_counts_and_census(mixed):
    K = 2
    kw = dict(channels=2, mode="robotic", fftsize=1024)
    if mixed:
        kw.update(pitch_range=(-2.0, 2.0), ratio_range=(1.0, 1.0))
    x = [signals.voice(6000, 2, seed=550 + i) for i in range(3)]
    blocks = [_blocks(v, 480) for v in x]
    with_car, plain, touched = (E.StreamPool(3, **kw) for _ in range(3))
    slots = [with_car.open() for _ in range(3)]
    assert slots == [plain.open() for _ in range(3)] == [touched.open() for _ in range(3)]
    with_car.set_carrier(1, "chord")
    for s in slots:  # set and taken back: a robotic pool again
        touched.set_carrier(s, "rosenberg")
        touched.set_carrier(s, "none")
    set_name = "pmix" if mixed else "pool"
    E.chain_census(True)
    try:
        groups = 0
        got, want = {s: [] for s in slots}, {s: [] for s in slots}
        for k in range(len(blocks[0])):
            before = with_car.info(1)["slices"]
            feed = {s: blocks[s][k] for s in slots}
            g, w, t = _pool_step(with_car, feed), _pool_step(plain, feed), _pool_step(touched, feed)
            made = with_car.info(1)["slices"] - before  # (every slot has the same schedule: one launch group or none)
            assert 0 <= made <= 16
            assert plain.last_launches() == touched.last_launches(), k
            assert with_car.last_launches() == plain.last_launches() + (K if made else 0), k
            groups += 1 if made else 0
            for s in slots:
                got[s].append(g[s]), want[s].append(w[s])
                assert bits_equal(t[s][1], w[s][1])
        census = E.analysis_census_read()
        for _ in range(3):  # the carrier slot sits out: the robotic count
            with_car.feed({0: blocks[0][0], 2: blocks[2][0]})
            plain.feed({0: blocks[0][0], 2: blocks[2][0]})
            assert with_car.last_launches() == plain.last_launches() > 0
    finally:
        E.chain_census(False)
    for s in (0, 2):
        _same(got[s], want[s])
    _same(got[1], _engine_run(_engine(2, "vocoder_chord", fftsize=1024), blocks[1]))
    # the analysis of the set ran once per group for each pool, and once more per group with a carrier slot
    ana = sum(n for key, n in census.items() if key[0] == set_name)
    assert groups > 0 and all(key[0] == set_name for key in census), census
    assert ana == 3 * groups + groups, (census, groups)


# ---- 9. refusals, each leaving the slot as it was
def test_refusals_change_nothing():
    x = signals.voice(4800, 2, seed=560)
    blocks = _blocks(x, 480)
    rob = E.StreamPool(3, channels=2, mode="robotic", fftsize=1024)
    s, w = rob.open(), rob.open(voice="whisper")
    c = rob.open(carrier="rosenberg")
    with pytest.raises(E.PvError, match="invalid"):  # an unknown carrier, a slot that is not open
        rob.set_carrier(s, 7)
    rob.close(c)
    with pytest.raises(E.PvError, match="invalid"):
        rob.set_carrier(c, "chord")
    c = rob.open(carrier="rosenberg")
    with pytest.raises(E.PvError, match="invalid"):  # a stream is one engine
        rob.set_carrier(w, "chord")
    assert "WHISPER" in E.lib().pv_last_error().decode()
    with pytest.raises(E.PvError, match="invalid"):
        rob.set_voice(c, "whisper")
    assert (rob.get_carrier(s), rob.get_carrier(w), rob.get_carrier(c)) == ("none", "none", "rosenberg")
    assert (rob.get_voice(s), rob.get_voice(w), rob.get_voice(c)) == ("robotic", "whisper", "robotic")
    engines = {s: _engine(2, "robotic", fftsize=1024), w: _engine(2, "whisper", fftsize=1024), c: _engine(2, "vocoder", fftsize=1024)}
    got = {q: [] for q in engines}
    want = {q: _engine_run(e, blocks) for q, e in engines.items()}
    for k, b in enumerate(blocks):
        if k == 5:  # after the first slice
            assert rob.info(s)["slices"] > 0
            with pytest.raises(E.PvError, match="invalid"):
                rob.set_carrier(s, "chord")
            with pytest.raises(E.PvError, match="invalid"):
                rob.set_carrier(c, "none")
            assert rob.get_carrier(s) == "none" and rob.get_carrier(c) == "rosenberg"
        step = _pool_step(rob, {q: b for q in engines})
        for q in engines:
            got[q].append(step[q])
    for q in engines:
        _same(got[q], want[q], q)

    # a uniform pool whose configuration resamples; a pool that is not ROBOTIC
    for kw, why in ((dict(mode="robotic", semitones=4.0), "pv_pool_create_mixed"), (dict(mode="normal_pitchshift", semitones=0.0), "ROBOTIC")):
        pool, twin = (E.StreamPool(2, channels=2, fftsize=1024, **kw) for _ in range(2))
        s, t = pool.open(), twin.open()
        with pytest.raises(E.PvError, match="unsupported"):
            pool.set_carrier(s, "rosenberg")
        assert why in E.lib().pv_last_error().decode()
        with pytest.raises(E.PvError, match="unsupported"):
            pool.open(carrier="chord")
        assert pool.open() == 1  # (the refused open left no slot behind)
        assert pool.get_carrier(s) == "none"
        _same(_pool_run(pool, s, blocks), _pool_run(twin, t, blocks))
    # ... while a uniform pool at pitch 0 takes the setting at any time ratio
    pool = E.StreamPool(1, channels=2, mode="robotic", fftsize=1024, time_ratio=1.25)
    s = pool.open(carrier="chord")
    _same(_pool_run(pool, s, blocks), _engine_run(_engine(2, "vocoder_chord", fftsize=1024, time_ratio=1.25), blocks))


# ---- 10. snapshots: version 3, restored elsewhere and forked, the carrier row rewritten from the closed form
def test_snapshot_restore_and_fork():
    x = signals.voice(14000, 2, seed=570)
    blocks = _blocks(x, 480)
    want = _engine_run(_engine(2, "vocoder"), blocks)
    a = E.StreamPool(4, channels=2, mode="robotic")
    b = E.StreamPool(6, channels=2, mode="robotic")
    never = E.StreamPool(4, channels=2, mode="robotic")
    rob_a, s, rob_never = a.open(), a.open(carrier="rosenberg"), never.open()
    assert rob_a == rob_never
    cut, held = 15, 3  # saved after `cut` feeds; the output of the last `held` of them is still pending then
    got = []
    for k in range(cut):
        a.feed({s: blocks[k], rob_a: blocks[k]})
        never.feed({rob_never: blocks[k]})
        if k < cut - held:
            assert a.available(s) == want[k][0], k
            got.append(a.retrieve(s, a.available(s)))
    pending = a.available(s)
    assert pending == sum(n for n, _ in want[cut - held:cut]) and pending > 0
    blob = a.save(s)
    info = E.blob_info(blob)
    assert info["cfg"]["mode"] == E.MODES["vocoder"] and info["version"] == 3 and info["pending_frames"] == pending
    assert a.save(s) == blob  # two saves of one history
    # a robotic neighbour's blob does not know of the carrier: version 1, the same bytes
    rob_blob = a.save(rob_a)
    assert E.blob_info(rob_blob)["version"] == 1 and E.blob_info(rob_blob)["cfg"]["mode"] == E.ROBOTIC
    assert rob_blob == never.save(rob_never)
    b.open(), b.open()  # (another slot index in the other pool, whose carrier buffers do not exist yet)
    t = b.restore(blob)
    f = a.fork(s)
    assert t == 2 and b.get_carrier(t) == "rosenberg" and a.get_carrier(f) == "rosenberg"
    assert b.available(t) == pending == a.available(f)
    assert b.save(t) == blob
    copies = {"restored": (b, t, list(got)), "forked": (a, f, list(got)), "original": (a, s, list(got))}
    for pool, q, acc in copies.values():
        acc.append(pool.retrieve(q, pending))
    for k in range(cut, len(blocks)):
        b.feed({t: blocks[k]})
        a.feed({f: blocks[k], s: blocks[k], rob_a: blocks[k]})
        for name, (pool, q, acc) in copies.items():
            assert pool.available(q) == want[k][0], (name, k)
            acc.append(pool.retrieve(q, pool.available(q)))
    full = np.concatenate([y for _, y in want], axis=1)
    for name, (_, _, acc) in copies.items():
        assert bits_equal(np.concatenate(acc, axis=1), full), name
    # a chord slot of a mixed pool at a pitch of its own, into a mixed pool; refused where its engine cannot live
    m = E.StreamPool(2, channels=2, mode="robotic", pitch_range=(-5.0, 5.0))
    u = m.open(semitones=4.0, carrier="chord")
    wantc = _engine_run(_engine(2, "vocoder_chord", semitones=4.0), blocks)
    head = _pool_run(m, u, blocks[:9])
    cblob = m.save(u)
    assert E.blob_info(cblob)["version"] == 3 and E.blob_info(cblob)["cfg"]["mode"] == E.MODES["vocoder_chord"]
    v = m.restore(cblob)
    assert m.info(v)["resample"] == 0 and m.get_carrier(v) == "chord"
    _same(head + _pool_run(m, v, blocks[9:]), wantc)
    # (a uniform pool at +4 st resamples: it keeps a stream ring the blob's pool does not size alike, and its one
    # kernel variant could not run the slot either -- whichever the restore names first, nothing is left behind)
    uniform = E.StreamPool(2, channels=2, mode="robotic", semitones=4.0)
    with pytest.raises(E.PvError, match="unsupported|invalid"):
        uniform.restore(cblob)
    assert uniform.open() == 0
    other = E.StreamPool(2, channels=2, mode="normal_pitchshift", semitones=0.0)
    with pytest.raises(E.PvError, match="mode"):
        other.restore(blob)
