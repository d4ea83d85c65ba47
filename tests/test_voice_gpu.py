"""The voice setting on the GPU (include/audiomod_pv.h "Voice setting"): a slot or stream of a ROBOTIC pool, mixed pool
or mixed batch that is given the WHISPER voice must be, bit for bit, the single-stream engine / Batch(1, ...) of mode
WHISPER -- its own rand() sequence from the default seed -- whatever its neighbours do; with the setting untouched an
object launches what it always launched.  The phases come from the device generator (pv_whisper_kernel), which is
checked on its own first."""
import os
import subprocess

import numpy as np
import pytest
import torch

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import bits_equal

pytestmark = pytest.mark.gpu

FRAMES = 20000
CUTS = (1, 63, 64, 65, 681, 682, 683, 2050, 4101)
RMS_TOL = 1e-4  # (tests/test_gpu_parity.py test_constant_and_whisper_modes)
IRREGULAR = (0, 1, 479, 7000, 13, 480, 0, 2500, 960, 1, 3000)  # a 0, a 1, one block of many slices


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


def _engine(channels, mode="whisper", **kw):
    cfg = E.make_config(channels, mode=mode, **kw)
    return E.PhaseVocoder(cfg.sample_rate, channels, cfg.time_ratio, cfg.pitch_semitones, cfg.mode, cfg.coremode,
                          cfg.fftsize, cfg.hopsize)


def _blocks(x, sizes):
    """x cut into blocks of `sizes` (an int: that size throughout; a tuple: cycled) up to its end"""
    out, pos, k = [], 0, 0
    while pos < x.shape[1]:
        n = sizes if isinstance(sizes, int) else sizes[k % len(sizes)]
        k += 1
        out.append(np.ascontiguousarray(x[:, pos:pos + n]))
        pos += n
    return out


def _engine_run(eng, blocks):
    """[(available, samples)] per block of the single-stream engine"""
    out = []
    for b in blocks:
        eng.processInData(b)
        n = eng.getOutSamples()
        out.append((n, eng.getOutData(n)))
        eng.num_res_ = 0
    return out


def _pool_run(pool, slot, blocks):
    out = []
    for b in blocks:
        pool.feed({slot: b})
        n = pool.available(slot)
        out.append((n, pool.retrieve(slot, n)))
    return out


def _same(got, want):
    assert [n for n, _ in got] == [n for n, _ in want]
    a, b = np.concatenate([y for _, y in got], axis=1), np.concatenate([y for _, y in want], axis=1)
    assert b.shape[1] > 0 and bits_equal(a, b), (a.shape, b.shape)


# ---- 1. the generator kernel alone
def test_generator_kernel_matches_rand():
    total = 200000
    want = E.whisper_phases(total)
    assert bits_equal(E.whisper_device_phases([total]), want)
    for cut in CUTS:
        assert bits_equal(E.whisper_device_phases([cut, total - cut]), want), cut
    row = list(CUTS) + [0, 1]
    assert bits_equal(E.whisper_device_phases(row + [total - sum(row)]), want)
    assert E.whisper_device_phases([]).shape == (0,) and E.whisper_device_phases([0, 0]).shape == (0,)


# ---- 2. a pool slot against the WHISPER engine
@pytest.mark.parametrize("sizes", [480, IRREGULAR], ids=["480", "irregular"])
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fft", [512, 2048])
def test_pool_slot_is_the_whisper_engine(fft, channels, sizes, arith):
    x = signals.voice(FRAMES, channels, seed=300 + channels)
    blocks = _blocks(x, sizes)
    pool = E.StreamPool(2, channels=channels, mode="robotic", fftsize=fft)
    s = pool.open(voice="whisper")
    assert pool.get_voice(s) == "whisper"
    _same(_pool_run(pool, s, blocks), _engine_run(_engine(channels, fftsize=fft), blocks))
    assert pool.info(s)["slices"] > 16  # (more than one launch group's worth in all)


def test_pool_slot_fft4096():
    x = signals.voice(FRAMES, 2, seed=310)
    blocks = _blocks(x, IRREGULAR)
    pool = E.StreamPool(1, channels=2, mode="robotic", fftsize=4096)
    s = pool.open(voice="whisper")
    _same(_pool_run(pool, s, blocks), _engine_run(_engine(2, fftsize=4096), blocks))


def test_pool_slot_against_the_oracle():
    """the reference CLI's offline loop through a whisper slot, against the oracle itself"""
    x = signals.voice(FRAMES, 2, seed=41)
    want, wc, _ = O.run_offline(x, mode="whisper")
    pool = E.StreamPool(1, channels=2, mode="robotic")
    s = pool.open(voice="whisper")
    outs, counts, produced = [], [], 0
    for b in _blocks(x, 480):
        pool.feed({s: b})
        counts.append(pool.available(s))
        outs.append(pool.retrieve(s, counts[-1]))
        produced += counts[-1]
    z = np.zeros((2, 480), np.float32)
    while produced < FRAMES:
        pool.feed({s: z})
        counts.append(pool.available(s))
        outs.append(pool.retrieve(s, counts[-1])[:, :FRAMES - produced])
        produced += outs[-1].shape[1]
    got = np.concatenate(outs, axis=1)
    assert counts == wc and got.shape == want.shape
    rms = float(np.sqrt(np.mean((got.astype(np.float64) - want) ** 2)))
    print(f"whisper slot vs oracle: RMS {rms:.3e}")
    assert rms <= RMS_TOL


# ---- 3. every slot has its own stream: staggered opens, close and reopen
def test_slots_opened_apart_and_reopened_are_fresh_streams():
    x = [signals.voice(9000, 2, seed=320 + i) for i in range(3)]
    blocks = [_blocks(v, 480) for v in x]
    want = [_engine_run(_engine(2), b) for b in blocks]
    pool = E.StreamPool(3, channels=2, mode="robotic")
    a = pool.open(voice="whisper")
    got = {0: [], 1: [], 2: []}
    live = {a: 0}  # slot -> stream
    pos = {0: 0, 1: 0, 2: 0}
    for call in range(64):
        if call == 7:  # a second whisper slot, seven feeds later
            live[pool.open(voice="whisper")] = 1
        if call == 12:  # the first slot closes in mid-stream and comes back as a fresh stream
            assert pool.info(a)["slices"] > 0
            pool.close(a)
            del live[a]
            s = pool.open(voice="whisper")
            assert s == a and pool.info(s)["slices"] == 0 and pool.get_voice(s) == "whisper"
            live[s] = 2
        feed = {s: blocks[i][pos[i]] for s, i in live.items() if pos[i] < len(blocks[i])}
        if not feed:
            break
        pool.feed(feed)
        for s in feed:
            i = live[s]
            n = pool.available(s)
            got[i].append((n, pool.retrieve(s, n)))
            pos[i] += 1
    assert pos[1] == len(blocks[1]) and pos[2] == len(blocks[2])
    _same(got[1], want[1])
    _same(got[2], want[2])


# ---- 4. robotic and whisper slots side by side; launch counts; census
def test_voices_side_by_side_launches_and_census():
    kw = dict(mode="robotic", fftsize=1024)
    x = [signals.voice(6000, 2, seed=330 + i) for i in range(4)]
    blocks = [_blocks(v, 480) for v in x]
    mixed, plain, touched = (E.StreamPool(4, channels=2, **kw) for _ in range(3))
    slots = [mixed.open() for _ in range(4)]
    assert slots == [plain.open() for _ in range(4)] == [touched.open() for _ in range(4)]
    mixed.set_voice(1, "whisper")
    mixed.set_voice(3, "whisper")
    for s in slots:
        touched.set_voice(s, "robotic")
    assert [mixed.get_voice(s) for s in slots] == ["robotic", "whisper", "robotic", "whisper"]
    ref = {s: _engine_run(_engine(2, fftsize=1024), blocks[s]) for s in (1, 3)}
    E.chain_census(True)
    try:
        got = {s: [] for s in slots}
        want_rob = {0: [], 2: []}
        generator_launches = 0
        for k in range(len(blocks[0])):
            feed = {s: blocks[s][k] for s in slots}
            before = mixed.info(1)["slices"]
            mixed.feed(feed), plain.feed(feed), touched.feed(feed)
            made = mixed.info(1)["slices"] - before  # (every slot has the same schedule: one launch group or none)
            assert 0 <= made <= 16
            assert plain.last_launches() == touched.last_launches(), k
            assert mixed.last_launches() == plain.last_launches() + (1 if made else 0), k
            generator_launches += 1 if made else 0
            for s in slots:
                n = mixed.available(s)
                got[s].append((n, mixed.retrieve(s, n)))
            for s in (0, 2):
                n = plain.available(s)
                want_rob[s].append((n, plain.retrieve(s, n)))
        census = E.voice_census_read()
    finally:
        E.chain_census(False)
    for s in (0, 2):
        _same(got[s], want_rob[s])
    for s in (1, 3):
        _same(got[s], ref[s])
    # one generator launch per feed of `mixed` that made slices, none for the two all-robotic pools
    assert generator_launches > 0 and census == {("pool", 512): generator_launches}


# ---- 5. the device feed, both wires, four calls in flight
@pytest.mark.parametrize("wire", ["f32", "i16"])
def test_feed_device_equals_feed_and_retrieve(wire):
    i16 = wire == "i16"
    x = signals.voice(480 * 24, 2, seed=340)
    if i16:
        xi = np.round(x * 32767.0).astype(np.int16)
        xf = xi.astype(np.float32) * np.float32(1.0 / 32768.0)
    blocks_f = _blocks(xf if i16 else x, 480)
    blocks_w = _blocks(xi, 480) if i16 else blocks_f
    pool, twin = (E.StreamPool(2, channels=2, mode="robotic", fftsize=2048) for _ in range(2))
    s, t = pool.open(voice="whisper"), twin.open(voice="whisper")
    r = pool.open()  # a robotic neighbour in the same calls
    assert twin.open() == r
    want, pending = [], []
    for k, (bw, bf) in enumerate(zip(blocks_w, blocks_f)):
        d_x = torch.from_numpy(np.stack([bw, bw])).cuda()
        out, frames = pool.feed_device([s, r], d_x)
        twin.feed({t: bf, r: bf})
        y = [twin.retrieve(q, twin.available(q)) for q in (t, r)]
        assert [int(f) for f in frames] == [v.shape[1] for v in y], k
        want.append(y)
        pending.append((out, frames))
        if len(pending) == 4 or k == len(blocks_w) - 1:  # four calls in flight, then their results
            torch.cuda.synchronize()
            for (o, fr), ys in zip(pending, want[-len(pending):]):
                for i, v in enumerate(ys):
                    g = o[i, :, :int(fr[i])].cpu().numpy()
                    if i16:
                        v = np.trunc(np.clip(v * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)
                        assert np.array_equal(g, v)
                    else:
                        assert bits_equal(g, v)
            pending = []
    assert sum(v[0].shape[1] for v in want) > 0


# ---- 6. a mixed ROBOTIC pool: the slot's own pitch and ratio
def test_mixed_pool_slot_uses_its_pitch_and_ratio():
    x = signals.voice(FRAMES, 2, seed=350)
    blocks = _blocks(x, IRREGULAR)
    pool = E.StreamPool(3, channels=2, mode="robotic", pitch_range=(-5.0, 5.0), ratio_range=(0.8, 1.5))
    r = pool.open(semitones=-2.0, time_ratio=1.0)
    s = pool.open(semitones=3.0, time_ratio=1.25, voice="whisper")
    want = _engine_run(_engine(2, semitones=3.0, time_ratio=1.25), blocks)
    want_r = _engine_run(_engine(2, mode="robotic", semitones=-2.0, time_ratio=1.0), blocks)
    got, got_r = [], []
    for b in blocks:
        pool.feed({r: b, s: b})
        for q, acc in ((s, got), (r, got_r)):
            n = pool.available(q)
            acc.append((n, pool.retrieve(q, n)))
    _same(got, want)
    _same(got_r, want_r)


# ---- 7. snapshots
def test_snapshot_carries_voice_and_generator_state():
    x = signals.voice(FRAMES, 2, seed=360)
    blocks = _blocks(x, 480)
    want = _engine_run(_engine(2), blocks)
    a = E.StreamPool(3, channels=2, mode="robotic")
    b = E.StreamPool(5, channels=2, mode="robotic")
    never = E.StreamPool(3, channels=2, mode="robotic")
    rob_a, s, rob_never = a.open(), a.open(voice="whisper"), never.open()
    assert rob_a == rob_never
    cut, held = 17, 3  # saved after `cut` feeds; the output of the last `held` of them is still pending then
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
    assert info["cfg"]["mode"] == E.WHISPER and info["version"] == 2 and info["pending_frames"] == pending
    # a robotic slot's blob does not know that a neighbour whispers: version 1, the same bytes
    rob_blob = a.save(rob_a)
    assert E.blob_info(rob_blob)["version"] == 1 and E.blob_info(rob_blob)["cfg"]["mode"] == E.ROBOTIC
    assert rob_blob == never.save(rob_never)
    b.open(), b.open()  # (another slot index in the other pool)
    t = b.restore(blob)
    assert t == 2 and b.get_voice(t) == "whisper" and b.available(t) == pending
    got.append(b.retrieve(t, pending))
    for k in range(cut, len(blocks)):
        b.feed({t: blocks[k]})
        assert b.available(t) == want[k][0], k
        got.append(b.retrieve(t, b.available(t)))
    assert bits_equal(np.concatenate(got, axis=1), np.concatenate([y for _, y in want], axis=1))
    # both kinds in one call
    both = a.save([rob_a, s])
    assert both[0] == rob_blob and both[1] == blob
    # a pool that is not ROBOTIC refuses the blob like any other mismatch
    other = E.StreamPool(2, channels=2, mode="normal_pitchshift", semitones=0.0)
    with pytest.raises(E.PvError, match="mode"):
        other.restore(blob)


# ---- 8. the mixed batch
def test_mixed_batch_streams_are_whisper_batches():
    voices = ["whisper", "robotic", "whisper", "whisper"]
    streams = [(1, 0.0, 1.0), (700, 3.0, 1.0), (4801, 0.0, 1.0), (12000, 3.0, 1.0)]
    clips = [signals.voice(f, 2, seed=370 + i) for i, (f, _, _) in enumerate(streams)]
    mb = E.MixedBatch(streams, channels=2, mode="robotic", fftsize=1024)
    fresh_launches = mb.kernel_launches
    mb.set_voice(voices)
    assert mb.kernel_launches == fresh_launches  # (the table is drawn by set_voice: a run launches nothing more)
    d_in = mb.pack(clips)
    first = [y.cpu().numpy() for y in mb.split(mb.run(d_in))]
    second = [y.cpu().numpy() for y in mb.split(mb.run(d_in))]
    for i, ((f, st, tr), v) in enumerate(zip(streams, voices)):
        bt = E.Batch(1, f, channels=2, mode=v, fftsize=1024, semitones=st, time_ratio=tr)
        want = bt.run(torch.from_numpy(clips[i][None]).cuda())
        torch.cuda.synchronize()
        want = want.cpu().numpy()[0]
        assert bits_equal(first[i], want), (i, v)
        assert bits_equal(second[i], first[i]), i
    # the PCM wire: 16-bit clips in, the float run's samples converted as the WAV writer does
    pcm = [np.round(c.T * 32767.0).astype(np.int16) for c in clips]
    as_float = [p.T.astype(np.float32) * np.float32(1.0 / 32768.0) for p in pcm]
    want16 = [y.cpu().numpy() for y in mb.split(mb.run(mb.pack(as_float)))]
    got16 = [y.cpu().numpy() for y in mb.split_pcm(mb.run_pcm(mb.pack_pcm(pcm)))]
    for i in range(len(streams)):
        w = np.trunc(np.clip(want16[i] * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))).astype(np.int16)
        assert np.array_equal(got16[i], w.T), i
    # a redraw: every stream robotic again, the launches of a fresh object
    mb.redraw(streams)
    assert mb.kernel_launches == fresh_launches
    again = [y.cpu().numpy() for y in mb.split(mb.run(d_in))]
    rob = E.MixedBatch(streams, channels=2, mode="robotic", fftsize=1024)
    want_rob = [y.cpu().numpy() for y in rob.split(rob.run(d_in))]
    assert all(bits_equal(g, w) for g, w in zip(again, want_rob))
    assert not bits_equal(again[2], first[2])


# ---- 9. refusals, each leaving the object's next output as it would have been
def test_refusals_change_nothing():
    x = signals.voice(4800, 2, seed=380)
    blocks = _blocks(x, 480)
    pool, twin = (E.StreamPool(2, channels=2, mode="normal_pitchshift", semitones=2.0) for _ in range(2))
    s, t = pool.open(), twin.open()
    with pytest.raises(E.PvError, match="unsupported"):
        pool.set_voice(s, "whisper")
    assert "ROBOTIC" in E.lib().pv_last_error().decode()
    with pytest.raises(E.PvError, match="unsupported"):
        pool.open(voice="whisper")
    assert pool.open() == 1  # (the refused open left no slot behind)
    _same(_pool_run(pool, s, blocks), _pool_run(twin, t, blocks))

    rob, rtwin = (E.StreamPool(2, channels=2, mode="robotic") for _ in range(2))
    s, t = rob.open(), rtwin.open()
    for bad, why in ((lambda: rob.set_voice(s, 7), "invalid"), (lambda: rob.set_voice(1, "whisper"), "invalid")):
        with pytest.raises(E.PvError, match=why):
            bad()
    head = _pool_run(rob, s, blocks[:5]), _pool_run(rtwin, t, blocks[:5])
    assert rob.info(s)["slices"] > 0
    with pytest.raises(E.PvError, match="invalid"):  # after the first slice
        rob.set_voice(s, "whisper")
    assert rob.get_voice(s) == "robotic"
    _same(head[0] + _pool_run(rob, s, blocks[5:]), head[1] + _pool_run(rtwin, t, blocks[5:]))

    streams = [(3000, 2.0, 1.0), (700, 0.0, 1.0)]
    clips = [signals.voice(f, 2, seed=390 + i) for i, (f, _, _) in enumerate(streams)]
    mb, mtwin = (E.MixedBatch(streams, channels=2, mode="normal_pitchshift") for _ in range(2))
    with pytest.raises(E.PvError, match="unsupported"):
        mb.set_voice(["whisper", "robotic"])
    d_in = mb.pack(clips)
    assert all(bits_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(mb.split(mb.run(d_in)), mtwin.split(mtwin.run(d_in))))
    mrob = E.MixedBatch(streams, channels=2, mode="robotic")
    with pytest.raises(E.PvError, match="invalid"):
        mrob.set_voice([1, 7])
    with pytest.raises(E.PvError):
        mrob.set_voice(["whisper"])


# ---- 10. the command-line tool
def test_cli_batch_whisper_takes_the_mixed_batch(tmp_path):
    from tests.test_cli_batch_gpu import CLI, TIMEOUT, _wav_bytes
    ins = []
    for i, spec in enumerate(((48000, 2, 16, 4801), (48000, 2, 24, 9000))):
        p = tmp_path / f"in{i}.wav"
        p.write_bytes(_wav_bytes(*spec, seed=800 + i))
        ins.append(str(p))
    outs = [str(tmp_path / f"out{i}.wav") for i in range(2)]
    man = tmp_path / "jobs.tsv"
    man.write_text("".join(f"{a}\t{b}\n" for a, b in zip(ins, outs)))
    census = tmp_path / "census.txt"
    env = dict(os.environ, AUDIOMOD_PV_CHAIN_CENSUS=str(census))
    r = subprocess.run([CLI, "batch", "whisper", str(man)], capture_output=True, text=True, timeout=TIMEOUT, env=env)
    assert r.returncode == 0, r.stderr
    assert [l.split("\t")[:2] for l in r.stdout.splitlines()] == [["ok", o] for o in outs], r.stdout
    lines = census.read_text().splitlines()
    chain = [l for l in lines if l.startswith("chain ")]
    assert chain and all("set=mb " in l for l in chain), lines
    for i, o in zip(ins, outs):
        single = str(tmp_path / "single.wav")
        q = subprocess.run([CLI, "whisper", i, single], capture_output=True, text=True, timeout=TIMEOUT)
        assert q.returncode == 0, q.stderr
        assert open(o, "rb").read() == open(single, "rb").read(), i
