"""GPU parity tests proper: the HIP path, through the C ABI, against the committed golden vectors
(captured from the compiled reference) and against the oracle on seeded inputs.

Tolerance (BASELINE.json north_star): output within 1e-4 RMS of the reference on identical input.
Everything that involves no device transcendental on a non-trivial argument must be BIT-exact
(integer scheduling, FFT, magnitudes, OLA, resampler)."""
import os

import numpy as np
import pytest

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import assert_shape, bits_equal, e2e_cases, load_e2e, oracle_floor

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rms(a, b):
    """RMS difference over the samples that are finite in the expected output `b`.  The reference emits NaN in a
    few situations (its Rosenberg carrier below ~22 kHz); there the engine has to be non-finite at the same
    positions: inf is returned if it is not."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(b)
    if a.shape != b.shape or not np.array_equal(np.isfinite(a), fin):
        return float("inf")
    return float(np.sqrt(np.mean((a[fin] - b[fin]) ** 2))) if fin.any() else 0.0


@pytest.mark.parametrize("name", e2e_cases())
def test_golden_streaming(name):
    x, y, counts, meta = load_e2e(name)
    api = meta.pop("api", "offline")
    if api == "rt":
        got, cnt = E.run_realtime(x, **meta)
    else:
        got, cnt = E.run_offline(x, **meta)
    assert cnt == counts
    assert got.shape == y.shape
    assert rms(got, y) <= RMS_TOL
    fin = np.isfinite(y)
    assert np.max(np.abs(got[fin] - y[fin]), initial=0.0) <= 2e-3


@pytest.mark.parametrize("name", [n for n in e2e_cases() if not n.startswith("rt_")])
def test_golden_batch(name):
    import torch
    x, y, counts, meta = load_e2e(name)
    flush = meta.pop("flush", True)
    S = 3
    b = E.Batch(S, x.shape[1], channels=x.shape[0], flush=flush, **meta)
    assert b.out_frames == y.shape[1]
    d_in = torch.from_numpy(np.stack([x] * S)).cuda()
    out = b.run(d_in)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for s in range(S):
        assert rms(out[s], y) <= RMS_TOL
    assert bits_equal(out[0], out[1]) and bits_equal(out[0], out[2])
    b.close()


def test_robotic_bit_exact():
    """phase == 0 everywhere: cosf(0) = 1, sinf(0) = 0, so the whole chain must match bit for bit."""
    x = signals.voice(20000, 2, seed=3)
    want, wc, _ = O.run_offline(x, mode="robotic")
    got, gc = E.run_offline(x, mode="robotic")
    assert gc == wc
    assert bits_equal(got, want)


def test_robotic_bit_exact_4096():
    x = signals.noise(20000, 2)
    want, wc, _ = O.run_offline(x, mode="robotic", fftsize=4096)
    got, gc = E.run_offline(x, mode="robotic", fftsize=4096)
    assert gc == wc
    assert bits_equal(got, want)


CASES = [
    dict(semitones=5.0, coremode=1),
    dict(semitones=-5.0, coremode=0),
    dict(semitones=2.0, coremode=2, fftsize=1024),
    dict(mode="time_stretch", time_ratio=0.75, flush=False),
    dict(mode="time_stretch", time_ratio=2.0, flush=False),
    dict(mode="time_stretch", time_ratio=1.0, coremode=0, flush=False),
    dict(mode="gender_change", semitones=0.0),
    dict(mode="formant_pitchshift", semitones=3.0, fftsize=4096),
    dict(semitones=12.0),
    dict(semitones=-12.0),
    dict(semitones=4.0, fftsize=512),
    dict(semitones=4.0, fftsize=8192),
]


@pytest.mark.parametrize("kw", CASES, ids=[str(i) for i in range(len(CASES))])
def test_seeded_vs_oracle(kw):
    x = signals.voice(30000, 2, seed=77)
    want, wc, _ = O.run_offline(x, **kw)
    got, gc = E.run_offline(x, **kw)
    assert gc == wc
    assert got.shape == want.shape
    assert rms(got, want) <= RMS_TOL


@pytest.mark.parametrize("kind", ["silence", "burst", "dual", "sweep", "noise", "mono", "ch3"])
def test_edge_inputs(kind):
    if kind == "silence":
        x = np.zeros((2, 20000), np.float32)
    elif kind == "burst":
        x = signals.silence_burst(40000, 2)
    elif kind == "dual":
        x = signals.dual_mono(20000)
    elif kind == "sweep":
        x = signals.sweep(20000)
    elif kind == "noise":
        x = signals.noise(20000)
    elif kind == "mono":
        x = signals.voice(20000, 1)
    else:
        x = signals.voice(20000, 3)
    want, wc, _ = O.run_offline(x, semitones=4.0)
    got, gc = E.run_offline(x, semitones=4.0)
    assert gc == wc
    assert rms(got, want) <= RMS_TOL


def test_ragged_and_empty_calls():
    """Odd block sizes, zero-length calls, a block larger than the input ring."""
    x = signals.voice(30000, 2, seed=5)
    sizes = [1, 0, 479, 4097, 0, 13, 9000, 480, 480, 7, 0]
    pv = E.PhaseVocoder(48000, 2, 1.0, -7.0, E.NORMAL_SHIFT, E.PHASE_LOCKED, 2048)
    o = O.Oracle(2, semitones=-7.0)
    pos = 0
    g_all, w_all = [], []
    for n in sizes:
        blk = x[:, pos:pos + n]
        pos += n
        pv.processInData(blk)
        avail = o.process(blk)
        assert pv.getOutSamples() == avail
        g_all.append(pv.getOutData(avail))
        w_all.append(o.retrieve(avail))
    g, w = np.concatenate(g_all, 1), np.concatenate(w_all, 1)
    assert g.shape == w.shape and g.shape[1] > 0
    assert rms(g, w) <= RMS_TOL


def test_chunking_independence_gpu():
    """Same stream through block 64, block 4800 and the batch API: bit-identical on the GPU."""
    import torch
    x = signals.voice(24000, 2, seed=9)
    a, _ = E.run_offline(x, semitones=4.0, block=64)
    b, _ = E.run_offline(x, semitones=4.0, block=4800)
    assert bits_equal(a, b)
    bt = E.Batch(1, x.shape[1], channels=2, semitones=4.0)
    out = bt.run(torch.from_numpy(x[None]).cuda())
    torch.cuda.synchronize()
    assert bits_equal(out.cpu().numpy()[0], a)


def test_batch_streams_are_independent():
    import torch
    S, F = 5, 24000
    xs = np.stack([signals.voice(F, 2, stream=s) for s in range(S)])
    bt = E.Batch(S, F, channels=2, semitones=4.0)
    out = bt.run(torch.from_numpy(xs).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for s in (0, 3):
        want, _, _ = O.run_offline(xs[s], semitones=4.0)
        assert rms(out[s], want) <= RMS_TOL
    single, _ = E.run_offline(xs[4], semitones=4.0)
    assert bits_equal(out[4], single)


def test_identity_reconstruction_full_size():
    """Size-independent property at BASELINE size (60 s stereo): ratio-1 simple PV reconstructs its input."""
    import torch
    F = 60 * 48000
    x = signals.voice(48000, 2)
    x = np.tile(x, (1, 60))
    bt = E.Batch(1, F, channels=2, mode="time_stretch", time_ratio=1.0, coremode=0, flush=False)
    out = bt.run(torch.from_numpy(x[None]).cuda())
    torch.cuda.synchronize()
    y = out.cpu().numpy()[0]
    n = y.shape[1]
    assert n > F - 3 * 2048
    # skip the first window (window-sum ramp-in); compare the rest sample by sample
    assert rms(y[:, 4096:n], x[:, 4096:n]) <= 2e-4


def test_full_size_single_stream_vs_oracle():
    """cfg2 at full BASELINE length on one stream: 60 s stereo, +4 st, phase-locked."""
    import torch
    F = 60 * 48000
    x = np.tile(signals.voice(4 * 48000, 2), (1, 15))
    want, _, _ = O.run_offline(x, semitones=4.0)
    bt = E.Batch(1, F, channels=2, semitones=4.0)
    out = bt.run(torch.from_numpy(x[None]).cuda())
    torch.cuda.synchronize()
    y = out.cpu().numpy()[0]
    assert y.shape == want.shape
    assert rms(y, want) <= RMS_TOL
    # ... and per sample and per 256-sample window (chunk seams at scale), sized by the oracle's own noise floor for
    # this input (tests/test_parity_shape_gpu.py)
    arith = E.get_arithmetic()
    floor = oracle_floor(O.run_offline, x, arith, want=want, semitones=4.0)
    assert_shape("full-size cfg2 60 s stereo +4 st", y, want, floor, arith)


@pytest.mark.parametrize("frames", [1, 100, 479, 2047, 2048, 2049, 5000])
def test_short_inputs(frames):
    """Inputs shorter than / around one FFT frame: the flush loop of the CLI drive pads with zeros."""
    x = signals.voice(max(frames, 8), 2, seed=21)[:, :frames]
    want, wc, _ = O.run_offline(x, semitones=4.0)
    got, gc = E.run_offline(x, semitones=4.0)
    assert gc == wc and got.shape == want.shape == (2, frames)
    assert rms(got, want) <= RMS_TOL
    import torch
    bt = E.Batch(2, frames, channels=2, semitones=4.0)
    out = bt.run(torch.from_numpy(np.stack([x, x])).cuda())
    torch.cuda.synchronize()
    assert bits_equal(out.cpu().numpy()[0], got)


def test_many_channels_and_big_block():
    x = signals.voice(30000, 6, seed=8)
    want, wc, _ = O.run_offline(x, semitones=-4.0, block=7000)
    got, gc = E.run_offline(x, semitones=-4.0, block=7000)
    assert gc == wc
    assert rms(got, want) <= RMS_TOL


def test_coremode0_and_2_batch_full_chunking():
    """coremode 0 (per-bin kernel) and 2 across several launches of the batch engine."""
    import torch
    x = signals.voice(6 * 48000, 2, seed=12)
    for cm in (0, 2):
        want, _, _ = O.run_offline(x, semitones=4.0, coremode=cm)
        bt = E.Batch(1, x.shape[1], channels=2, semitones=4.0, coremode=cm)
        out = bt.run(torch.from_numpy(x[None]).cuda())
        torch.cuda.synchronize()
        assert rms(out.cpu().numpy()[0], want) <= RMS_TOL


def test_streaming_long_run_state_carry():
    """Many small calls: per-row phase state is carried across hundreds of launches."""
    x = signals.voice(4 * 48000, 2, seed=31)
    want, wc, _ = O.run_offline(x, semitones=7.0, mode="gender_change", block=256)
    got, gc = E.run_offline(x, semitones=7.0, mode="gender_change", block=256)
    assert gc == wc
    assert rms(got, want) <= RMS_TOL


@pytest.mark.parametrize("frames", [30001, 30002, 30003])
def test_batch_rows_at_unaligned_offsets(frames):
    """Batch rows start (stream * channels + channel) * frames floats into the buffer: with frames not a multiple
    of four the analysis kernel's aligned 16-byte frame loads begin in the previous row's tail and every
    sub-alignment of the pre-delayed window copies is exercised."""
    import torch
    x = np.stack([signals.voice(frames, 2, seed=40 + s) for s in range(3)])
    b = E.Batch(3, frames, channels=2, semitones=4.0)
    out = b.run(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    b.close()
    for s in range(3):
        want, _, _ = O.run_offline(x[s], semitones=4.0)
        assert out[s].shape == want.shape
        assert rms(out[s], want) <= RMS_TOL


def test_pipelined_batch_path_is_bit_identical_to_the_plain_one():
    """pv_batch_run keeps two chunks in flight in phase-locked mode (rotation chain on a second stream); with
    AUDIOMOD_PV_PIPELINE=0 it runs chunk after chunk on one stream.  Same kernels, same data: identical bits.
    Small chunks so that many of them are in the pipeline."""
    import hashlib
    import subprocess
    import sys
    code = """
import hashlib, numpy as np, sys, torch
sys.path.insert(0, %r)
from audiomod_amd import engine as E, signals
x = np.stack([signals.voice(60000, 2, seed=70 + s) for s in range(3)])
b = E.Batch(3, 60000, channels=2, semitones=4.0)
out = b.run(torch.from_numpy(x).cuda())
torch.cuda.synchronize()
print("PIPELINED", int(b.pipelined), "LAUNCHES", b.launches, "SHA", hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest())
""" % (ROOT,)
    res = {}
    for pipe in ("1", "0"):
        env = dict(os.environ, AUDIOMOD_PV_PIPELINE=pipe, AUDIOMOD_PV_CHUNK_SLICES="8")
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        f = r.stdout.split()
        res[pipe] = (int(f[1]), int(f[3]), f[5])
    assert res["1"][0] == 1 and res["0"][0] == 0
    assert res["1"][1] == res["0"][1] and res["1"][1] > 10
    assert res["1"][2] == res["0"][2]


def test_single_launch_streaming_kernel():
    """The opt-in one-launch-per-call kernel of the streaming path (AUDIOMOD_PV_STREAM_LAUNCHES=single; read once
    per process, hence the child process) must give the same results as one launch per stage."""
    import subprocess
    import sys
    code = """
import numpy as np, sys
sys.path.insert(0, %r)
from audiomod_amd import engine as E, signals
from oracle import oracle_py as O
x = signals.voice(40000, 2, seed=5)
for kw in (dict(semitones=4.0), dict(semitones=-7.0, mode="formant_pitchshift"), dict(semitones=3.0, coremode=0),
           dict(mode="time_stretch", time_ratio=1.5, fftsize=4096, flush=False), dict(mode="robotic"),
           dict(mode="formant_cepstral", semitones=5.0)):
    want, wc, _ = O.run_offline(x, **kw)
    got, gc = E.run_offline(x, **kw)
    assert gc == wc, kw
    e = float(np.sqrt(np.mean((got.astype(np.float64) - want) ** 2)))
    assert e <= 1e-4, (kw, e)
print("single-launch ok")
""" % (ROOT,)
    env = dict(os.environ, AUDIOMOD_PV_STREAM_LAUNCHES="single")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "single-launch ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("kw", [dict(mode="constant"), dict(mode="constant", fftsize=4096), dict(mode="whisper"),
                                dict(mode="whisper", fftsize=1024)], ids=["const", "const4096", "whisper", "whisper1024"])
def test_constant_and_whisper_modes(kw):
    """SURVEY 8f-2 modes.  CONSTANT passes the analysis phase through; WHISPER uses the rand() sequence of a
    fresh reference process, drawn by the host planner."""
    import torch
    x = signals.voice(30000, 2, seed=41)
    want, wc, _ = O.run_offline(x, **kw)
    got, gc = E.run_offline(x, **kw)
    assert gc == wc and got.shape == want.shape
    assert rms(got, want) <= RMS_TOL
    bt = E.Batch(2, x.shape[1], channels=2, **kw)
    out = bt.run(torch.from_numpy(np.stack([x, x])).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert bits_equal(out[0], got) and bits_equal(out[1], got)


def test_constant_realtime_api():
    x = signals.voice(20000, 2, seed=42)
    want, wc = O.run_realtime(x, mode="constant")
    got, gc = E.run_realtime(x, mode="constant")
    assert gc == wc
    assert rms(got, want) <= RMS_TOL


@pytest.mark.parametrize("kw", [dict(mode="vocoder"), dict(mode="vocoder_chord"), dict(mode="vocoder", fftsize=4096),
                                dict(mode="vocoder_chord", fftsize=1024, sample_rate=44100)],
                         ids=["rosenberg", "chord", "rosenberg4096", "chord1024"])
def test_channel_vocoder_modes(kw):
    """Rosenberg / chord carrier shaped by the band magnitudes of the input."""
    import torch
    x = signals.voice(30000, 2, seed=43)
    want, wc, _ = O.run_offline(x, **kw)
    got, gc = E.run_offline(x, **kw)
    assert gc == wc and got.shape == want.shape
    assert rms(got, want) <= RMS_TOL
    bt = E.Batch(2, x.shape[1], channels=2, **kw)
    out = bt.run(torch.from_numpy(np.stack([x, x])).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert bits_equal(out[0], got) and bits_equal(out[1], got)


def test_vocoder_realtime_api():
    x = signals.voice(20000, 1, seed=44)
    want, wc = O.run_realtime(x, mode="vocoder")
    got, gc = E.run_realtime(x, mode="vocoder")
    assert gc == wc
    assert rms(got, want) <= RMS_TOL


FULL = [
    ("cfg3", dict(mode="time_stretch", time_ratio=1.5, coremode=1, fftsize=4096, flush=False)),
    ("cfg4_formant+7", dict(mode="formant_pitchshift", semitones=7.0, coremode=1, fftsize=2048)),
    ("cfg4_gender-7", dict(mode="gender_change", semitones=-7.0, coremode=1, fftsize=2048)),
]


@pytest.mark.parametrize("name,kw", FULL, ids=[n for n, _ in FULL])
def test_full_size_other_baseline_configs(name, kw):
    """BASELINE configs[2] and configs[3] at full length (60 s stereo) on one stream of a 2-stream batch."""
    import torch
    F = 60 * 48000
    x = np.tile(signals.voice(4 * 48000, 2, seed=17), (1, 15))
    kw = dict(kw)
    flush = kw.pop("flush", True)
    want, _, _ = O.run_offline(x, flush=flush, **kw)
    bt = E.Batch(2, F, channels=2, flush=flush, **kw)
    out = bt.run(torch.from_numpy(np.stack([x, x])).cuda())
    torch.cuda.synchronize()
    y = out.cpu().numpy()
    assert y[0].shape == want.shape
    assert rms(y[0], want) <= RMS_TOL
    assert bits_equal(y[0], y[1])


@pytest.mark.parametrize("kw", [dict(semitones=4.0), dict(semitones=-7.0), dict(semitones=7.0, fftsize=4096),
                                dict(semitones=4.0, coremode=0), dict(semitones=0.0),
                                dict(semitones=5.0, fftsize=1024), dict(semitones=-4.0, fftsize=512),
                                dict(semitones=3.0, fftsize=8192, coremode=2), dict(semitones=-9.0, fftsize=256)])
def test_formant_cepstral_mode(kw):
    """extension mode: the reference's (unreachable) cepstral formant shift, oracle pinned on the real function; every
    FFT size (2048 / 4096: one wave per slice; the others, since round 2: one workgroup per slice through the generic
    LDS transforms -- formantShiftSlice itself is size-agnostic)"""
    x = signals.voice(30000, 2, seed=91)
    want, wc, _ = O.run_offline(x, mode="formant_cepstral", **kw)
    got, gc = E.run_offline(x, mode="formant_cepstral", **kw)
    assert gc == wc
    assert rms(got, want) <= RMS_TOL
    if kw.get("semitones"):
        plain, _, _ = O.run_offline(x, mode="normal_pitchshift", **kw)
        assert rms(want, plain) > 20 * RMS_TOL  # the mode really does something
    # and through the batch API
    import torch
    b = E.Batch(2, x.shape[1], channels=2, mode="formant_cepstral", **kw)
    out = b.run(torch.from_numpy(np.stack([x, x])).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert rms(out[0], want) <= RMS_TOL and bits_equal(out[0], out[1])
    b.close()


def test_formant_cepstral_needs_room_for_its_lifter():
    """the lifter keeps 60 quefrencies: frames below 128 points are refused (every larger size is served)"""
    with pytest.raises(E.PvError):
        E.PhaseVocoder(48000, 2, 1.0, 4.0, E.FORMANT_CEPSTRAL, 1, 64)


# Configurations the randomised sweep (tests/sweeps/fuzz_parity.py) turned up as refused or wrong at some point.
SWEEP_FINDS = [
    # per-call output above the streaming staging buffer: fixed-hop modes through a > 2x up-sampling resampler
    (dict(mode="robotic", fftsize=1024, sample_rate=16000, semitones=-15.8), 2, 887, 4724, True),
    (dict(mode="constant", fftsize=512, semitones=-14.53), 3, 5105, 1650, True),
    (dict(mode="vocoder_chord", fftsize=1024, semitones=-13.0), 2, 12000, 4800, True),
    # many frames under one overlap-add tile: small FFT, large pitch scale / small ratio, automatic hop
    (dict(fftsize=256, semitones=15.558), 2, 20000, 480, True),
    (dict(mode="time_stretch", fftsize=256, time_ratio=0.374, coremode=0, sample_rate=96000), 1, 9000, 64, False),
    (dict(mode="constant", fftsize=256, semitones=14.65, sample_rate=16000), 3, 4000, 480, True),
    # the reference's Rosenberg carrier is NaN below ~22 kHz (zero-length opening phase, rosenberg.cc:19-53)
    (dict(mode="vocoder", fftsize=2048, sample_rate=16000, semitones=-6.0), 2, 6000, 480, True),
    (dict(mode="vocoder_chord", fftsize=512, sample_rate=22050, semitones=8.0), 2, 9000, 4800, True),
]


@pytest.mark.parametrize("kw,ch,frames,block,flush", SWEEP_FINDS, ids=[str(i) for i in range(len(SWEEP_FINDS))])
def test_sweep_finds(kw, ch, frames, block, flush):
    import torch
    x = signals.voice(frames, ch, seed=31)
    want, wc, _ = O.run_offline(x, block=block, flush=flush, **kw)
    got, gc = E.run_offline(x, block=block, flush=flush, **kw)
    assert list(gc) == list(wc) and got.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)  # non-finite exactly where the reference is
    assert rms(got[fin], want[fin]) <= RMS_TOL if fin.any() else True
    b = E.Batch(2, frames, channels=ch, block=block, flush=flush, **kw)
    out = b.run(torch.from_numpy(np.stack([x, x])).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    b.close()
    assert out.shape[2] == want.shape[1]
    for s_ in range(2):
        assert np.array_equal(np.isfinite(out[s_]), fin)
        assert rms(out[s_][fin], want[fin]) <= RMS_TOL if fin.any() else True


def test_process_block_ignores_time_stretch():
    """processBlock has no branch for NORMAL_STRETCH (phasevocoder.cc:126-152): buffer untouched, always ready."""
    x = signals.voice(5000, 2, seed=5)
    got, cnt = E.run_realtime(x, block=480, mode="time_stretch", time_ratio=1.5)
    want, wc = O.run_realtime(x, block=480, mode="time_stretch", time_ratio=1.5)
    assert cnt == wc == [480] * 10 + [200]
    assert bits_equal(got, x) and bits_equal(want, x)


def test_synthesis_specialisation_is_bit_identical_to_the_generic_kernel():
    """The plain pitch-shift / stretch cases (any core mode) run specialisations of the synthesis kernel (mode
    switches folded at compile time); AUDIOMOD_PV_SYNTH_GENERIC=1 (read once per process, hence the child) sends it through the all-modes
    kernel instead.  Same arithmetic: the outputs must agree bit for bit, at 2048 and 4096 points."""
    import subprocess
    import sys
    code = """
import numpy as np, sys, torch
sys.path.insert(0, %r)
from audiomod_amd import engine as E, signals
x = np.stack([signals.voice(30000, 2, seed=11 + s) for s in range(3)])
outs = []
for kw in (dict(semitones=4.0), dict(mode="time_stretch", time_ratio=1.5, fftsize=4096, flush=False),
           dict(semitones=-3.0, coremode=0), dict(semitones=12.0, coremode=2), dict(semitones=5.0, coremode=0, fftsize=4096)):
    b = E.Batch(3, 30000, channels=2, **kw)
    o = b.run(torch.from_numpy(x).cuda()); torch.cuda.synchronize()
    outs.append(o.cpu().numpy()); b.close()
    g, _ = E.run_offline(x[0], **kw)
    outs.append(g)
np.savez(sys.argv[1], *outs)
""" % (ROOT,)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        files = []
        # (AUDIOMOD_PV_EXACT=1: only the specialisations have a free-form twin; this test is about the exact kernels)
        for tag, env in (("spec", {"AUDIOMOD_PV_EXACT": "1"}),
                         ("generic", {"AUDIOMOD_PV_SYNTH_GENERIC": "1", "AUDIOMOD_PV_EXACT": "1"})):
            f = os.path.join(d, tag + ".npz")
            r = subprocess.run([sys.executable, "-c", code, f], capture_output=True, text=True,
                               env=dict(os.environ, **env), timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            files.append(np.load(f))
        a, b = files
        assert len(a.files) == len(b.files) == 10
        for k in a.files:
            assert bits_equal(a[k], b[k]), k


def test_randomised_sweep_slice():
    """120 configurations of tests/sweeps/fuzz_parity.py (seed 7): streaming API, batch API on every second case and the
    processBlock loop on every third, against the oracle.  The full sweeps are in profiles/r01."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sweeps", "fuzz_parity.py"), "120", "7", "300"],
                       capture_output=True, text=True, timeout=900)
    tail = "\n".join(line for line in r.stdout.splitlines() if not line.startswith("#"))[-2000:]
    assert r.returncode == 0, tail
    assert " 0 failed" in r.stdout, tail


def test_batch_with_no_output_at_all():
    """Shorter than one FFT frame and no flush (the time_stretch rule, main.cc:471-478): zero output frames is a
    valid job, not an argument error."""
    import torch
    b = E.Batch(2, 1482, channels=2, flush=False, semitones=7.04, fftsize=8192)
    assert b.out_frames == 0
    out = b.run(torch.zeros(2, 2, 1482, device="cuda"))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 2, 0)
    b.close()


def test_invalid_modes_fail_loudly():
    for mode in (9, 42, -2):
        with pytest.raises(E.PvError):
            E.PhaseVocoder(48000, 2, 1.0, 0.0, mode)


def test_fused_overlap_add_is_bit_identical_to_the_tile_path():
    """The default path adds the synthesis frames into the reference's accumulator in LDS, in slice order (fused
    synthesis + overlap-add, pv_synth_chain_kernel / pv_frames_chain_kernel); AUDIOMOD_PV_FUSED=0 (read at engine
    creation) writes them to the HBM frame ring and gathers them per output tile.  Same additions in the same
    order, same resampler arithmetic: the outputs must agree bit for bit -- batch and streaming, every FFT size
    class (wave-per-frame 2048 / 4096, generic 512 / 8192), resampling up, down and not at all."""
    import subprocess
    import sys
    import tempfile
    code = """
import numpy as np, sys, torch
sys.path.insert(0, %r)
from audiomod_amd import engine as E, signals
x = np.stack([signals.voice(40000, 2, seed=23 + s) for s in range(3)])
outs = []
for kw in (dict(semitones=4.0), dict(semitones=-7.0, mode="formant_pitchshift"),
           dict(mode="time_stretch", time_ratio=1.5, fftsize=4096, flush=False), dict(semitones=7.0, fftsize=4096, coremode=0),
           dict(semitones=3.0, fftsize=512), dict(semitones=-5.0, fftsize=8192, coremode=2), dict(mode="robotic", fftsize=1024),
           dict(semitones=12.0), dict(mode="time_stretch", time_ratio=0.6, flush=False, coremode=0),
           dict(mode="vocoder"), dict(mode="constant", semitones=-4.0)):
    kw = dict(kw); flush = kw.pop("flush", True)
    b = E.Batch(3, 40000, channels=2, flush=flush, **kw)
    xin = torch.from_numpy(x).cuda()
    o = b.run(xin, d_out=torch.full((3, 2, b.out_frames), float("nan"), device="cuda"))  # an unwritten sample shows
    torch.cuda.synchronize()
    outs.append(o.cpu().numpy()); b.close()
    g, _ = E.run_offline(x[1], flush=flush, block=777, **kw)
    outs.append(g)
np.savez(sys.argv[1], *outs)
""" % (ROOT,)
    def both_paths(d):
        files = []
        # (AUDIOMOD_PV_EXACT=1: the batch engine's default arithmetic regroups the synthesis side's sums on the fused
        # path -- this test is about the exact variant's order of additions)
        for tag, env in (("fused", {"AUDIOMOD_PV_FUSED": "2", "AUDIOMOD_PV_EXACT": "1"}),
                         ("tiles", {"AUDIOMOD_PV_FUSED": "0", "AUDIOMOD_PV_EXACT": "1"})):
            f = os.path.join(d, f"{tag}.npz")
            r = subprocess.run([sys.executable, "-c", code, f], capture_output=True, text=True,
                               env=dict(os.environ, **env), timeout=900)
            assert r.returncode == 0, r.stdout + r.stderr
            files.append(np.load(f))
        return files

    def mismatches(a, b):
        bad = [k for k in a.files if not bits_equal(a[k], b[k])]
        bad += [f"row-vs-stream {i}" for i in range(0, 22, 2) if not bits_equal(a[f"arr_{i}"][1], a[f"arr_{i + 1}"])]
        return bad

    with tempfile.TemporaryDirectory() as d:
        a, b = both_paths(d)
        assert len(a.files) == len(b.files) == 22
        bad = mismatches(a, b)
        if bad:
            # Keep what differed where it survives the run (gpurun merges gpurun_out/ back): both arrays of every
            # differing pair and the positions -- round 2 lost three occurrences of a rare mismatch to a temp directory.
            keep = os.path.join(ROOT, "gpurun_out", "fused_vs_tiles_mismatch")
            os.makedirs(keep, exist_ok=True)
            where = {}
            for k in bad:
                if k.startswith("arr_"):
                    m = np.argwhere(a[k].view(np.uint32) != b[k].view(np.uint32))
                    where[k] = (len(m), m[:8].tolist(), [(float(a[k][tuple(i)]), float(b[k][tuple(i)])) for i in m[:8]])
                    np.savez(os.path.join(keep, k + ".npz"), fused=a[k], tiles=b[k], positions=m)
            with open(os.path.join(keep, "where.txt"), "w") as fh:
                fh.write(repr((bad, where)))
            pytest.fail(f"fused and tile path differ: {bad} {where}")


def test_short_square_root_is_correctly_rounded_on_every_float_of_its_range():
    """pv_sqrt_safe (pv_atan2f.h: rsq, one multiply, an exact residual, one fma) against the compiler's correctly rounded
    sqrtf on EVERY float in [2^-96, 2^127) -- the range the analysis kernels' fast path guarantees for re^2 + im^2."""
    import ctypes as C
    lo = int(np.float32(2.0 ** -96).view(np.uint32))
    hi = int(np.float32(2.0 ** 127).view(np.uint32))
    bad, first = C.c_uint64(0), C.c_uint32(0)
    E._check(E.lib().pv_debug_sqrt_sweep(lo, hi - lo, C.byref(bad), C.byref(first), 0), "pv_debug_sqrt_sweep")
    assert bad.value == 0, (bad.value, hex(first.value))


OVERRUN_GPU = [
    (dict(semitones=-3.0), 2, [100000, 480, 480, 50000, 480, 480]),
    (dict(semitones=5.0, fftsize=256), 2, [6000, 6000, 64, 6000]),
    (dict(mode="constant", fftsize=256), 3, [4800, 4800, 64, 9000, 480]),
    (dict(mode="vocoder", fftsize=512), 1, [9000, 480, 9000]),
    (dict(mode="time_stretch", time_ratio=2.5, fftsize=512, coremode=0), 2, [12000, 100, 12000]),
    (dict(mode="robotic", fftsize=1024, semitones=-9.0), 2, [40000, 480]),
    (dict(semitones=4.0, fftsize=4096, coremode=2), 2, [130000, 3000]),
]


@pytest.mark.parametrize("kw,ch,calls", OVERRUN_GPU, ids=[str(i) for i in range(len(OVERRUN_GPU))])
def test_output_overrun_drops_slices_like_the_reference(kw, ch, calls):
    """Calls so large that the reference's own output ring overruns: it drops slices there (frame added to the
    accumulators, writeSlice skipped: phasevocoderprocess.cc:337-364; the CONSTANT loop even leaves after channel
    0, :139-150), so the following frames pile up on one overlap-add position.  The engine reproduces that -- same
    per-call counts, same audio -- instead of refusing the call."""
    x = signals.voice(sum(calls), ch, seed=55)
    pv = E.PhaseVocoder(kw.get("sample_rate", 48000), ch, kw.get("time_ratio", 1.0), kw.get("semitones", 0.0),
                        E.MODES[kw.get("mode", "normal_pitchshift")], kw.get("coremode", 1), kw.get("fftsize", 2048))
    o = O.Oracle(ch, **kw)
    pos, g_all, w_all, dropped = 0, [], [], False
    for n in calls:
        blk = x[:, pos:pos + n]
        pos += n
        pv.processInData(blk)
        avail = o.process(blk)
        assert pv.getOutSamples() == avail
        dropped = dropped or avail >= o.info()["outbuf_capacity"] - 2 * o.info()["fftsize"]
        g_all.append(pv.getOutData(avail))
        w_all.append(o.retrieve(avail))
    assert dropped  # the case really drives the ring full
    g, w = np.concatenate(g_all, 1), np.concatenate(w_all, 1)
    assert g.shape == w.shape and g.shape[1] > 0
    assert rms(g, w) <= RMS_TOL
    pv.close()


def test_feed_is_transactional_and_retrieve_is_bounded():
    """A call the engine refuses leaves it where it was (nothing fed, nothing pending): the caller goes on with
    valid calls and gets exactly the reference's output for those.  The refusal used here: the tile path
    (AUDIOMOD_PV_FUSED=0) cannot represent dropped slices and rejects a call that overruns the output ring."""
    import subprocess
    import sys
    code = """
import numpy as np, sys
sys.path.insert(0, %r)
from audiomod_amd import engine as E, signals
from oracle import oracle_py as O
x = signals.voice(20000, 2, seed=61)
pv = E.PhaseVocoder(48000, 2, 1.0, 4.0)
try:
    pv.processInData(np.zeros((2, 200000), np.float32))
    raise SystemExit("the overrunning call was not refused")
except E.PvError as ex:
    assert "output ring" in str(ex), ex
assert pv.L.pv_available(pv.h) == 0
got, gc = [], []
for i in range(0, 20000, 480):
    pv.processInData(x[:, i:i + 480])
    n = pv.getOutSamples()
    gc.append(n)
    got.append(pv.getOutData(n))
out = np.zeros((2, 64), np.float32)
assert pv.L.pv_retrieve(pv.h, E._pp([out[0], out[1]]), 64) == 0   # nothing left: nothing handed out
want, wc, _ = O.run_offline(x, semitones=4.0, flush=False)
assert gc == wc, (gc[:8], wc[:8])
e = float(np.sqrt(np.mean((np.concatenate(got, 1).astype(np.float64) - want) ** 2)))
assert e <= 1e-4, e
print("transactional ok")
""" % (ROOT,)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       env=dict(os.environ, AUDIOMOD_PV_FUSED="0"), timeout=600)
    assert r.returncode == 0 and "transactional ok" in r.stdout, r.stdout + r.stderr


def test_device_atan2f_is_libms_bit_for_bit():
    """The analysis kernels' atan2f as the DEVICE computes it (its own short division, pv_atan2f.h) against the C
    library's on the box: spectrum-like magnitudes, random finite bit patterns, every reduction threshold, zeros and
    signed zeros.  (The host build of the same header is swept in tests/test_native_host.py.)"""
    import ctypes as C
    rng = np.random.default_rng(2024)
    n = 6_000_000
    parts_y, parts_x = [], []
    e = rng.uniform(-8, 3, (2, n)).astype(np.float32)
    sg = rng.choice(np.array([-1.0, 1.0], np.float32), (2, n))
    parts_y.append((10.0 ** e[0]).astype(np.float32) * sg[0])
    parts_x.append((10.0 ** e[1]).astype(np.float32) * sg[1])
    bits = rng.integers(0, 2 ** 32, (2, n), dtype=np.uint64).astype(np.uint32)
    fy, fx = bits[0].view(np.float32), bits[1].view(np.float32)
    fin = np.isfinite(fy) & np.isfinite(fx)
    parts_y.append(fy[fin])
    parts_x.append(fx[fin])
    for t in (0.4375, 0.6875, 1.1875, 2.4375, 1.0, 3.7e-9, 3.3554432e7):
        r = (np.float32(t).view(np.uint32) + np.arange(-20000, 20001, dtype=np.int64)).astype(np.uint32).view(np.float32)
        for xv in (1.0, 0.37, 123.456, -0.37, -5e-3):
            parts_y += [r * np.float32(xv), -r * np.float32(xv)]
            parts_x += [np.full_like(r, xv), np.full_like(r, xv)]
    z = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 3.4e38, -3.4e38, 1e-30, 1e30], np.float32)
    parts_y.append(np.repeat(z, len(z)))
    parts_x.append(np.tile(z, len(z)))
    y = np.ascontiguousarray(np.concatenate(parts_y), np.float32)
    x = np.ascontiguousarray(np.concatenate(parts_x), np.float32)
    got, want = np.zeros_like(y), np.zeros_like(y)
    E._check(E.lib().pv_debug_atan2f(y.ctypes.data, x.ctypes.data, got.ctypes.data, len(y), 0), "pv_debug_atan2f")
    L = O.lib()
    L.pvo_atan2f_array.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long]
    L.pvo_atan2f_array(y.ctypes.data, x.ctypes.data, want.ctypes.data, len(y))
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, y[bad[:5]], x[bad[:5]], got[bad[:5]], want[bad[:5]])
    # the wave-per-frame kernels' polar conversion (table-driven atan2f; short division and square root where the
    # operands' range allows): phases against libm again, magnitudes against the correctly rounded sqrtf of the
    # separately rounded re^2 + im^2 (FFT.cc:2623-2630 as the reference's x86 build evaluates it)
    ew = rng.uniform(-14.4, 18.9, (2, n)).astype(np.float32)  # the whole range the fast path accepts, and beyond
    sgw = rng.choice(np.array([-1.0, 1.0], np.float32), (2, n))
    y = np.ascontiguousarray(np.concatenate([y, (10.0 ** ew[0]).astype(np.float32) * sgw[0]]), np.float32)
    x = np.ascontiguousarray(np.concatenate([x, (10.0 ** ew[1]).astype(np.float32) * sgw[1]]), np.float32)
    ph, mg, want = np.zeros_like(y), np.zeros_like(y), np.zeros_like(y)
    E._check(E.lib().pv_debug_polar(y.ctypes.data, x.ctypes.data, ph.ctypes.data, mg.ctypes.data, len(y), 0),
             "pv_debug_polar")
    L.pvo_atan2f_array(y.ctypes.data, x.ctypes.data, want.ctypes.data, len(y))
    bad = np.nonzero(ph.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, y[bad[:5]], x[bad[:5]], ph[bad[:5]], want[bad[:5]])
    with np.errstate(over="ignore", under="ignore"):
        wm = np.sqrt((x * x).astype(np.float32) + (y * y).astype(np.float32), dtype=np.float32)
    bad = np.nonzero(mg.view(np.uint32) != wm.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, y[bad[:5]], x[bad[:5]], mg[bad[:5]], wm[bad[:5]])


FAST_CASES = [dict(semitones=4.0), dict(semitones=-7.0, mode="formant_pitchshift"), dict(semitones=12.0),
              dict(semitones=7.0, mode="gender_change"), dict(mode="time_stretch", time_ratio=1.5, fftsize=4096, flush=False)]


@pytest.mark.parametrize("kw", FAST_CASES, ids=[str(i) for i in range(len(FAST_CASES))])
def test_fast_arithmetic_of_the_batch_path_stays_within_the_contract(kw):
    """PV_ARITH_FAST (the batch engine's default, include/audiomod_pv.h) lets the fused many-stream path -- 192 rows and
    up -- fuse multiply-adds and regroup sums behind the phase propagation.  Both settings against the oracle on a
    batch large enough to take that path (every stream its own signal): fast within the 1e-4 RMS contract -- and, as
    measured, within 1e-6 -- exact as before; the two differ by rounding only."""
    import torch
    kw = dict(kw)
    flush = kw.pop("flush", True)
    S, F = 96, 16000
    x = np.stack([signals.voice(F, 2, stream=s) for s in range(S)])
    d_in = torch.from_numpy(x).cuda()
    outs = {}
    prev = E.get_arithmetic()
    try:
        for arith in (E.ARITH_FAST, E.ARITH_EXACT):
            E.set_arithmetic(arith)
            b = E.Batch(S, F, channels=2, flush=flush, **kw)
            o = b.run(d_in)
            torch.cuda.synchronize()
            outs[arith] = o.cpu().numpy()
            b.close()
    finally:
        E.set_arithmetic(prev)
    for s in (0, 37, 95):
        want, _, _ = O.run_offline(x[s], flush=flush, **kw)
        assert outs[E.ARITH_EXACT][s].shape == want.shape
        assert rms(outs[E.ARITH_EXACT][s], want) <= RMS_TOL
        r = rms(outs[E.ARITH_FAST][s], want)
        assert r <= 1e-6, r
    assert rms(outs[E.ARITH_FAST], outs[E.ARITH_EXACT]) <= 1e-6


FFT1024 = [dict(semitones=4.0), dict(semitones=2.0, coremode=0), dict(semitones=2.0, coremode=2),
           dict(mode="time_stretch", time_ratio=1.5, flush=False), dict(mode="formant_pitchshift", semitones=5.0),
           dict(mode="robotic"), dict(mode="whisper"), dict(mode="vocoder"), dict(mode="formant_cepstral", semitones=3.0)]


@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("fftsize", [512, 1024])
@pytest.mark.parametrize("kw", FFT1024, ids=[str(i) for i in range(len(FFT1024))])
def test_fft512_and_1024_run_through_the_wave_per_frame_kernels(kw, fftsize, arith):
    """Round 3: 1024- and 512-point frames (512 / 256 complex points, kissfft stages 2 4 4 4 4 / 4 4 4 4) have a
    wave-per-frame transform too -- four passes of eight / four elements per lane (pv_wavefft.h WF<512>, WF<256>; the
    core is checked bit for bit on the host, tests/native/host_wavefft.cc) -- and with it the fused overlap-add path
    and, for the plain modes, the free-form kernels.  Streaming and batch API against the oracle under both arithmetic
    settings; ROBOTIC bit for bit; the batch equal to the stream bit for bit."""
    import torch
    kw = dict(kw, fftsize=fftsize)
    flush = kw.pop("flush", True)
    x = signals.voice(30000, 2, seed=77)
    prev = E.get_arithmetic()
    try:
        E.set_arithmetic(E.ARITH_FAST if arith == "fast" else E.ARITH_EXACT)
        want, wc, _ = O.run_offline(x, flush=flush, **kw)
        got, gc = E.run_offline(x, flush=flush, **kw)
        S = 5
        b = E.Batch(S, x.shape[1], channels=2, flush=flush, **kw)
        o = b.run(torch.from_numpy(np.stack([x] * S)).cuda())
        torch.cuda.synchronize()
        o = o.cpu().numpy()
        b.close()
    finally:
        E.set_arithmetic(prev)
    assert gc == wc and got.shape == want.shape
    assert rms(got, want) <= RMS_TOL and rms(o[S - 1], want) <= RMS_TOL
    assert bits_equal(o[0], got) and bits_equal(o[S - 1], got)
    if kw.get("mode") == "robotic":
        assert bits_equal(got, want.astype(np.float32))


FFT4096 = [dict(mode="time_stretch", time_ratio=1.5, flush=False), dict(semitones=4.0), dict(semitones=-3.0, coremode=0),
           dict(mode="formant_pitchshift", semitones=5.0), dict(mode="robotic")]


@pytest.mark.parametrize("kw", FFT4096, ids=[str(i) for i in range(len(FFT4096))])
def test_fft4096_analysis_on_two_waves_equals_the_one_wave_kernel_bit_for_bit(kw, monkeypatch):
    """Round 3: the analysis kernel of 4096-point frames runs a frame on TWO waves (pv_analyze_split_kernel, pv_wavefft.h
    WF2048S: 128 lanes x 16 elements; the spec is checked bit for bit on the host, tests/native/host_wavefft.cc).  Same
    arithmetic in the same order, so under PV_ARITH_EXACT the whole output -- streaming API, with its short first and last
    calls, and a batch whose last frames run past the input's end (the edge path of the frame load) -- is bit-identical
    to the one-wave kernel's (AUDIOMOD_PV_SPLIT_ANALYSIS=0), and within the contract of the oracle."""
    import torch
    kw = dict(kw, fftsize=4096)
    flush = kw.pop("flush", True)
    x = signals.voice(41000, 2, seed=91)
    prev = E.get_arithmetic()
    outs = {}
    try:
        E.set_arithmetic(E.ARITH_EXACT)
        for split in ("0", "1"):
            monkeypatch.setenv("AUDIOMOD_PV_SPLIT_ANALYSIS", split)   # read when an engine is created
            got, gc = E.run_offline(x, flush=flush, **kw)
            S = 3
            b = E.Batch(S, x.shape[1], channels=2, flush=flush, **kw)
            o = b.run(torch.from_numpy(np.stack([x] * S)).cuda())
            torch.cuda.synchronize()
            outs[split] = (got, gc, o.cpu().numpy())
            b.close()
    finally:
        E.set_arithmetic(prev)
    want, wc, _ = O.run_offline(x, flush=flush, **kw)
    (g0, c0, b0), (g1, c1, b1) = outs["0"], outs["1"]
    assert c0 == c1 == wc and g0.shape == g1.shape == want.shape
    assert bits_equal(g0, g1) and bits_equal(b0, b1)
    assert rms(g1, want) <= RMS_TOL and rms(b1[2], want) <= RMS_TOL
