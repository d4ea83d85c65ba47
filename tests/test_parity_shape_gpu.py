"""Error-shape tier: the GPU path against the oracle per sample and per window of one resampler tile, next to the
whole-output RMS <= 1e-4 contract, which is an average and three to four orders looser than the code.

The bar (tests/helpers.py): for the largest absolute error and for the worst RMS over any 256-sample window of one
channel, metric(got, want) <= 8 * floor + 4 ulp(peak(want)).  The floor comes from the reference alone: the oracle run
on the very input and configuration under test with every synthesis sine / cosine nudged by +-delta (random signs),
against the plain oracle; delta is the documented error of the sine / cosine in use (4.8e-7 for
PV_ARITH_FAST's v_sin_f32 / v_cos_f32, 1.2e-7 = 1.5 ulp for pv_sincos.h under PV_ARITH_EXACT).  The case lists are
those of tests/test_gpu_parity.py; the old assertions stay where they are."""
import numpy as np
import pytest

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import assert_shape, oracle_floor, parity_shape
from tests.test_gpu_parity import CASES, FAST_CASES, FFT1024, RMS_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[E.ARITH_FAST, E.ARITH_EXACT], ids=["fast", "exact"])
def arith(request):
    prev = E.set_arithmetic(request.param)
    yield request.param
    E.set_arithmetic(prev)


def stream_case(label, x, arith, **kw):
    kw = dict(kw)
    flush = kw.pop("flush", True)
    want, wc, info = O.run_offline(x, flush=flush, **kw)
    floor = oracle_floor(O.run_offline, x, arith, want=want, flush=flush, **kw)
    got, gc = E.run_offline(x, flush=flush, **kw)
    assert list(gc) == list(wc) and got.shape == want.shape
    assert parity_shape(got, want)["rms"] <= RMS_TOL
    assert_shape(label, got, want, floor, arith)
    return info


@pytest.mark.parametrize("i", range(len(CASES)))
def test_seeded_vs_oracle(i, arith):
    stream_case(f"seeded[{i}] {CASES[i]}", signals.voice(30000, 2, seed=77), arith, **CASES[i])


@pytest.mark.parametrize("kind", ["silence", "burst", "dual", "sweep", "noise", "mono", "ch3"])
def test_edge_inputs(kind, arith):
    x = {"silence": lambda: np.zeros((2, 20000), np.float32), "burst": lambda: signals.silence_burst(40000, 2),
         "dual": lambda: signals.dual_mono(20000), "sweep": lambda: signals.sweep(20000),
         "noise": lambda: signals.noise(20000), "mono": lambda: signals.voice(20000, 1),
         "ch3": lambda: signals.voice(20000, 3)}[kind]()
    stream_case(f"edge[{kind}] +4", x, arith, semitones=4.0)


@pytest.mark.parametrize("i", range(len(FAST_CASES)))
def test_96_stream_batch(i, arith):
    """The many-stream fused path with every row its own signal: the only route to the 16-row fast / matrix-core
    resampler with distinct rows.  Streams on both sides of a row-group boundary (15 | 16), the first and the last."""
    import torch
    kw = dict(FAST_CASES[i])
    flush = kw.pop("flush", True)
    S, F = 96, 16000
    x = np.stack([signals.voice(F, 2, stream=s) for s in range(S)])
    b = E.Batch(S, F, channels=2, flush=flush, **kw)
    out = b.run(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    b.close()
    for s in (0, 15, 16, 37, 95):
        want, _, _ = O.run_offline(x[s], flush=flush, **kw)
        floor = oracle_floor(O.run_offline, x[s], arith, want=want, flush=flush, **kw)
        assert parity_shape(out[s], want)["rms"] <= RMS_TOL
        assert_shape(f"batch96[{i}] {FAST_CASES[i]} stream {s}", out[s], want, floor, arith)


@pytest.mark.parametrize("fftsize", [512, 1024])
@pytest.mark.parametrize("i", range(len(FFT1024)))
def test_fft512_and_1024(i, fftsize, arith):
    stream_case(f"fft{fftsize}[{i}] {FFT1024[i]}", signals.voice(30000, 2, seed=77), arith, fftsize=fftsize, **FFT1024[i])


ROBOTIC_PITCH = [dict(semitones=4.0), dict(semitones=-7.0), dict(semitones=12.0), dict(semitones=-12.0),
                 dict(semitones=3.7), dict(semitones=4.0, fftsize=1024), dict(semitones=-7.0, fftsize=4096)]


@pytest.mark.parametrize("i", range(len(ROBOTIC_PITCH)))
def test_robotic_with_a_pitch(i, arith):
    """Phases all zero: the floor is zero and the bar is four ulps of the peak, per sample, through the resampler --
    streaming and in a batch large enough for the many-stream path (tests/test_parity_exact_gpu.py holds
    PV_ARITH_EXACT to the bit; this is the same configuration under either setting)."""
    import torch
    kw = dict(ROBOTIC_PITCH[i], mode="robotic")
    info = stream_case(f"robotic[{i}] {ROBOTIC_PITCH[i]}", signals.voice(30000, 2, seed=77), arith, **kw)
    assert info["resample"] == 1
    S, F = 96, 12000
    x = np.stack([signals.voice(F, 2, stream=s) for s in range(S)])
    b = E.Batch(S, F, channels=2, **kw)
    out = b.run(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    b.close()
    for s in (0, 15, 16, 95):
        want, _, _ = O.run_offline(x[s], **kw)
        floor = oracle_floor(O.run_offline, x[s], arith, want=want, **kw)
        assert floor["max_abs"] == 0.0
        assert_shape(f"robotic-batch96[{i}] {ROBOTIC_PITCH[i]} stream {s}", out[s], want, floor, arith)


POOL = {  # one slot per kernel variant of the mixed pool's resampler: interpolated up / down, direct table
    "plain": (dict(semitones=4.0, coremode=1, fftsize=2048), (-7.0, 3.7, 12.0)),
    "plain1024": (dict(semitones=4.0, coremode=1, fftsize=1024), (-7.0, 4.0, -12.0)),
    "formant": (dict(mode="formant_pitchshift", semitones=0.0), (-5.0, 5.0)),
    "robotic": (dict(mode="robotic", semitones=0.0), (-7.0, 4.0, 12.0)),
}


@pytest.mark.parametrize("name", list(POOL))
def test_mixed_pool_slots(name, arith):
    kw, pitches = POOL[name]
    pool = E.StreamPool(len(pitches), channels=2, pitch_range=(-12, 12), **kw)
    slots = [pool.open(semitones=p) for p in pitches]
    frames = 36000
    xs = [signals.voice(frames, 2, seed=600 + j) for j in range(len(slots))]
    got = [[] for _ in slots]
    for i in range(0, frames, 480):
        pool.feed({s: xs[j][:, i:i + 480] for j, s in enumerate(slots)})
        for j, s in enumerate(slots):
            got[j].append(pool.retrieve(s, pool.available(s)))
    pool.close_pool()
    for j, p in enumerate(pitches):
        okw = dict(kw, semitones=p)
        want, wc, _ = O.run_offline(xs[j], flush=False, **okw)
        floor = oracle_floor(O.run_offline, xs[j], arith, want=want, flush=False, **okw)
        assert [g.shape[1] for g in got[j]] == list(wc)
        g = np.concatenate(got[j], axis=1)
        assert parity_shape(g, want)["rms"] <= RMS_TOL
        assert_shape(f"mixed-pool[{name}] slot at {p:+.1f} st", g, want, floor, arith)
