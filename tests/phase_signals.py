"""Signals that put the phase-locked stage's peak lists and step patterns where the tests want them.

float32 in [-1, 1) on the int16 grid, like audiomod_amd/signals.py.  What each of them does to the oracle's per-step trace
(oracle_py.Oracle.phase_trace) is asserted in tests/test_phase_forms_host.py; tests/test_phase_forms_gpu.py runs them
through every form of the stage.
"""
import numpy as np


def _grid(x):
    return (np.clip(np.round(np.asarray(x, np.float64) * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


def comb_bins(N):
    """the bins a comb of an N-point frame sits on: 2, 5, 8, ... < N/2 - 2 -- as many as a peak list can hold"""
    return np.arange(2, N // 2 - 2, 3)


def comb(N, frames, channels=2, seed=0):
    """Cosines of equal amplitude and seeded random phase (one draw per channel) at every bin of comb_bins(N), peak 0.9.
    A Hann frame of it has a strict peak at every third bin: a full peak list, ceil((N/2 - 4) / 3) entries."""
    rng = np.random.default_rng(seed)
    bins = comb_bins(N)
    n = np.arange(N, dtype=np.int64)
    out = np.empty((channels, frames), dtype=np.float64)
    for c in range(channels):
        ph = rng.uniform(0.0, 2 * np.pi, bins.size)
        # exactly periodic in N: one period, tiled (the argument is reduced in integers)
        arg = (2 * np.pi / N) * ((bins[:, None] * n[None, :]) % N)
        period = np.cos(arg + ph[:, None]).sum(axis=0)
        x = np.tile(period, frames // N + 1)[:frames]
        out[c] = x * (0.9 / np.max(np.abs(period)))
    return _grid(out)


def comb_gaps(N, hop, frames, channels=2, seed=0, gap_channel=0, gap_len=None, starts=()):
    """comb() with exact zeros in channel `gap_channel` over [s, s + gap_len) for every s in `starts`.  A gap of
    N + hop // 2 frames holds exactly one whole analysis frame, whatever its position: one step without a peak."""
    x = comb(N, frames, channels, seed)
    gap_len = N + hop // 2 if gap_len is None else gap_len
    for s in starts:
        x[gap_channel, max(s, 0):max(s + gap_len, 0)] = 0.0
    return x


def quarter(frames, channels=1):
    """0.5 * cos(pi n / 2): a single line at a quarter of the sample rate, which is 0.5, 0, -0.5, 0 exactly"""
    x = np.tile(np.array([0.5, 0.0, -0.5, 0.0]), frames // 4 + 1)[:frames]
    return _grid(np.broadcast_to(x, (channels, frames)))


def dc(frames, channels=1):
    """0.25 throughout: energy in bins 0 and 1 only, where no peak is looked for"""
    return _grid(np.full((channels, frames), 0.25))
