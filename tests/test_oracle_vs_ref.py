"""Live cross-check of the oracle against the REAL reference binaries in oracle/_ref/ (built by
oracle/ref.mk from /root/reference).  Skipped where those binaries are absent."""
import numpy as np
import pytest

from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import bits_equal

pytestmark = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built (needs /root/reference)")

CASES = [
    dict(semitones=5.0, coremode=1),
    dict(semitones=-5.0, coremode=0),
    dict(semitones=2.0, coremode=2, fftsize=1024),
    dict(mode="time_stretch", time_ratio=0.75, flush=False),
    dict(mode="time_stretch", time_ratio=2.0, flush=False),
    dict(mode="gender_change", semitones=0.0),
    dict(mode="formant_pitchshift", semitones=3.0, fftsize=4096),
    dict(semitones=4.0, block=64),
    dict(semitones=4.0, block=4800),
    dict(mode="robotic"),
    # large pitch ratios (tests/test_resample_rungs_host.py): long filters, oversampling 4 / 2, direct tables with 256 and
    # 512 taps, den = 4 and den = oversample = 8, and the 32-bit wrap in the oversampling rule just above 0 semitones
    dict(semitones=24.0, fftsize=512),
    dict(semitones=30.0, fftsize=512),
    dict(semitones=36.0, fftsize=512),
    dict(semitones=-24.0, fftsize=512),
    dict(semitones=-36.0, fftsize=512),
    dict(semitones=0.16, fftsize=512),
]


@pytest.mark.parametrize("kw", CASES, ids=[str(i) for i in range(len(CASES))])
def test_offline_matches_reference(kw):
    x = signals.voice(20000, 2, seed=321)
    want, wc = O.ref_run(x, **kw)
    got, gc, _ = O.run_offline(x, **kw)
    assert gc == wc
    assert bits_equal(got, want)


# The level cases of tests/analysis_signals.py (voice times a power of two: components below 2^-48, subnormal and
# underflowing squares, components above 2^63; a DC offset; holes) and the peak search's corner cases: where the plane
# tests find the device and the oracle apart, this says which of the two the reference sides with.
LEVEL_FFTS = (512, 1024, 4096)


@pytest.mark.parametrize("fft", LEVEL_FFTS)
@pytest.mark.parametrize("kind", ["ordinary", "mixed", "out", "subnormal", "zero", "loud", "dc", "holes", "corners",
                                  "outer", "dcnyq", "single"])
def test_level_and_corner_cases_match_reference(kind, fft):
    from tests import analysis_signals as A
    c = A.BY_NAME[f"{kind}_{fft}"]
    for j in (0, 1):
        x = A.streams(c.name)[j]
        want, wc = O.ref_run(x, block=A.BLOCK, fftsize=fft, **c.cfg)
        got, gc, _ = A.oracle(c.name, j)
        assert list(gc) == wc
        assert bits_equal(got, want)
        assert np.isfinite(want).all() and (kind == "zero" or np.abs(want).max() > 0)


def _ola_rows():
    from tests import ola_advance_signals as S
    return S.DEFINED


@pytest.mark.parametrize("name", _ola_rows())
def test_overlap_add_advance_rows_match_reference(name):
    """The rows of tests/ola_advance_signals.py (advances from 1 to the FFT size, dropped slices, the non-finite samples
    of an advance of N) through the compiled reference: the same counts, and the same bits wherever the reference's
    samples are finite -- and non-finite samples at the same positions."""
    from tests import ola_advance_signals as S
    row = S.BY_NAME[name]
    want, wc = O.ref_run(S.clip(name), block=row.block, flush=True, **row.cfg)
    run = S.oracle(name)
    assert list(run.counts) == wc
    fin = np.isfinite(want)
    assert want.shape == run.y.shape and np.array_equal(np.isfinite(run.y), fin)
    assert np.array_equal(run.y.view(np.uint32)[fin], want.view(np.uint32)[fin])
    assert np.count_nonzero(~fin) == S.FIGURES[name][4]


def test_realtime_matches_reference():
    x = signals.noise(20000, 2)
    want, wc = O.ref_run(x, api="rt", semitones=-7.0, block=512)
    got, gc = O.run_realtime(x, semitones=-7.0, block=512)
    assert gc == wc
    assert bits_equal(got, want)


def test_chunking_independence():
    """Output stream does not depend on call chunking."""
    x = signals.voice(20000, 2, seed=9)
    a, _, _ = O.run_offline(x, semitones=4.0, block=64)
    b, _, _ = O.run_offline(x, semitones=4.0, block=4800)
    assert bits_equal(a, b)


def test_random_configurations_bit_identical_to_the_reference():
    """A slice of tests/sweeps/fuzz_oracle_vs_ref.py (the full sweep: profiles/r01/fuzz_oracle_vs_ref_summary.txt):
    random mode / pitch / ratio / FFT size / hop / rate / channels / call size through the oracle and through the
    compiled reference, offline and real-time loops, outputs compared bit for bit."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "sweeps", "fuzz_oracle_vs_ref.py"), "120", "9"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "differing or failed: 0" in r.stdout
