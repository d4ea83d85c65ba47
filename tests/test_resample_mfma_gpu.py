"""The fast resampler on the matrix cores (pv_resample_mfma_kernel, the default) against the vector kernel it replaces
(AUDIOMOD_PV_RES_MFMA=0, pv_resample_fast_kernel): the same input in two child processes (the switch is read once per
process) must give the same bits -- the matrix-core body is the vector loop's fma chain in the same order.  Where an
input puts inf or NaN into the resampled stream, the matrix-core kernel runs the vector loop for the workgroups that see
it: the non-finite positions and every finite output must agree too."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from audiomod_amd import engine as E, signals

def batch(ns, ch, frames, st, seed):
    import torch
    x = np.stack([signals.voice(frames, ch, seed=seed + s) for s in range(ns)]).astype(np.float32)
    b = E.Batch(ns, frames, channels=ch, semitones=st)
    y = b.run(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    out = y.cpu().numpy()
    b.close()
    return out

def stream(x, sizes, st, **kw):
    pv = E.PhaseVocoder(48000, x.shape[0], 1.0, st, kw.get("mode", E.NORMAL_SHIFT), E.PHASE_LOCKED, 2048)
    pos, outs = 0, []
    while pos < x.shape[1]:
        for n in sizes:
            pv.processInData(x[:, pos:pos + n])
            pos += n
            outs.append(pv.getOutData(pv.getOutSamples()))
    pv.close()
    return np.concatenate(outs, 1)

res = {}
# pitch: interpolated table (+4, +7, -7) and direct table (+12); down- and up-sampling
for st in (4.0, 7.0, -7.0, 12.0):
    res["pitch%%+g" %% st] = batch(6, 2, 30000, st, 11)
# +16.5: 164 taps, oversampling 4, 64 064 of the 65 536 bytes of LDS below which the matrix-core kernel runs -- the only
# large-ratio regime in which the two settings of the switch still run different kernels (16 rows of 9 streams + 1)
res["pitch+16.5"] = batch(9, 2, 6000, 16.5, 21)
# -24: the direct table at 18 rows -- under the vector switch the only route to the 16-row vector kernel with a direct
# table (the census says which kernel each child launched)
E.chain_census(True)
res["pitch-24x18"] = batch(9, 2, 6000, -24.0, 31)
res["census-24x18"] = np.array(repr(sorted(E.resample_census_read())))
E.chain_census(False)
# rows per batch: partial row groups of the 16-row workgroups
for ns, ch in ((1, 1), (1, 2), (3, 1), (17, 1), (128, 2)):
    res["rows%%d" %% (ns * ch)] = batch(ns, ch, 12000 if ns * ch > 32 else 24000, 4.0, 40 + ns)
# the single-stream engine, ragged calls: partial last tiles of every size
x = signals.voice(40000, 2, seed=5)
res["ragged+4"] = stream(x, [1, 479, 4097, 13, 9000, 480, 7, 333], 4.0)
res["ragged-7"] = stream(x, [7, 1021, 97, 2500], -7.0)
res["ragged+12"] = stream(x, [641, 3, 1500], 12.0)
res["ragged+16.5"] = stream(x[:, :12000], [1, 479, 4097, 13, 480, 7, 333], 16.5)
# an inf / NaN burst in the input
y = signals.voice(30000, 2, seed=9)
y[0, 12000:12040] = np.inf
y[1, 12000:12003] = np.nan
y[1, 20000] = -np.inf
res["nonfinite"] = stream(y, [480], 4.0)
np.savez(sys.argv[1], **res)
print("child ok")
"""


def _run(tmp_path, mfma):
    out = str(tmp_path / ("mfma%s.npz" % mfma))
    env = dict(os.environ)
    env.pop("AUDIOMOD_PV_RES_MFMA", None)
    if mfma == "0":
        env["AUDIOMOD_PV_RES_MFMA"] = "0"
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, out], capture_output=True, text=True, env=env,
                       timeout=900)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
    return dict(np.load(out))


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    d = tmp_path_factory.mktemp("resmfma")
    return _run(d, "1"), _run(d, "0")


CASES = ["pitch+4", "pitch+7", "pitch-7", "pitch+12", "pitch+16.5", "pitch-24x18", "rows1", "rows2", "rows3", "rows17",
         "rows256", "ragged+4", "ragged-7", "ragged+12", "ragged+16.5"]


@pytest.mark.parametrize("case", CASES)
def test_matrix_core_resampler_is_bit_identical(both, case):
    m, v = both[0][case], both[1][case]
    assert m.shape == v.shape and m.size > 0
    assert np.isfinite(v).all()
    diff = np.flatnonzero(m.view(np.uint32) != v.view(np.uint32))
    assert diff.size == 0, (case, diff.size, diff[:8])


def test_the_two_children_ran_different_kernels(both):
    assert str(both[0]["census-24x18"]) == repr([("batch", "mfma", 0, 0)])
    assert str(both[1]["census-24x18"]) == repr([("batch", "vec16", 0, 0)])


def test_matrix_core_resampler_non_finite_fallback(both):
    m, v = both[0]["nonfinite"], both[1]["nonfinite"]
    assert m.shape == v.shape
    fin = np.isfinite(v)
    assert not fin.all() and fin.any()  # the burst reached the output, and not all of it
    assert np.array_equal(np.isfinite(m), fin)
    assert np.array_equal(np.isnan(m), np.isnan(v))
    assert np.array_equal(m[fin].view(np.uint32), v[fin].view(np.uint32))
