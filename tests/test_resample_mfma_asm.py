"""Static checks on the gfx950 assembly of the fast resampling kernel (pv_resample_mfma_kernel): it runs its filter
taps on the f32 matrix cores, does not spill, and asks for no LDS beyond the dynamic size its launcher computes --
the tables plus at most 16 rows x lds_floats, what the vector kernel's 16-row launch used."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc")

KERNEL = "pv_resample_mfma_kernel"


@pytest.fixture(scope="module")
def kernel_asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("asm") / "pv_kernels.s")
    flags = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]  # the Makefile's
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", *flags, f"-I{ROOT}/include",
           f"-I{ROOT}/audiomod_amd/csrc", "--cuda-device-only", "-S", f"{ROOT}/audiomod_amd/csrc/pv_kernels.hip", "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return open(out).read()


def _kernels(text):
    names = sorted(set(re.findall(r"^(_ZN2pv\d+%s\w*):" % KERNEL, text, re.M)))
    assert len(names) == 2, names  # kRes = 1 (direct sinc table) and 2 (interpolated table)
    return names


def _body(text, name):
    i = text.index("\n" + name + ":")
    return text[i:text.index(".end_amdhsa_kernel", i)]


def _meta(text, name):
    """the kernel's entry in the amdhsa.kernels metadata"""
    i = text.index(".name:           " + name)
    j = text.find("\n  - .", i)
    k = text.rfind("\n  - .", 0, i)
    return text[k:j if j > 0 else len(text)]


def test_fast_resampler_runs_on_f32_matrix_cores(kernel_asm):
    for name in _kernels(kernel_asm):
        body = _body(kernel_asm, name)
        assert re.search(r"\bv_mfma_f32_(16x16x4|32x32x2)_f32\b", body), name


def test_fast_resampler_uses_no_scratch(kernel_asm):
    for name in _kernels(kernel_asm):
        assert re.search(r"\.private_segment_fixed_size: 0\b", _meta(kernel_asm, name)), name
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", _body(kernel_asm, name)), name


def test_fast_resampler_has_no_static_lds(kernel_asm):
    """All of its LDS is the dynamic request of launch_resample_fast (tables, staged rows at a padded stride that
    stays below lds_floats, four flag words in the room that saves): a static segment would add to it."""
    for name in _kernels(kernel_asm):
        assert re.search(r"\.group_segment_fixed_size: 0\b", _meta(kernel_asm, name)), name
        assert re.search(r"\.amdhsa_group_segment_fixed_size 0\b", _body(kernel_asm, name)), name
