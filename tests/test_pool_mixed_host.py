"""Mixed stream pool (include/audiomod_pv.h pv_pool_create_mixed / pv_pool_open_with / pv_pool_last_launches): the C
ABI, the range checks that come before any device call, and the scratch use of the per-slot-parameter kernels.  No GPU
needed."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import pytest

from audiomod_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
ENTRY_POINTS = ("pv_pool_create_mixed", "pv_pool_open_with", "pv_pool_last_launches")
PV_ERR_INVALID_ARG, PV_ERR_UNSUPPORTED, PV_ERR_NO_DEVICE = 1, 2, 3


def test_header_and_library_have_the_mixed_pool():
    with open(os.path.join(ROOT, "include", "audiomod_pv.h")) as f:
        hdr = f.read()
    assert "typedef struct pv_pool_range {" in hdr
    L = E.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(L, name), name


def _create(rng, capacity=4, channels=2, **kw):
    cfg = E.make_config(channels, **kw)
    h = C.c_void_p()
    r = E.PoolRange(*rng) if rng is not None else None
    st = E.lib().pv_pool_create_mixed(C.byref(cfg), C.byref(r) if r is not None else None, capacity, 0, C.byref(h))
    if st == 0:
        E.lib().pv_pool_destroy(h)
    return st


NAN = float("nan")


@pytest.mark.parametrize("rng,kw", [
    ((12.0, -12.0, 1.0, 1.0), dict(semitones=4.0)),          # inverted pitch range
    ((-12.0, 12.0, 2.0, 1.0), dict(semitones=4.0)),          # inverted ratio range
    ((NAN, 12.0, 1.0, 1.0), dict(semitones=4.0)),
    ((-12.0, 12.0, 1.0, NAN), dict(semitones=4.0)),
    ((-12.0, math.inf, 1.0, 1.0), dict(semitones=4.0)),
    ((-12.0, 3.0, 1.0, 1.0), dict(semitones=4.0)),           # excludes cfg's pitch
    ((-12.0, 12.0, 1.5, 2.0), dict(semitones=4.0)),          # excludes cfg's time ratio
], ids=["inverted", "inverted_ratio", "nan_lo", "nan_ratio", "inf", "excludes_pitch", "excludes_ratio"])
def test_bad_range_is_invalid_before_any_device_call(rng, kw):
    assert _create(rng, **kw) == PV_ERR_INVALID_ARG
    assert E.lib().pv_last_error().decode().startswith("stream pool range")


@pytest.mark.parametrize("kw", [
    dict(mode="vocoder"), dict(mode="whisper"), dict(mode="constant"), dict(mode="formant_cepstral", semitones=4.0),
    dict(semitones=4.0, fftsize=256), dict(semitones=4.0, fftsize=8192),
], ids=["vocoder", "whisper", "constant", "cepstral", "fft256", "fft8192"])
def test_out_of_scope_is_unsupported(kw):
    assert _create((-12.0, 12.0, 1.0, 1.0), **kw) == PV_ERR_UNSUPPORTED
    assert E.lib().pv_last_error().decode().startswith("stream pool")


def test_range_too_wide_for_the_resampling_kernel_names_it():
    assert _create((-12.0, 60.0, 1.0, 1.0), semitones=4.0) == PV_ERR_UNSUPPORTED
    assert "resampling kernel" in E.lib().pv_last_error().decode()


@pytest.mark.parametrize("coremode", [0, 1, 2])
def test_twelve_semitones_each_way_fits(coremode):
    # passes every range check: on a machine without the device it gets as far as the device, otherwise it is created
    st = _create((-12.0, 12.0, 1.0, 1.0), semitones=4.0, coremode=coremode, fftsize=2048)
    assert st == (0 if E.lib().pv_device_count() >= 1 else PV_ERR_NO_DEVICE), E.lib().pv_last_error()


def test_null_handles_are_invalid():
    L = E.lib()
    cfg = E.make_config(2, semitones=4.0)
    h = C.c_void_p()
    assert L.pv_pool_create_mixed(C.byref(cfg), None, 4, 0, C.byref(h)) == PV_ERR_INVALID_ARG
    r = E.PoolRange(-12.0, 12.0, 1.0, 1.0)
    assert L.pv_pool_create_mixed(None, C.byref(r), 4, 0, C.byref(h)) == PV_ERR_INVALID_ARG
    assert L.pv_pool_create_mixed(C.byref(cfg), C.byref(r), 4, 0, None) == PV_ERR_INVALID_ARG
    assert L.pv_pool_create_mixed(C.byref(cfg), C.byref(r), 0, 0, C.byref(h)) == PV_ERR_INVALID_ARG
    s = C.c_int32(-1)
    assert L.pv_pool_open_with(None, 1.0, 4.0, C.byref(s)) == PV_ERR_INVALID_ARG
    n = C.c_int32(-1)
    assert L.pv_pool_last_launches(None, C.byref(n)) == PV_ERR_INVALID_ARG


def test_no_device_no_mixed_pool():
    if E.lib().pv_device_count() >= 1:
        pytest.skip("a gfx950 device is present")
    with pytest.raises(E.PvError, match="no gfx950"):
        E.StreamPool(4, channels=2, semitones=4.0, pitch_range=(-12, 12))


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc")
def test_benchmarked_per_slot_kernels_use_no_scratch(tmp_path):
    """fft 2048, plain phase-locked pitch shift, resampling: the per-slot-parameter analysis, phase, fused synthesis +
    overlap-add and resampling kernels (both arithmetic settings, both resampling tables) must not spill."""
    out = str(tmp_path / "pv_kernels.s")
    flags = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize"]  # the Makefile's
    cmd = [HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", *flags, f"-I{ROOT}/include",
           f"-I{ROOT}/audiomod_amd/csrc", "--cuda-device-only", "-S", f"{ROOT}/audiomod_amd/csrc/pv_kernels.hip", "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    text = open(out).read()
    names = ["_ZN2pv27pv_pmix_analyze_wave_kernelILi1024EEEvNS_11AnalyzeArgsENS_10PoolLaunchEPKNS_10PoolParamsE",
             "_ZN2pv20pv_pmix_phase_kernelILi8EEEvNS_9MatchArgsENS_7SeqArgsENS_10PoolLaunchEPKNS_10PoolParamsE"]
    for fast in ("1", "0"):
        names.append("_ZN2pv26pv_pmix_synth_chain_kernelILi1024ELi1ELi1ELb%sEEEvNS_9SynthArgsENS_9ChainArgsENS_10"
                     "PoolLaunchEPKNS_10PoolParamsE" % fast)
    for k in ("1", "2"):
        names.append("_ZN2pv23pv_pmix_resample_kernelILi%sEEEvNS_7ResArgsENS_10PoolLaunchEPKNS_10PoolParamsE" % k)
        names.append("_ZN2pv28pv_pmix_resample_fast_kernelILi%sEEEvNS_7ResArgsENS_10PoolLaunchEPKNS_10PoolParamsE" % k)
    for name in names:
        m = re.search(r"\.set %s\.private_seg_size, (\d+)" % re.escape(name), text)
        assert m, name
        assert int(m.group(1)) == 0, name
