"""CPU checks of the PCM wire's host-side pieces, compiled with g++ from the same headers the product uses:
audiomod_amd/csrc/pv_pcm.h (the conversions of the mixed batch's PCM kernels) against the WAV reader's and writer's own
expressions, and audiomod_amd/csrc/pv_cli_batch.h (manifest parser, WAV reader, sub-batch arithmetic of
`audiomod-pv-exe batch`) on hostile input under ASan + UBSan, as a stand-alone program.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_pcm_conversions_equal_the_wav_readers_double_expressions(tmp_path):
    """every 8-, 16- and 24-bit value, the 32-bit values around every multiple of 2^7 ... 2^31 plus 2^26 random ones,
    and the writer on every int16 boundary with its float neighbours and the special values"""
    exe = str(tmp_path / "host_pcm")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{ROOT}/audiomod_amd/csrc",
                    os.path.join(ROOT, "tests/native/host_pcm.cc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout + r.stderr
    # the kernels convert with this header's functions, not with a restatement
    dev = open(os.path.join(ROOT, "audiomod_amd/csrc/pv_kernels.hip")).read()
    for name in ("pv_pcm_u8_to_f32(", "pv_pcm_i16_to_f32(", "pv_pcm_i32_to_f32(", "pv_pcm_load(", "pv_pcm_f32_to_i16("):
        assert name in dev, name


def test_cli_batch_header_under_sanitizers(tmp_path):
    """hostile manifests, the hostile WAV headers of test_cli_wav.py and the sub-batch arithmetic at its limits"""
    exe = str(tmp_path / "host_cli_batch_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           f"-I{ROOT}/audiomod_amd/csrc", os.path.join(ROOT, "tests/native/host_cli_batch_sanitize.cc"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        pytest.skip("sanitizer runtimes not installed")
    assert b.returncode == 0, b.stderr
    work = tmp_path / "wavs"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
