"""The span arithmetic (audiomod_amd/csrc/pv_plan.cc batch_span) as a stand-alone program under ASan + UBSan: a few
hundred seeded random jobs, every division into spans checked against the contract of pv_batch_span_info.  CPU only;
nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_span_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_spans_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", f"-I{ROOT}/include", f"-I{ROOT}/audiomod_amd/csrc",
           os.path.join(ROOT, "tests/native/host_spans_sanitize.cc"), os.path.join(ROOT, "audiomod_amd/csrc/pv_plan.cc"),
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        pytest.skip("sanitizer runtimes not installed")
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    env.pop("AUDIOMOD_PV_CHUNK_SLICES", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
