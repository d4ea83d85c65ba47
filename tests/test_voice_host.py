"""The voice setting without a GPU: the device generator's step (audiomod_amd/csrc/pv_whisper.h) run natively, lane by
lane as the kernel runs it, against WhisperRng -- 200 000 draws in one launch and split at every boundary of the
step's geometry, words, phases and the carried state bit for bit -- once plain and once under AddressSanitizer +
UndefinedBehaviorSanitizer; and the new symbols and constants of the C ABI (include/audiomod_pv.h "Voice setting")."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from audiomod_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests/native/host_whisper.cc"), os.path.join(ROOT, "audiomod_amd/csrc/pv_plan.cc")]
INCLUDES = [f"-I{ROOT}/include", f"-I{ROOT}/audiomod_amd/csrc"]
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@needs_gxx
def test_generator_step_matches_rand(tmp_path):
    exe = str(tmp_path / "host_whisper")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *INCLUDES, *SOURCES, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"host_whisper: (\d+) cases, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 12, r.stdout  # one launch, the nine cuts, all cuts in a row, the layout


@needs_gxx
def test_generator_step_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_whisper_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", *INCLUDES, *SOURCES, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        pytest.skip("sanitizer runtimes not installed")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert ", 0 failures" in r.stdout, r.stdout


def test_symbols_and_constants():
    L = E.lib()
    for name in ("pv_pool_set_voice", "pv_pool_get_voice", "pv_mbatch_set_voice", "pv_debug_whisper_phases"):
        assert hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "audiomod_pv.h")).read()
    assert re.search(r"#define PV_VOICE_ROBOTIC 0\b", header) and re.search(r"#define PV_VOICE_WHISPER 1\b", header)
    assert re.search(r"#define PV_CENSUS_VOICE 8\b", header)
    assert E.VOICES == {"robotic": 0, "whisper": 1} and E.CENSUS_VOICE == 8


def test_host_only_refusals():
    """what is decided without a device: NULL objects, and the diagnostics call's arguments"""
    L = E.lib()
    v = C.c_int(5)
    assert L.pv_pool_set_voice(None, 0, 1) == 1
    assert L.pv_pool_get_voice(None, 0, C.byref(v)) == 1 and v.value == 5
    assert L.pv_mbatch_set_voice(None, None) == 1
    counts = (C.c_int64 * 2)(4, -1)
    out = (C.c_float * 8)()
    assert L.pv_debug_whisper_phases(counts, 2, out, 0) == 1
    assert L.pv_debug_whisper_phases(None, 2, out, 0) == 1
    counts = (C.c_int64 * 1)(4)
    assert L.pv_debug_whisper_phases(counts, 1, None, 0) == 1
    # the census key exists (and reads 0 with the census off); a neighbouring number is no kind
    E.chain_census(False)
    assert L.pv_debug_chain_census_count(E.CENSUS_VOICE, 1, 1024, 0, 0, 0) == 0
    assert L.pv_debug_chain_census_count(E.CENSUS_VOICE, 1, 1000, 0, 0, 0) == -1
    assert L.pv_debug_chain_census_count(9, 1, 1024, 0, 0, 0) == -1
