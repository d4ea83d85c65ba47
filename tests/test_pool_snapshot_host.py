"""Stream-pool snapshots without a GPU: the blob codec (audiomod_amd/csrc/pv_snapshot.h) driven natively -- host state
through a blob and back, continued side by side with the original; the validator against every prefix and thousands of
flips -- once plain and once under AddressSanitizer + UndefinedBehaviorSanitizer, and the host-only entry points of
the C ABI (include/audiomod_pv.h pv_pool_blob_info and the NULL refusals)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from audiomod_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
SOURCES = [os.path.join(ROOT, "tests/native/host_snapshot.cc"), os.path.join(ROOT, "audiomod_amd/csrc/pv_plan.cc")]
INCLUDES = [f"-I{ROOT}/include", f"-I{ROOT}/audiomod_amd/csrc"]


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """the native program, built once; running it with a path also writes a blob of known fields there"""
    d = tmp_path_factory.mktemp("host_snapshot")
    exe = str(d / "host_snapshot")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *INCLUDES, *SOURCES, "-o", exe], check=True)
    blob = str(d / "blob.bin")
    r = subprocess.run([exe, blob], capture_output=True, text=True)
    return r, blob


def test_host_state_round_trip_and_validator(native):
    r, _ = native
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
    assert int(r.stdout.split(" configurations")[0].split()[-1]) >= 200, r.stdout


def test_codec_under_sanitizers(tmp_path):
    exe = str(tmp_path / "host_snapshot_sanitize")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", *INCLUDES, *SOURCES, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        pytest.skip("sanitizer runtimes not installed")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout


def test_blob_info_reports_what_the_codec_wrote(native):
    r, path = native
    assert r.returncode == 0, r.stdout + r.stderr
    blob = open(path, "rb").read()
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("blob:")).split()
    said = {line[i]: int(line[i + 1]) for i in range(1, len(line), 2)}
    info = E.blob_info(blob)
    assert info["version"] == 1 and info["total_bytes"] == len(blob) == said["total"]
    assert info["cfg"] == dict(sample_rate=44100, channels=2, time_ratio=1.25, pitch_semitones=-3.5, mode=E.NORMAL_SHIFT,
                               coremode=1, fftsize=1024, hopsize=0)
    assert (info["time_ratio"], info["pitch_semitones"]) == (1.25, -3.5)
    assert info["arithmetic"] == said["arith"] and info["arithmetic"] in (E.ARITH_FAST, E.ARITH_EXACT)
    assert info["slices"] == said["slices"] > 0
    assert info["pending_frames"] == said["pending"] > 0
    assert info["payload_bytes"] == said["payload"] > 0
    for bad in (blob[:-1], blob[:len(blob) // 2], blob + b"\0", blob[:200] + bytes([blob[200] ^ 1]) + blob[201:]):
        with pytest.raises(E.PvError, match="invalid argument"):
            E.blob_info(bad)


def test_host_only_refusals():
    L = E.lib()
    d = E.BlobDesc()
    garbage = bytes(range(256)) * 4
    for blob, n in ((garbage, len(garbage)), (b"", 0), (None, 0), (None, 4096), (garbage, -1)):
        assert L.pv_pool_blob_info(blob, n, C.byref(d)) == 1
        assert L.pv_last_error()
    assert L.pv_pool_blob_info(garbage, len(garbage), None) == 1
    assert L.pv_pool_restore(None, 0, None, None, None) == 1
    assert L.pv_pool_save(None, 0, None, None, None, None) == 1
    assert L.pv_pool_snapshot_bytes(None, 0) == -1
