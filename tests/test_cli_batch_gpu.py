"""`audiomod-pv-exe batch` on the GPU: every output file must be byte for byte -- header included -- what the single-file
command writes for the same file and amount, whichever route the job takes (the mixed batch's PCM wire, or one engine
per file where the mixed batch does not serve the model), however the group is cut into sub-batches, and whatever
happens to the jobs beside it."""
import os
import struct
import subprocess

import numpy as np
import pytest

from audiomod_amd import engine as E
from audiomod_amd import signals
from tests.helpers import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "audiomod_amd", "lib", "audiomod-pv-exe")
TIMEOUT = 120

# name: (rate, channels, bits, frames)
FILES = {
    "a": (48000, 2, 16, 4801),
    "b": (48000, 2, 24, 700),
    "c": (48000, 1, 16, 12000),
    "d": (44100, 2, 16, 3000),
    "e": (48000, 2, 8, 1),
    "f": (48000, 2, 32, 9000),
}


def _wav_bytes(rate, channels, bits, frames, seed):
    v = signals.voice(frames, channels, seed=seed, sample_rate=rate, dtype=np.float64).T
    rng = np.random.default_rng(seed)
    if bits == 8:
        x = np.clip(np.round(v * 128.0) + 128, 0, 255)
    elif bits == 16:
        x = np.round(v * 32768.0)
    else:
        x = np.round(v * 32768.0) * (1 << (bits - 16)) + rng.integers(0, 1 << (bits - 16), size=v.shape)
    data = E.pcm_bytes(x.astype(np.int64), bits).tobytes()
    ba = channels * bits // 8
    fmt = struct.pack("<HHIIHH", 1, channels, rate, rate * ba, ba, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body + (b"\x00" if len(data) & 1 else b"")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("corpus")
    paths = {}
    for i, (name, spec) in enumerate(sorted(FILES.items())):
        p = d / f"in {name}.wav"  # (a space in every path: fields are separated by tabs)
        p.write_bytes(_wav_bytes(*spec, seed=700 + i))
        paths[name] = str(p)
    return paths


@pytest.fixture(scope="module")
def single(corpus, tmp_path_factory):
    """the single-file command's output for (model, file, arguments), run once per module"""
    d = tmp_path_factory.mktemp("single")
    cache = {}

    def get(model, name, args):
        key = (model, name, tuple(args))
        if key not in cache:
            out = d / f"{len(cache)}.wav"
            r = subprocess.run([CLI, model, corpus[name], str(out), *args], capture_output=True, text=True, timeout=TIMEOUT)
            assert r.returncode == 0, r.stderr
            cache[key] = out.read_bytes()
        return cache[key]
    return get


def _batch(tmp_path, model, jobs, corpus, args, extra=()):
    """jobs: (file name, amount or None); returns the process and the output paths"""
    outs = [str(tmp_path / f"out {i} {name}.wav") for i, (name, _) in enumerate(jobs)]
    lines = ["# manifest of the test", ""]
    for (name, amount), out in zip(jobs, outs):
        lines.append(corpus.get(name, name) + "\t" + out + ("" if amount is None else "\t" + amount))
    man = tmp_path / "jobs.tsv"
    man.write_text("\n".join(lines) + "\n")
    r = subprocess.run([CLI, "batch", model, str(man), *args, *extra], capture_output=True, text=True, timeout=TIMEOUT)
    return r, outs


def _assert_ok(r, jobs, outs):
    assert r.returncode == 0, r.stderr
    rows = [l.split("\t") for l in r.stdout.splitlines()]
    assert [row[:2] for row in rows] == [["ok", o] for o in outs], r.stdout
    for row, o in zip(rows, outs):
        size = os.path.getsize(o)
        assert int(row[2]) * 2 * FILES[os.path.basename(o)[-5]][1] == size - 56


PITCH_JOBS = [("a", "-3"), ("b", None), ("c", "7"), ("d", "12"), ("e", "-12"), ("f", "0.5")]


def test_pitch_shift_outputs_are_the_single_file_commands(corpus, single, tmp_path):
    r, outs = _batch(tmp_path, "normal_pitchshift", PITCH_JOBS, corpus, ("4", "1", "512"))
    _assert_ok(r, PITCH_JOBS, outs)
    for (name, amount), out in zip(PITCH_JOBS, outs):
        want = single("normal_pitchshift", name, (amount or "4", "1", "512"))
        assert open(out, "rb").read() == want, (name, amount)


def test_time_stretch_outputs_are_the_single_file_commands(corpus, single, tmp_path):
    jobs = [("a", None), ("f", "0.75"), ("c", "2")]
    r, outs = _batch(tmp_path, "time_stretch", jobs, corpus, ("1.5", "1", "512"))
    _assert_ok(r, jobs, outs)
    for (name, amount), out in zip(jobs, outs):
        assert open(out, "rb").read() == single("time_stretch", name, (amount or "1.5", "1", "512")), (name, amount)


def test_whisper_takes_the_single_stream_route(corpus, single, tmp_path):
    jobs = [("a", None), ("d", None)]
    r, outs = _batch(tmp_path, "whisper", jobs, corpus, ())
    _assert_ok(r, jobs, outs)
    for (name, _), out in zip(jobs, outs):
        assert open(out, "rb").read() == single("whisper", name, ()), name


def test_a_small_budget_cuts_three_sub_batches_and_redraws(corpus, single, tmp_path):
    """Estimates (bytes, stereo): a 249 652, b 37 800, f 504 000, e 50.  With 0.00028 GiB (300 647 bytes) the 48 kHz
    stereo group a, b, f, e is cut into [a, b], [f] (alone: above the budget on its own) and [e]; the third has the
    second's clip count and re-draws its object in place."""
    jobs = [("a", "-3"), ("c", "7"), ("b", None), ("f", "0.5"), ("d", "12"), ("e", "-12")]
    r, outs = _batch(tmp_path, "normal_pitchshift", jobs, corpus, ("4", "1", "512"), ("--mem-gb", "0.00028"))
    _assert_ok(r, jobs, outs)
    assert "48000 Hz, 2 ch: 4 clips, 3 sub-batches, 1 re-drawn in place" in r.stderr, r.stderr
    for (name, amount), out in zip(jobs, outs):
        assert open(out, "rb").read() == single("normal_pitchshift", name, (amount or "4", "1", "512")), (name, amount)


def test_a_bad_file_fails_alone(corpus, single, tmp_path):
    cut = tmp_path / "truncated.wav"
    cut.write_bytes(open(corpus["a"], "rb").read()[:30])
    missing = str(tmp_path / "nowhere.wav")
    jobs = [("a", "-3"), (str(cut), None), ("f", "0.5"), (missing, "2")]
    r, outs = _batch(tmp_path, "normal_pitchshift", jobs, corpus, ("4", "1", "512"))
    assert r.returncode == 1, r.stderr
    rows = [l.split("\t") for l in r.stdout.splitlines()]
    assert [row[0] for row in rows] == ["ok", "failed", "ok", "failed"], r.stdout
    assert rows[0][1] == outs[0] and rows[2][1] == outs[2]
    assert rows[1][1] == str(cut) and "WAV" in rows[1][2]
    assert rows[3][1] == missing and "cannot open" in rows[3][2]
    assert not os.path.exists(outs[1]) and not os.path.exists(outs[3])
    assert open(outs[0], "rb").read() == single("normal_pitchshift", "a", ("-3", "1", "512"))
    assert open(outs[2], "rb").read() == single("normal_pitchshift", "f", ("0.5", "1", "512"))
