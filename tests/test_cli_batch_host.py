"""`audiomod-pv-exe batch` without a GPU: every manifest error is reported with its line number and exit status 2 before
any file is opened or any device call is made, and a valid manifest on a machine without a device ends with the
no-device message and no output file.  (The child processes see no device whatever the machine has.)"""
import os
import struct
import subprocess

import pytest

from tests.helpers import ROOT

CLI = os.path.join(ROOT, "audiomod_amd", "lib", "audiomod-pv-exe")
NO_GPU = dict(os.environ, HIP_VISIBLE_DEVICES="-1")  # the HIP runtime then reports no device


def _wav(path, frames=600, channels=2, rate=48000):
    data = b"\x00\x01" * (frames * channels)
    fmt = struct.pack("<HHIIHH", 1, channels, rate, rate * channels * 2, channels * 2, 16)
    body = b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


def _batch(tmp_path, text, model="normal_pitchshift", args=("4", "1", "512")):
    assert os.path.exists(CLI), "run `make` first"
    man = tmp_path / "jobs.tsv"
    man.write_bytes(text.encode() if isinstance(text, str) else text)
    return subprocess.run([CLI, "batch", model, str(man), *args], capture_output=True, text=True, env=NO_GPU, timeout=60)


def _outputs(tmp_path):
    return sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("out"))


@pytest.mark.parametrize("name,lines,model,args,line", [
    ("one field", ["{a}\t{o1}", "{b}"], "normal_pitchshift", ("4", "1", "512"), 2),
    ("spaces instead of tabs", ["{a} {o1}"], "normal_pitchshift", ("4", "1", "512"), 1),
    ("four fields", ["# jobs", "{a}\t{o1}\t2\t3"], "normal_pitchshift", ("4", "1", "512"), 2),
    ("empty output path", ["{a}\t"], "normal_pitchshift", ("4", "1", "512"), 1),
    ("amount is not a number", ["{a}\t{o1}", "", "{b}\t{o2}\tfast"], "normal_pitchshift", ("4", "1", "512"), 3),
    ("amount is not finite", ["{a}\t{o1}\tnan"], "time_stretch", ("1.5", "1", "512"), 1),
    ("amount on a model that takes none", ["{a}\t{o1}", "{b}\t{o2}\t3"], "whisper", (), 2),
    ("amount on robotic", ["{a}\t{o1}\t0"], "robotic", (), 1),
    ("two jobs with the same output", ["{a}\t{o1}", "{b}\t{o2}", "{b}\t{o1}"], "normal_pitchshift", ("4", "1", "512"), 3),
    ("an output that is also an input", ["{a}\t{o1}", "{b}\t{a}"], "normal_pitchshift", ("4", "1", "512"), 2),
    ("an output that is a later job's input", ["{a}\t{b}", "{b}\t{o2}"], "normal_pitchshift", ("4", "1", "512"), 1),
    ("empty manifest", [], "normal_pitchshift", ("4", "1", "512"), 0),
    ("comments and blank lines only", ["# nothing", "", "   "], "normal_pitchshift", ("4", "1", "512"), 0),
])
def test_manifest_errors_exit_2_with_the_line_number_and_write_nothing(name, lines, model, args, line, tmp_path):
    a, b = _wav(tmp_path / "in a.wav"), _wav(tmp_path / "in b.wav")
    before = {p.name: p.read_bytes() for p in tmp_path.iterdir()}
    names = dict(a=a, b=b, o1=str(tmp_path / "out 1.wav"), o2=str(tmp_path / "out 2.wav"))
    text = "".join(l.format(**names) + "\n" for l in lines)
    r = _batch(tmp_path, text, model, args)
    assert r.returncode == 2, (name, r.returncode, r.stderr)
    assert "line %d:" % line in r.stderr, (name, r.stderr)
    assert r.stdout == ""
    assert _outputs(tmp_path) == []
    for k, v in before.items():  # the inputs are untouched (an output path may name one of them)
        assert (tmp_path / k).read_bytes() == v


def test_a_missing_manifest_is_status_2(tmp_path):
    r = subprocess.run([CLI, "batch", "whisper", str(tmp_path / "nothing.tsv")], capture_output=True, text=True, env=NO_GPU,
                       timeout=60)
    assert r.returncode == 2 and "manifest" in r.stderr


@pytest.mark.parametrize("model,args", [("normal_pitchshift", ("4", "1", "512")), ("whisper", ()),
                                        ("time_stretch", ("1.5", "1", "512", "--mem-gb", "0.5"))])
def test_valid_manifest_without_a_device_gives_the_no_device_message(model, args, tmp_path):
    a, b = _wav(tmp_path / "in a.wav"), _wav(tmp_path / "in b.wav", channels=1, rate=44100)
    amount = "\t-3" if args else ""
    text = "# two jobs\r\n%s\t%s%s\r\n\n%s\t%s\n" % (a, tmp_path / "out 1.wav", amount, b, tmp_path / "out 2.wav")
    r = _batch(tmp_path, text, model, args)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "no gfx950 device" in r.stderr, r.stderr
    assert _outputs(tmp_path) == []


def test_the_single_file_grammar_is_unchanged_without_a_device(tmp_path):
    """a well-formed file still fails with the class's no-device message and leaves no output"""
    a = _wav(tmp_path / "in.wav")
    r = subprocess.run([CLI, "normal_pitchshift", a, str(tmp_path / "out.wav"), "4", "1", "512"], capture_output=True,
                       text=True, env=NO_GPU, timeout=60)
    assert r.returncode == 1 and "no gfx950 device" in r.stderr, r.stderr
    assert _outputs(tmp_path) == []
    r = subprocess.run([CLI, "normal_pitchshift", a], capture_output=True, text=True, env=NO_GPU, timeout=60)
    assert r.returncode == 255 and "usage" in r.stderr
