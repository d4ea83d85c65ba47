"""The workload bench.py times (BASELINE configs[4]'s per-GPU share: 128 stereo streams x 60 s, +4 st, fft 2048,
phase-locked, two chunks in flight, default chunking) checked at its own size, and the N-rank launch path of
bench.py itself.

Reference loop each stream replicates: /root/reference/main/main.cc:471-510."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RMS_TOL = 1e-4


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.mark.gpu
def test_cfg5_per_gpu_share_at_full_size():
    """128 stereo streams x 60 s through the batch engine exactly as bench.py drives it (rows = 256, 28 chunks of
    128 K slices -- 56 of 64 K until the last change of round 2 -- pipelined): four streams spread over the grid (first, last, two mid-grid rows) against the oracle,
    duplicate-input streams bit for bit, and two runs of the same batch bit for bit."""
    import torch

    from audiomod_amd import engine as E
    from audiomod_amd import signals
    from oracle import oracle_py as O

    S, F = 128, 60 * 48000
    kw = dict(mode="normal_pitchshift", semitones=4.0, coremode=1, fftsize=2048)
    dups = [(S - 1, 0), (S // 2, 1)]
    d_in = signals.synthetic_batch(torch, S, F, torch.device("cuda", 0), duplicates=dups)
    b = E.Batch(S, F, channels=2, block=480, flush=True, **kw)
    assert b.pipelined and b.launches >= 25  # the geometry of the bench line, not a small stand-in
    assert b.slices * 2 * S // b.launches >= 60000
    out = b.run(d_in)
    torch.cuda.synchronize()
    first = signals.batch_checksum(torch, out)[0]
    for a, c in dups:
        assert torch.equal(out[a].view(torch.int32), out[c].view(torch.int32)), (a, c)
    assert not torch.equal(out[2].view(torch.int32), out[3].view(torch.int32))
    for s in (0, S // 3, S // 2 + 5, S - 2):
        want, _, _ = O.run_offline(d_in[s].cpu().numpy(), block=480, flush=True, **kw)
        got = out[s].cpu().numpy()
        assert got.shape == want.shape
        assert _rms(got, want) <= RMS_TOL, s
    out2 = b.run(d_in)  # a second pass over the same device buffers (what bench.py's steps do)
    torch.cuda.synchronize()
    assert signals.batch_checksum(torch, out2)[0] == first
    b.close()


def _bench(args, env=None, timeout=900):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    e.pop("LOCAL_RANK", None)
    if env:
        e.update(env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          env=e, timeout=timeout, cwd=ROOT)


@pytest.mark.gpu
def test_bench_gpus_2_really_runs_two_ranks():
    """`python bench.py --gpus 2` (the form the driver uses, no torchrun around it) must launch two ranks and say
    so; rehearsed on one card with --force-device 0.  Rank sync is gloo on CPU tensors: no RCCL on this path."""
    r = _bench(["--gpus", "2", "--force-device", "0", "--steps", "1", "--warmup", "1", "--streams", "16",
                "--seconds", "10", "--full", "--no-cpu-baseline"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2
    assert line["config"]["streams_per_gpu"] == 16 and "gloo" in line["config"]["rank_sync"]
    assert line["verified"]["ok"] and line["verified"]["ranks_ok"] == 2
    assert line["verified"]["max_rms_vs_oracle"] <= RMS_TOL


@pytest.mark.gpu
def test_bench_line_carries_its_own_verification():
    r = _bench(["--steps", "1", "--warmup", "1", "--streams", "8", "--seconds", "10", "--full", "--no-cpu-baseline"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    v = line["verified"]
    assert line["n_gpus"] == 1 and v["ok"] and v["duplicate_streams_bit_identical"]
    assert v["same_checksum_after_warmup_and_timed_steps"] is True
    assert len(v["batch_checksum_sha256"]) == 64 and len(v["streams_checked"]) >= 2


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) prints the headline line only, and --dump-outputs writes what its last timed step
    computed: the same bits as the batch engine gives on bench.py's seeded input (8 streams: the whole batch fits)."""
    import torch

    from audiomod_amd import engine as E
    from audiomod_amd import signals

    r = _bench(["--steps", "2", "--warmup", "1", "--streams", "8", "--seconds", "10", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "Msamples/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["value"] > 0
    assert not {"roofline", "verified", "cpu_baseline"} & set(line)
    assert os.listdir(tmp_path) == ["output.npy"]
    got = np.load(tmp_path / "output.npy")
    S, F = 8, 10 * 48000
    d_in = signals.synthetic_batch(torch, S, F, torch.device("cuda", 0), duplicates=[(S - 1, 0), (S // 2, 1)])
    b = E.Batch(S, F, channels=2, block=480, flush=True, mode="normal_pitchshift", semitones=4.0, coremode=1,
                fftsize=2048)
    want = b.run(d_in)
    torch.cuda.synchronize()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.cpu().numpy().view(np.uint32))
    b.close()


def test_dump_outputs_samples_a_large_batch_within_its_budget(tmp_path):
    """Above the budget: stream 0 (cut to half the budget) and every stream at the same seeded frame positions."""
    import torch

    import bench

    out = torch.randn(16, 2, 50000)
    budget = 1 << 20
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(torch, out, str(d), budget=budget)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["output_sample.npy", "output_sample_frames.npy", "output_stream0.npy"]
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in files) <= budget
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))  # same positions every run
    first = np.load(tmp_path / "a" / "output_stream0.npy")
    assert np.array_equal(first, out[0, :, :first.shape[1]].numpy())
    frames = np.load(tmp_path / "a" / "output_sample_frames.npy")
    assert frames.dtype == np.float64 and np.all(np.diff(frames) > 0)
    sample = np.load(tmp_path / "a" / "output_sample.npy")
    assert np.array_equal(sample, out[:, :, frames.astype(np.int64)].numpy())


def test_bench_refuses_zero_steps():
    r = _bench(["--steps", "0"], timeout=120)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    """Started under a launcher with the wrong number of ranks, bench.py must fail instead of reporting the wrong
    n_gpus (runs without a GPU: the check comes before anything touches torch)."""
    r = _bench(["--gpus", "4"], env={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, timeout=120)
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr and "--gpus 4" in r.stderr


def test_bench_gpus_n_spawns_ranks_before_touching_the_gpu():
    """Without a GPU the ranks fail with the no-GPU message: proof that `--gpus 2` alone reached the launcher and
    started workers (torchrun tears the other rank down as soon as one exits, so only one message is guaranteed; the
    launcher's own log names both ranks; on the GPU box the gpu-marked test above checks the successful run)."""
    r = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], timeout=600)
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by test_bench_gpus_2_really_runs_two_ranks")
    assert r.returncode != 0
    assert (r.stdout + r.stderr).count("no GPU visible") >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("wire", ["f32", "i16"])
def test_host_staged_path_equals_device_resident(wire):
    """pv_hostio_*: streams held in host memory, staged in groups through the GPU (copy-in / kernels / copy-out
    overlapped).  float32 on the wire: bit-equal to the device-resident batch.  int16 on the wire: equal to the
    reference's WAV writer conversion (saturate(x * 32768) truncated, main/wavfile.cc:1334-1342) of that output.
    11 streams in groups of 4: two full groups and a short last one -- three groups for three buffer slots, so no
    slot is reused here and none of the reuse waits of pv_hostio_run executes; tests/test_hostio_gpu.py holds those
    (eight groups, both wires, saturating int16 output, stale rows)."""
    import torch

    from audiomod_amd import engine as E
    from audiomod_amd import signals

    S, F = 11, 48000
    kw = dict(mode="normal_pitchshift", semitones=4.0, coremode=1, fftsize=2048)
    x = np.stack([signals.voice(F, 2, stream=s) for s in range(S)])
    b = E.Batch(S, F, channels=2, **kw)
    ref = b.run(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    b.close()
    h = E.HostIO(S, F, channels=2, streams_per_group=4, wire=wire, **kw)
    hin = h.pinned((S, 2, F))
    hin[...] = x if wire == "f32" else np.round(x * 32768.0).astype(np.int16)
    out = h.run(hin)
    assert out.shape == ref.shape
    if wire == "f32":
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    else:
        want = np.trunc(np.clip(ref * np.float32(32768.0), -32768.0, 32767.0)).astype(np.int16)
        assert np.array_equal(out, want)
    out2 = h.run(hin).copy()  # a second pass over the same buffers
    assert np.array_equal(out2, out)
    h.close()
