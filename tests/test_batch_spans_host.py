"""Batch spans (include/audiomod_pv.h pv_batch_plan_spans / pv_batch_span / pv_batch_run_span and
pv_hostio_create_segmented): the C ABI, the contract of the planned ranges and the checks that come before any device
call.  No GPU needed.

The ranges are checked against a restatement of what the analysis kernels load for a slice (pv_kernels.hip): the
generic kernel and the slow branch of the wave kernels read [a0, min(frames, a0 + N)); the wave kernels' fast branch,
taken when a0 + N + 4 <= frames, reads the N / 4 + 1 aligned 16-byte pieces from the one that holds a0."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from audiomod_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pv_batch_plan_spans", "pv_batch_span", "pv_batch_run_span", "pv_hostio_create_segmented",
                "pv_hostio_staging_bytes")
PV_ERR_INVALID_ARG, PV_ERR_UNSUPPORTED, PV_ERR_NO_DEVICE = 1, 2, 3
BLOCK = 480
CHUNK = "4"  # slices per launch: many launches on short inputs

# name: (configuration, streams, frames, flush)
CASES = {
    "a_pitch_fft2048_cm1": (dict(channels=2, semitones=4.0, coremode=1, fftsize=2048), 2, 20000, True),
    "b_stretch_fft4096": (dict(channels=2, mode="time_stretch", time_ratio=1.5, fftsize=4096), 2, 20000, False),
    "c_formant_down7": (dict(channels=2, mode="formant_pitchshift", semitones=-7.0, fftsize=2048), 2, 20000, True),
    "d_fft256_up15": (dict(channels=2, semitones=15.558, fftsize=256), 2, 9000, True),
    "e_mono_fft1024_hop300": (dict(channels=1, semitones=3.0, fftsize=1024, sample_rate=44100, hopsize=300), 2, 20000, True),
    "f_shorter_than_a_frame": (dict(channels=2, mode="time_stretch", time_ratio=1.5, fftsize=4096), 2, 100, False),
    "g_2049_frames": (dict(channels=2, semitones=4.0, coremode=1, fftsize=2048), 2, 2049, True),
    "h_96_streams": (dict(channels=2, semitones=4.0, coremode=1, fftsize=2048), 96, 6000, True),
}
BOTH_ARITH = ("a_pitch_fft2048_cm1", "b_stretch_fft4096")


@pytest.fixture(autouse=True)
def _chunks(monkeypatch):
    monkeypatch.setenv("AUDIOMOD_PV_CHUNK_SLICES", CHUNK)


@pytest.fixture
def exact():
    prev = E.set_arithmetic(E.ARITH_EXACT)
    yield
    E.set_arithmetic(prev)


def test_header_and_library_have_the_spans():
    with open(os.path.join(ROOT, "include", "audiomod_pv.h")) as f:
        hdr = f.read()
    assert "typedef struct pv_batch_span_info {" in hdr
    L = E.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(L, name), name
    assert C.sizeof(E.SpanInfo) == 56


def _job(name):
    """(spans of one launch each, hop, N, slices, out_frames as the planner alone gives them)"""
    kw, S, frames, flush = CASES[name]
    one = E.plan_spans(S, frames, 1, block=BLOCK, flush=flush, **kw)
    calls = [min(BLOCK, frames - i) for i in range(0, frames, BLOCK)]
    avail, shift, _, info = E.plan_simulate(calls, **kw)
    if flush:
        out_frames = frames  # the flush feeds zeros until `frames` outputs exist and truncates to them
        slices = None        # (how many flush calls that takes is the batch planner's business)
    else:
        out_frames, slices = int(avail.sum()), len(shift)
    return one, info["hop_in"], info["fftsize"], slices, out_frames


def _check_contract(spans, frames, hop, N, slices, out_frames):
    assert len(spans) >= 1
    k, launch, t = 0, 0, 0
    prev = None
    for sp in spans:
        assert sp["first_launch"] == launch and sp["slice_begin"] == t
        launch += sp["launches"]
        t = sp["slice_end"]
        assert sp["slice_end"] >= sp["slice_begin"]
        assert sp["slice_end"] - sp["slice_begin"] <= sp["launches"] * int(CHUNK)
        # out ranges partition [0, out_frames) in order
        assert sp["out_begin"] == k and sp["out_end"] >= k
        k = sp["out_end"]
        # input range
        assert 0 <= sp["in_begin"] <= sp["in_end"] <= frames
        assert sp["in_begin"] % 4 == 0
        if prev is not None:
            for key in ("in_begin", "in_end", "out_begin", "out_end"):
                assert sp[key] >= prev[key], key
        prev = sp
        if sp["slice_end"] > sp["slice_begin"]:
            lo, hi = sp["slice_begin"] * hop, min(frames, (sp["slice_end"] - 1) * hop + N)
            if hi > lo:
                assert sp["in_begin"] <= lo and hi <= sp["in_end"]
        # everything the analysis kernels load for each slice
        for s in range(sp["slice_begin"], sp["slice_end"]):
            a0 = s * hop
            if a0 + N + 4 <= frames:   # the wave kernels' fast branch: aligned pieces, one more than the frame needs
                lo, hi = a0 - a0 % 4, a0 - a0 % 4 + N + 4
            else:                      # element by element, tested against the stream's length
                lo, hi = min(a0, frames), min(frames, a0 + N)
            if hi > lo:
                assert sp["in_begin"] <= lo and hi <= sp["in_end"], (s, sp)
    assert k == out_frames
    if slices is not None:
        assert t == slices


def _merge(parts):
    return dict(first_launch=parts[0]["first_launch"], launches=sum(p["launches"] for p in parts),
                slice_begin=parts[0]["slice_begin"], slice_end=parts[-1]["slice_end"],
                in_begin=min(p["in_begin"] for p in parts), in_end=max(p["in_end"] for p in parts),
                out_begin=parts[0]["out_begin"], out_end=parts[-1]["out_end"])


def _check_case(name):
    kw, S, frames, flush = CASES[name]
    one, hop, N, slices, out_frames = _job(name)
    _check_contract(one, frames, hop, N, slices, out_frames)
    launches = sum(sp["launches"] for sp in one)
    if name != "f_shorter_than_a_frame" and name != "g_2049_frames":
        assert launches > 6, launches
    cuts = {sp["out_end"] for sp in one}
    for k in (2, 3, max(launches, 1)):
        spans = E.plan_spans(S, frames, k, block=BLOCK, flush=flush, **kw)
        assert len(spans) == max(1, -(-launches // k))
        _check_contract(spans, frames, hop, N, slices, out_frames)
        assert {sp["out_end"] for sp in spans} <= cuts
        # a merged span's ranges are the hull of its parts
        for sp in spans:
            parts = one[sp["first_launch"]:sp["first_launch"] + sp["launches"]]
            if parts:
                assert sp == _merge(parts), (sp, parts)
    return one


@pytest.mark.parametrize("name", sorted(CASES))
def test_planned_spans_keep_the_contract(name):
    _check_case(name)


@pytest.mark.parametrize("name", BOTH_ARITH)
def test_planned_spans_keep_the_contract_exact(name, exact):
    _check_case(name)


def test_a_job_without_slices_is_one_empty_span():
    kw, S, frames, flush = CASES["f_shorter_than_a_frame"]
    spans = E.plan_spans(S, frames, 1, block=BLOCK, flush=flush, **kw)
    assert spans == [dict(first_launch=0, launches=0, slice_begin=0, slice_end=0, in_begin=0, in_end=0, out_begin=0,
                          out_end=0)]


def test_the_chunk_knob_and_the_row_count_decide_the_launches(monkeypatch):
    kw, S, frames, flush = CASES["a_pitch_fft2048_cm1"]
    four = E.plan_spans(S, frames, 1, block=BLOCK, flush=flush, **kw)
    monkeypatch.setenv("AUDIOMOD_PV_CHUNK_SLICES", "8")
    eight = E.plan_spans(S, frames, 1, block=BLOCK, flush=flush, **kw)
    assert len(eight) == -(-four[-1]["slice_end"] // 8) and len(four) == -(-four[-1]["slice_end"] // 4)
    # pv_batch_create's own rule: 65536 / rows slices (131072 for the wide chunks), between 16 and 256 (512) per launch
    monkeypatch.delenv("AUDIOMOD_PV_CHUNK_SLICES")
    prev = E.set_arithmetic(E.ARITH_EXACT)
    try:
        assert E.plan_spans(2, 200000, 1, block=BLOCK, **kw)[0]["slice_end"] == 256
        assert E.plan_spans(96, 200000, 1, block=BLOCK, **kw)[0]["slice_end"] == 512    # 192 rows: wide
        assert E.plan_spans(2000, 200000, 1, block=BLOCK, **kw)[0]["slice_end"] == 32
        E.set_arithmetic(E.ARITH_FAST)
        assert E.plan_spans(2, 200000, 1, block=BLOCK, **kw)[0]["slice_end"] == 512     # fused path at any row count
    finally:
        E.set_arithmetic(prev)


def test_refusals_come_before_any_device_call():
    L = E.lib()
    cfg = E.make_config(2, semitones=4.0, fftsize=2048)
    arr = (E.SpanInfo * 4)()
    plan = L.pv_batch_plan_spans
    assert plan(None, 2, 20000, BLOCK, 1, 1, arr, 4) == -PV_ERR_INVALID_ARG
    assert plan(C.byref(cfg), 0, 20000, BLOCK, 1, 1, arr, 4) == -PV_ERR_INVALID_ARG
    assert plan(C.byref(cfg), 2, 0, BLOCK, 1, 1, arr, 4) == -PV_ERR_INVALID_ARG
    assert plan(C.byref(cfg), 2, 20000, BLOCK, 1, 0, arr, 4) == -PV_ERR_INVALID_ARG
    assert plan(C.byref(cfg), 2, 20000, BLOCK, 1, 1, None, 4) == -PV_ERR_INVALID_ARG
    # writes min(count, max) entries and returns the count
    n = plan(C.byref(cfg), 2, 20000, BLOCK, 1, 1, arr, 2)
    assert n > 4 and arr[1].first_launch == 1 and arr[2].launches == 0
    # a configuration derive refuses: its status
    bad = E.make_config(2, mode=99, semitones=4.0, fftsize=2048)
    assert plan(C.byref(bad), 2, 20000, BLOCK, 1, 1, arr, 4) == -PV_ERR_UNSUPPORTED
    with pytest.raises(E.PvError):
        E.plan_spans(2, 20000, 0, semitones=4.0)
    assert L.pv_batch_run_span(None, 0, 1, None, 0, None, 0, None) == PV_ERR_INVALID_ARG
    assert L.pv_batch_span(None, 0, 1, C.byref(arr[0])) == PV_ERR_INVALID_ARG
    assert L.pv_hostio_staging_bytes(None) == -1
    h = C.c_void_p()
    seg = L.pv_hostio_create_segmented
    assert seg(C.byref(cfg), 4, 20000, BLOCK, 1, 0, 0, 0, C.byref(h)) == PV_ERR_INVALID_ARG     # launches_per_segment 0
    assert seg(C.byref(cfg), 4, 20000, BLOCK, 1, 0, 1, 2, C.byref(h)) == PV_ERR_INVALID_ARG     # no such wire
    assert seg(None, 4, 20000, BLOCK, 1, 0, 1, 0, C.byref(h)) == PV_ERR_INVALID_ARG
    assert seg(C.byref(cfg), 0, 20000, BLOCK, 1, 0, 1, 0, C.byref(h)) == PV_ERR_INVALID_ARG
    with pytest.raises(E.PvError):
        E.HostIO(4, 20000, launches_per_segment=0, semitones=4.0)
    if L.pv_device_count() < 1:
        assert seg(C.byref(cfg), 4, 20000, BLOCK, 1, 0, 1, 0, C.byref(h)) == PV_ERR_NO_DEVICE
        assert not h.value
