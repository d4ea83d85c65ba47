"""PCM wire of the mixed batch (include/audiomod_pv.h pv_mbatch_pcm_layout / pv_mbatch_run_pcm / pv_mbatch_run_pcm_host
and the two debug entries): declarations, exports, the byte layout against a numpy restatement and the refusals that
come before any device call.  The layout belongs to an object, and an object needs a device: without one the layout
checks assert the no-device status instead (tests/test_mbatch_pcm_gpu.py repeats them where a device is certain)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from audiomod_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pv_mbatch_pcm_layout", "pv_mbatch_run_pcm", "pv_mbatch_run_pcm_host", "pv_debug_pcm_ingest",
                "pv_debug_pcm_egress")
PV_ERR_INVALID_ARG, PV_ERR_NO_DEVICE = 1, 3
STREAMS = [(1, -12.0, 1.0), (7, 0.0, 1.0), (8, 4.0, 1.0), (9, 4.0, 1.0), (479, -5.0, 1.0), (2049, 0.0, 1.0),
           (4097, 7.0, 1.0), (9000, 12.0, 0.75)]
CFG = dict(fftsize=512, coremode=1)


def expected_layout(frames, out_frames, channels, bits):
    """the layout restated: clips in order, each rounded up to the next multiple of 16 bytes"""
    def offsets(sizes):
        offs, at = [], 0
        for s in sizes:
            offs.append(at)
            at += (s + 15) // 16 * 16
        return offs, at
    ins, nin = offsets([f * channels * (b // 8) for f, b in zip(frames, bits)])
    outs, nout = offsets([f * channels * 2 for f in out_frames])
    return dict(in_offsets=ins, out_offsets=outs, in_bytes=nin, out_bytes=nout)


def test_header_and_library_have_the_pcm_wire():
    with open(os.path.join(ROOT, "include", "audiomod_pv.h")) as f:
        hdr = f.read()
    L = E.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(L, name), name
    for method in ("pcm_layout", "pack_pcm", "run_pcm", "split_pcm", "run_pcm_host"):
        assert callable(getattr(E.MixedBatch, method)), method


def test_null_handles_and_bad_depths_are_refused_before_any_device_call():
    L = E.lib()
    n = C.c_int64(0)
    buf = np.zeros(64, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    assert L.pv_mbatch_pcm_layout(None, None, None, None, C.byref(n), C.byref(n)) == PV_ERR_INVALID_ARG
    assert L.pv_mbatch_run_pcm(None, None, p, p, None) == PV_ERR_INVALID_ARG
    assert L.pv_mbatch_run_pcm_host(None, None, p, p) == PV_ERR_INVALID_ARG
    f = np.zeros(64, np.float32)
    for bits in (0, 12, 64, -16):
        assert L.pv_debug_pcm_ingest(buf.ctypes.data, bits, 1, 4, f.ctypes.data, 0) == PV_ERR_INVALID_ARG, bits
    assert L.pv_debug_pcm_ingest(buf.ctypes.data, 16, 0, 4, f.ctypes.data, 0) == PV_ERR_INVALID_ARG
    assert L.pv_debug_pcm_ingest(None, 16, 1, 4, f.ctypes.data, 0) == PV_ERR_INVALID_ARG
    assert L.pv_debug_pcm_egress(f.ctypes.data, 1, -1, buf.ctypes.data, 0) == PV_ERR_INVALID_ARG
    assert L.pv_debug_pcm_egress(None, 2, 4, buf.ctypes.data, 0) == PV_ERR_INVALID_ARG


def _object(channels):
    """a mixed batch of STREAMS, or None (after asserting the status) where there is no device"""
    if E.lib().pv_device_count() >= 1:
        return E.MixedBatch(STREAMS, channels=channels, **CFG)
    cfg = E.make_config(channels, **CFG)
    h = C.c_void_p()
    st = E.lib().pv_mbatch_create(C.byref(cfg), E._mixed_streams(STREAMS), len(STREAMS), 480, 1, 0, C.byref(h))
    assert st == PV_ERR_NO_DEVICE and not h.value
    return None


@pytest.mark.parametrize("channels", [1, 2, 3])
def test_layout_is_the_restated_one(channels):
    mb = _object(channels)
    if mb is None:
        return
    frames = [f for f, _, _ in STREAMS]
    cycle = [(16, 8, 24, 32)[i % 4] for i in range(len(STREAMS))]
    for bits in (None, 8, 16, 24, 32, cycle):
        lst = [16] * len(STREAMS) if bits is None else [bits] * len(STREAMS) if isinstance(bits, int) else bits
        lay = mb.pcm_layout(bits)
        assert lay == expected_layout(frames, mb.out_frames, channels, lst), bits
        assert all(o % 16 == 0 for o in lay["in_offsets"] + lay["out_offsets"])
        assert lay["in_bytes"] % 16 == 0 and lay["out_bytes"] % 16 == 0
        assert lay["in_offsets"] == sorted(lay["in_offsets"]) and lay["out_offsets"] == sorted(lay["out_offsets"])
    # every output pointer may be NULL
    assert mb.L.pv_mbatch_pcm_layout(mb.h, None, None, None, None, None) == 0


def test_a_bad_depth_is_refused_on_a_real_object():
    mb = _object(2)
    if mb is None:
        return
    n = len(STREAMS)
    buf = np.zeros(64, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    for bad in (0, 12, 20, 64):
        bits = (C.c_int32 * n)(*([16] * (n - 1) + [bad]))
        assert mb.L.pv_mbatch_pcm_layout(mb.h, bits, None, None, None, None) == PV_ERR_INVALID_ARG
        assert "bits per sample" in mb.L.pv_last_error().decode()
        assert mb.L.pv_mbatch_run_pcm(mb.h, bits, p, p, None) == PV_ERR_INVALID_ARG
        assert mb.L.pv_mbatch_run_pcm_host(mb.h, bits, p, p) == PV_ERR_INVALID_ARG
