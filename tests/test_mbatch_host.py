"""Mixed batch (include/audiomod_pv.h pv_mbatch_*): the C ABI, the packing against the planner and the checks that come
before any device call.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from audiomod_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pv_mbatch_layout", "pv_mbatch_create", "pv_mbatch_destroy", "pv_mbatch_nstreams", "pv_mbatch_out_frames",
                "pv_mbatch_in_offset", "pv_mbatch_out_offset", "pv_mbatch_in_floats", "pv_mbatch_out_floats",
                "pv_mbatch_launches", "pv_mbatch_get_info", "pv_mbatch_run")
PV_ERR_INVALID_ARG, PV_ERR_UNSUPPORTED, PV_ERR_NO_DEVICE = 1, 2, 3

# (frames, semitones, time_ratio): a clip shorter than one frame, a stream that does not resample beside ones that do,
# +-12 st (direct tables) beside interpolated ones, two streams of equal length at different pitches
STREAMS = [(1, -12.0, 1.0), (479, -5.0, 1.0), (4097, 0.0, 1.0), (9000, 4.0, 1.0), (24000, 7.0, 0.75), (24000, 12.0, 1.5)]
CFG = dict(fftsize=512, coremode=1)


def test_header_and_library_have_the_mixed_batch():
    with open(os.path.join(ROOT, "include", "audiomod_pv.h")) as f:
        hdr = f.read()
    assert "typedef struct pv_mbatch_stream {" in hdr and "typedef struct pv_mbatch pv_mbatch;" in hdr
    L = E.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(L, name), name


def _planner(frames, block, flush, **kw):
    """(out_frames, slices) of one stream driven the way run_offline drives the engine: `block`-frame calls over the
    input, everything available retrieved after each; then, with flush, zero blocks until `frames` outputs exist, the
    result truncated to `frames`."""
    data = [min(block, frames - i) for i in range(0, frames, block)]
    if not flush:
        avail, shift, _, _ = E.plan_simulate(data, **kw)
        return int(avail.sum()), len(shift)
    extra = 64
    while True:
        avail, _, _, _ = E.plan_simulate(data + [block] * extra, **kw)
        done = np.nonzero(np.cumsum(avail.astype(np.int64)) >= frames)[0]
        if len(done) and done[0] < len(avail):
            ncalls = max(int(done[0]) + 1, len(data))  # the input is always fed whole
            break
        extra *= 2
        assert extra < 1 << 20
    avail, shift, _, _ = E.plan_simulate((data + [block] * extra)[:ncalls], **kw)
    assert avail.sum() >= frames
    # what the input's own calls return is kept whole (a stretch may give more than `frames`); only the flush truncates
    return max(frames, int(avail[:len(data)].sum())), len(shift)


@pytest.mark.parametrize("flush", [True, False], ids=["flush", "noflush"])
@pytest.mark.parametrize("block", [480, 64])
def test_layout_is_the_planners(block, flush):
    lay = E.mbatch_layout(STREAMS, channels=2, block=block, flush=flush, **CFG)
    want = [_planner(f, block, flush, channels=2, semitones=s, time_ratio=r, **CFG) for f, s, r in STREAMS]
    assert lay["out_frames"] == [w[0] for w in want]
    assert lay["slices"] == [w[1] for w in want]
    frames = [f for f, _, _ in STREAMS]
    assert lay["in_offsets"] == [2 * sum(frames[:i]) for i in range(len(frames))]
    assert lay["out_offsets"] == [2 * sum(lay["out_frames"][:i]) for i in range(len(frames))]
    assert lay["in_floats"] == 2 * sum(frames)
    assert lay["out_floats"] == 2 * sum(lay["out_frames"])


def _layout_status(streams, n=None, block=480, cfg=True, channels=2, **kw):
    c = E.make_config(channels, **kw)
    arr = E._mixed_streams(streams) if streams is not None else None
    fin, fout = C.c_int64(0), C.c_int64(0)
    return E.lib().pv_mbatch_layout(C.byref(c) if cfg else None, arr, len(streams) if n is None else n, block, 1, None,
                                    None, None, None, C.byref(fin), C.byref(fout))


def _create_status(streams, n=None, block=480, out=True, channels=2, **kw):
    c = E.make_config(channels, **kw)
    h = C.c_void_p()
    st = E.lib().pv_mbatch_create(C.byref(c), E._mixed_streams(streams), len(streams) if n is None else n, block, 1, 0,
                                  C.byref(h) if out else None)
    if st == 0:
        E.lib().pv_mbatch_destroy(h)
    return st


@pytest.mark.parametrize("kw", [
    dict(mode="vocoder"), dict(mode="vocoder_chord"), dict(mode="whisper"), dict(mode="constant"),
    dict(mode="formant_cepstral"), dict(fftsize=256), dict(fftsize=8192),
], ids=["vocoder", "chord", "whisper", "constant", "cepstral", "fft256", "fft8192"])
def test_out_of_scope_is_unsupported(kw):
    for status in (_layout_status, _create_status):
        assert status(STREAMS, **kw) == PV_ERR_UNSUPPORTED
        assert E.lib().pv_last_error().decode().startswith("mixed batch")


def test_too_many_rows_is_unsupported():
    assert _layout_status([(1000, 0.0, 1.0)] * 4, channels=16384, fftsize=2048) == PV_ERR_UNSUPPORTED
    assert E.lib().pv_last_error().decode().startswith("mixed batch")


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("streams,kw", [
    (STREAMS, dict(n=0)),
    (STREAMS, dict(n=-3)),
    (STREAMS, dict(block=0)),
    (STREAMS[:2] + [(0, 4.0, 1.0)], {}),
    (STREAMS[:2] + [(-5, 4.0, 1.0)], {}),
    (STREAMS[:2] + [(1000, NAN, 1.0)], {}),
    (STREAMS[:2] + [(1000, 4.0, NAN)], {}),
    (STREAMS[:2] + [(1000, INF, 1.0)], {}),
    (None, dict(n=3)),
    (STREAMS, dict(cfg=False)),
], ids=["no_streams", "negative_streams", "block0", "frames0", "negative_frames", "nan_pitch", "nan_ratio", "inf_pitch",
        "null_streams", "null_cfg"])
def test_bad_arguments_are_invalid(streams, kw):
    assert _layout_status(streams, fftsize=2048, **kw) == PV_ERR_INVALID_ARG
    if streams is not None and kw.get("cfg", True):
        assert _create_status(streams, fftsize=2048, **{k: v for k, v in kw.items() if k != "cfg"}) == PV_ERR_INVALID_ARG


def test_null_handle_is_invalid():
    assert _create_status(STREAMS, out=False, **CFG) == PV_ERR_INVALID_ARG
    L = E.lib()
    assert L.pv_mbatch_nstreams(None) == -1 and L.pv_mbatch_launches(None) == -1
    assert L.pv_mbatch_out_frames(None, 0) == -1 and L.pv_mbatch_in_floats(None) == -1
    assert L.pv_mbatch_run(None, None, None, None) == PV_ERR_INVALID_ARG
    assert L.pv_mbatch_get_info(None, 0, None) == PV_ERR_INVALID_ARG


def test_refused_stream_is_named_by_index():
    # (ten octaves up: the engine takes +60 st at this size, so that is no refusal to test with)
    streams = STREAMS[:3] + [(9000, 120.0, 1.0)] + STREAMS[4:]
    one = E.make_config(2, semitones=120.0, fftsize=2048)
    want = E.lib().pv_plan_simulate(C.byref(one), None, 0, None, None, None, 0, None, None)
    assert want != 0  # the engine itself refuses it
    for status in (_layout_status, _create_status):
        assert status(streams, fftsize=2048) == want
        msg = E.lib().pv_last_error().decode()
        assert msg.startswith("mixed batch") and "stream 3" in msg, msg


def test_cfg_own_pitch_and_ratio_are_ignored():
    a = E.mbatch_layout(STREAMS, semitones=0.0, time_ratio=1.0, **CFG)
    b = E.mbatch_layout(STREAMS, semitones=60.0, time_ratio=3.0, **CFG)
    assert a == b


def test_valid_create_needs_the_device():
    st = _create_status(STREAMS, **CFG)
    assert st == (0 if E.lib().pv_device_count() >= 1 else PV_ERR_NO_DEVICE), E.lib().pv_last_error()
    if st:
        with pytest.raises(E.PvError, match="no gfx950"):
            E.MixedBatch(STREAMS, **CFG)
