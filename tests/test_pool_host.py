"""Stream pool (include/audiomod_pv.h pv_pool_*): the C ABI and its checks that come before any device call, so
they run on a machine without a GPU as well."""
import ctypes as C
import os
import re

import pytest

from audiomod_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pv_pool_create", "pv_pool_destroy", "pv_pool_capacity", "pv_pool_open", "pv_pool_close",
                "pv_pool_feed", "pv_pool_available", "pv_pool_retrieve", "pv_pool_get_info")
PV_ERR_INVALID_ARG, PV_ERR_UNSUPPORTED = 1, 2


def test_header_and_library_have_the_pool():
    with open(os.path.join(ROOT, "include", "audiomod_pv.h")) as f:
        hdr = f.read()
    assert "typedef struct pv_pool pv_pool;" in hdr
    L = E.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(L, name), name


def _create(capacity, channels=2, **kw):
    cfg = E.make_config(channels, **kw)
    h = C.c_void_p()
    st = E.lib().pv_pool_create(C.byref(cfg), capacity, 0, C.byref(h))
    if st == 0:
        E.lib().pv_pool_destroy(h)
    return st


@pytest.mark.parametrize("kw", [
    dict(mode="vocoder"), dict(mode="vocoder_chord"), dict(mode="whisper"), dict(mode="constant"),
    dict(mode="formant_cepstral", semitones=4.0), dict(semitones=4.0, fftsize=256), dict(semitones=4.0, fftsize=8192),
], ids=["vocoder", "vocoder_chord", "whisper", "constant", "cepstral", "fft256", "fft8192"])
def test_out_of_scope_is_unsupported(kw):
    assert _create(4, **kw) == PV_ERR_UNSUPPORTED
    assert E.lib().pv_last_error().decode().startswith("stream pool")


def test_bad_capacity_is_invalid():
    assert _create(0, semitones=4.0) == PV_ERR_INVALID_ARG
    assert _create(-3, semitones=4.0) == PV_ERR_INVALID_ARG
    assert _create(32768, channels=2, semitones=4.0) == PV_ERR_INVALID_ARG  # 65536 rows
    assert _create(65536, channels=1, semitones=4.0) == PV_ERR_INVALID_ARG


def test_null_handles_are_invalid():
    L = E.lib()
    assert L.pv_pool_capacity(None) == -1
    assert L.pv_pool_available(None, 0) == -1
    assert L.pv_pool_close(None, 0) == PV_ERR_INVALID_ARG
    assert L.pv_pool_feed(None, 0, None, None, None) == PV_ERR_INVALID_ARG


def test_no_device_no_pool():
    if E.lib().pv_device_count() >= 1:
        pytest.skip("a gfx950 device is present")
    with pytest.raises(E.PvError, match="no gfx950"):
        E.StreamPool(4, channels=2, semitones=4.0)
