"""Mixed batch, re-drawing in place (include/audiomod_pv.h pv_mbatch_redraw): the C ABI and what needs no device."""
import ctypes as C
import inspect
import os
import re

from audiomod_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pv_mbatch_redraw", "pv_mbatch_last_build_timing", "pv_mbatch_debug_descriptors")
PV_ERR_INVALID_ARG = 1


def test_header_and_library_have_the_redraw():
    with open(os.path.join(ROOT, "include", "audiomod_pv.h")) as f:
        hdr = f.read()
    L = E.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert hasattr(L, name), name
    assert "#define PV_MB_DESC_WDEN" in hdr and "#define PV_MB_DESC_OTAB" in hdr


def test_null_arguments_are_invalid_without_a_device():
    L = E.lib()
    s = E._mixed_streams([(1000, 4.0, 1.0)])
    assert L.pv_mbatch_redraw(None, s) == PV_ERR_INVALID_ARG
    assert L.pv_last_error().decode().startswith("mixed batch")
    # (a non-null object cannot exist without a device; the null stream list is refused before the object is read)
    fake = C.create_string_buffer(8)
    assert L.pv_mbatch_redraw(C.cast(fake, C.c_void_p), None) == PV_ERR_INVALID_ARG
    assert L.pv_mbatch_last_build_timing(None, None, None, None) == PV_ERR_INVALID_ARG
    assert L.pv_mbatch_debug_descriptors(None, 0, 0, None, 0) == -PV_ERR_INVALID_ARG


def test_python_interface():
    assert list(inspect.signature(E.MixedBatch.redraw).parameters) == ["self", "streams"]
    assert list(inspect.signature(E.MixedBatch.last_build_timing).parameters) == ["self"]
    assert (E.DESC_WDEN, E.DESC_OTAB) == (0, 1)
