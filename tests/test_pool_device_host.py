"""The stream pool's device-resident feed, host side (no GPU): the C ABI has pv_pool_plan_feed and pv_pool_feed_device,
both refuse a NULL pool, and include/audiomod_pv.h declares them."""
import ctypes
import os
import re

from audiomod_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pv_pool_plan_feed", "pv_pool_feed_device")
PV_ERR_INVALID_ARG = 1


def test_library_exports_the_symbols():
    L = ctypes.CDLL(E.LIB_PATH)
    for n in SYMBOLS:
        assert hasattr(L, n), f"{n} not exported"


def test_header_declares_them():
    text = open(os.path.join(ROOT, "include", "audiomod_pv.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(pv_[a-z_0-9]+)\s*\(", hdr))
    for n in SYMBOLS:
        assert n in names, f"{n} not declared in include/audiomod_pv.h"
    assert re.search(r"PV_ERR_INVALID_ARG\s*=\s*%d\b" % PV_ERR_INVALID_ARG, hdr)


def test_null_pool_is_an_invalid_argument():
    L = E.lib()
    slots = (ctypes.c_int32 * 1)(0)
    n = (ctypes.c_int32 * 1)(480)
    out = (ctypes.c_int32 * 1)(-5)
    assert L.pv_pool_plan_feed(None, 1, slots, n, out) == PV_ERR_INVALID_ARG
    assert L.pv_pool_feed_device(None, 1, slots, n, None, 480, None, 480, 0, out, None) == PV_ERR_INVALID_ARG
    assert L.pv_pool_feed_device(None, 0, None, None, None, 0, None, 0, 1, None, None) == PV_ERR_INVALID_ARG
    assert out[0] == -5  # nothing written
