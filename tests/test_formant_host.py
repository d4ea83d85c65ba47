"""The formant setting without a GPU (include/audiomod_pv.h "Formant setting"): the six entry points exist, the host-only
pv_formant_env_comp is the documented arithmetic -- the pitch scale's bits with the knob at 0 -- and refuses what it
must, and the oracle's plane trace holds the magnitudes BEFORE the cepstral stage (mode formant_cepstral traces what
normal_pitchshift traces), which is what tests/test_formant_gpu.py builds its expected planes on."""
import os
import re

import numpy as np
import pytest

from audiomod_amd import engine as E
from audiomod_amd import signals
from oracle import oracle_py as O
from tests.helpers import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pv_formant_env_comp", "pv_set_formant", "pv_batch_set_formant", "pv_pool_set_formant",
                "pv_pool_get_formant", "pv_mbatch_set_formant")
PV_ERR_INVALID_ARG = 1


def test_header_and_library_export_the_entry_points():
    with open(os.path.join(ROOT, "include", "audiomod_pv.h")) as f:
        header = f.read()
    L = E.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert getattr(L, name) is not None
    assert re.search(r"^#define PV_CENSUS_CEPSTRAL 7\b", header, re.M)


@pytest.mark.parametrize("pitch", [4.0, -4.0, 7.0, -7.0, 12.0])
def test_knob_at_zero_is_the_pitch_scale(pitch):
    _, _, _, info = E.plan_simulate([480], max_slices=64, channels=2, semitones=pitch, fftsize=2048)
    want = np.float32(info["pitch_scale"])
    got = E.formant_env_comp(pitch, 0.0)
    assert got.view(np.uint32) == want.view(np.uint32), (pitch, got, want)


@pytest.mark.parametrize("pitch,formant", [(4.0, -3.0), (-5.0, 2.0), (4.0, 4.5), (0.0, 3.0), (0.0, -6.0), (4.0, 4.0),
                                           (-12.0, 48.0), (11.5, -48.0), (0.0, 0.0)])
def test_env_comp_is_the_documented_formula(pitch, formant):
    def scale(st):   # float quotient, double pow, stored float -- as derive() makes the pitch scale
        st = np.float32(st)
        return np.float32(1.0) if st == 0 else np.float32(np.power(np.float64(2.0), np.float64(st / np.float32(12))))
    want = np.float32(scale(pitch) / scale(formant))
    got = E.formant_env_comp(pitch, formant)
    assert got.view(np.uint32) == want.view(np.uint32), (pitch, formant, got, want)
    if pitch == formant:
        assert got == np.float32(1.0)


@pytest.mark.parametrize("pitch,formant", [(0.0, float("nan")), (0.0, float("inf")), (0.0, -float("inf")),
                                           (0.0, 48.001), (0.0, -49.0), (float("nan"), 0.0), (float("inf"), 0.0)])
def test_env_comp_refuses(pitch, formant):
    import ctypes as C
    v = C.c_float(-1.0)
    assert E.lib().pv_formant_env_comp(pitch, formant, C.byref(v)) == PV_ERR_INVALID_ARG
    assert v.value == -1.0   # a refused call writes nothing
    assert E.lib().pv_formant_env_comp(0.0, 0.0, None) == PV_ERR_INVALID_ARG


@pytest.mark.parametrize("fft,pitch", [(2048, 4.0), (512, -4.0)])
def test_oracle_trace_is_before_the_cepstral_stage(fft, pitch):
    x = signals.voice(6000, 2, seed=3)
    _, _, plain = O.run_offline(x, planes=True, mode="normal_pitchshift", semitones=pitch, fftsize=fft)
    _, _, cep = O.run_offline(x, planes=True, mode="formant_cepstral", semitones=pitch, fftsize=fft)
    assert plain["slices"] == cep["slices"] and plain["planes"]["mag"].shape == cep["planes"]["mag"].shape
    assert plain["planes"]["mag"].shape[0] == 2 * plain["slices"]   # one step per (slice, channel)
    assert bits_equal(plain["planes"]["mag"], cep["planes"]["mag"])
    # ... and the stage itself changes them: the oracle's function on a traced plane
    m = plain["planes"]["mag"][7].copy()
    O.lib().pvo_formant_shift(fft, m.ctypes.data, float(E.formant_env_comp(pitch, 0.0)))
    assert not bits_equal(m, plain["planes"]["mag"][7])
