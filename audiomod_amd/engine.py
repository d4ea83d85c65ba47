"""Host-side Python mirror of the reference's phase-vocoder interface, over the C ABI.

Everything here calls audiomod_amd/lib/libaudiomod_pv.so (HIP kernels for gfx950 + C++ host
engine, include/audiomod_pv.h).  There is no Python or CPU implementation of the DSP in this
package: if the library is missing or no MI355X is visible, construction fails loudly.

`PhaseVocoder` keeps the method names and call semantics of audiomod::phasevocoder
(reference include/dafx/phasevocoder.h:42-117, src/phasevocoder/phasevocoder.cc:87-183) so the
parity tests read like drives of the reference class.  `Batch` is the device-resident throughput
path (many independent streams), used by bench.py; `MixedBatch` is the same path for streams that differ in length,
pitch and time ratio.  `StreamPool` serves many live streams, each with the
semantics of a `PhaseVocoder`, with one launch sequence per call for all of them.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (AUDIOMOD_PV_LIB: a diagnostic build of the library -- tools/build_variant.sh -- instead of the product's)
LIB_PATH = os.environ.get("AUDIOMOD_PV_LIB") or os.path.join(_HERE, "lib", "libaudiomod_pv.so")

MODES = {"constant": -1, "normal_pitchshift": 0, "gender_change": 1, "formant_pitchshift": 2,
         "vocoder": 3, "vocoder_chord": 4, "time_stretch": 5, "robotic": 6, "whisper": 7,
         "formant_cepstral": 8}  # 8 = extension of this engine (PV_MODE_FORMANT_CEPSTRAL)
CONSTANT, NORMAL_SHIFT, GENDER_CHANGE, FORMANT_PRESERVE = -1, 0, 1, 2
VOCODER_ROSENBERG, VOCODER_CHORD, NORMAL_STRETCH, ROBOTIC, WHISPER = 3, 4, 5, 6, 7
FORMANT_CEPSTRAL = 8
NORMAL_PV, PHASE_LOCKED, INT_RATIO = 0, 1, 2
KERNELS = ("pv_analyze_kernel", "pv_match_kernel", "pv_seq_kernel", "pv_prop_kernel", "pv_synth_kernel",
           "pv_ola_kernel", "pv_cepstral_kernel", "pv_synth_ola_kernel")


class PvError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("time_ratio", C.c_float),
                ("pitch_semitones", C.c_float), ("mode", C.c_int32), ("coremode", C.c_int32),
                ("fftsize", C.c_int32), ("hopsize", C.c_int32)]


class Info(C.Structure):
    _fields_ = [("fftsize", C.c_int32), ("hop_in", C.c_int32), ("hop_out_nominal", C.c_int32),
                ("outbuf_capacity", C.c_int32), ("pitch_scale", C.c_float), ("hs_ratio", C.c_float),
                ("int_ratio", C.c_int32), ("resample", C.c_int32), ("res_num", C.c_uint32), ("res_den", C.c_uint32),
                ("res_filt_len", C.c_int32), ("res_oversample", C.c_int32), ("res_interp", C.c_int32),
                ("slices", C.c_int64), ("bytes_per_slice", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MixedStream(C.Structure):
    _fields_ = [("frames", C.c_int64), ("time_ratio", C.c_float), ("pitch_semitones", C.c_float)]


class SpanInfo(C.Structure):
    _fields_ = [("first_launch", C.c_int32), ("launches", C.c_int32), ("slice_begin", C.c_int64),
                ("slice_end", C.c_int64), ("in_begin", C.c_int64), ("in_end", C.c_int64), ("out_begin", C.c_int64),
                ("out_end", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PoolRange(C.Structure):
    _fields_ = [("min_semitones", C.c_float), ("max_semitones", C.c_float), ("min_time_ratio", C.c_float),
                ("max_time_ratio", C.c_float)]


class BlobDesc(C.Structure):
    _fields_ = [("version", C.c_int32), ("arithmetic", C.c_int32), ("cfg", Config), ("time_ratio", C.c_float),
                ("pitch_semitones", C.c_float), ("slices", C.c_int64), ("pending_frames", C.c_int64),
                ("payload_bytes", C.c_int64), ("total_bytes", C.c_int64)]


class ChainRung(C.Structure):
    _fields_ = [("nc", C.c_int32), ("plain_core", C.c_int32), ("resample", C.c_int32), ("fast", C.c_int32),
                ("wave_bound", C.c_int32), ("reciprocal_wden", C.c_int32)]


class ResampleRung(C.Structure):
    _fields_ = [("resample", C.c_int32), ("res_num", C.c_int32), ("res_den", C.c_int32), ("filt_len", C.c_int32),
                ("oversample", C.c_int32), ("interp", C.c_int32), ("tab_bytes", C.c_int32), ("lds_floats", C.c_int32),
                ("rung", C.c_int32), ("refused", C.c_int32), ("lds_bytes", C.c_int64)]


class PlaneInfo(C.Structure):
    _fields_ = [("slice_begin", C.c_int64), ("slice_end", C.c_int64), ("hs", C.c_int32), ("peak_capacity", C.c_int32),
                ("has_peaks", C.c_int32), ("has_chain", C.c_int32)]


_lib = None


def lib():
    """Load the native library; raise (never fall back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PvError(f"{LIB_PATH} not built: run `make` (or __graft_entry__.build()); there is no fallback path")
    # PyTorch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64; two HIP runtimes in one process
    # cannot both own the GPU.  Loading torch first makes our DT_NEEDED libamdhip64.so.7 resolve to the copy
    # torch already mapped, so tensors and our kernels share one runtime.  Without torch (e.g. the C++
    # drop-in) the library uses /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    fpp = C.POINTER(C.POINTER(C.c_float))
    L.pv_strerror.restype = C.c_char_p
    L.pv_strerror.argtypes = [C.c_int]
    L.pv_last_error.restype = C.c_char_p
    L.pv_device_count.restype = C.c_int
    L.pv_kernel_name.restype = C.c_char_p
    L.pv_kernel_name.argtypes = [C.c_int]
    L.pv_plan_simulate.argtypes = [C.POINTER(Config), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int64, C.POINTER(C.c_int64), C.POINTER(Info)]
    L.pv_plan_whisper_phases.argtypes = [C.c_int64, C.c_void_p]
    L.pv_plan_table.argtypes = [C.POINTER(Config), C.c_int, C.c_void_p, C.c_int64]
    L.pv_plan_table.restype = C.c_int64
    L.pv_create.argtypes = [C.POINTER(Config), C.c_int, C.POINTER(C.c_void_p)]
    L.pv_destroy.argtypes = [C.c_void_p]
    L.pv_feed.argtypes = [C.c_void_p, fpp, C.c_int32]
    L.pv_available.argtypes = [C.c_void_p]
    L.pv_available.restype = C.c_int32
    L.pv_retrieve.argtypes = [C.c_void_p, fpp, C.c_int32]
    L.pv_retrieve.restype = C.c_int32
    L.pv_get_info.argtypes = [C.c_void_p, C.POINTER(Info)]
    L.pv_batch_create.argtypes = [C.POINTER(Config), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int,
                                  C.POINTER(C.c_void_p)]
    L.pv_batch_destroy.argtypes = [C.c_void_p]
    L.pv_batch_out_frames.argtypes = [C.c_void_p]
    L.pv_batch_out_frames.restype = C.c_int64
    L.pv_batch_slices.argtypes = [C.c_void_p]
    L.pv_batch_slices.restype = C.c_int64
    L.pv_batch_launches.argtypes = [C.c_void_p]
    L.pv_batch_launches.restype = C.c_int32
    L.pv_batch_pipelined.argtypes = [C.c_void_p]
    L.pv_batch_pipelined.restype = C.c_int32
    L.pv_batch_get_info.argtypes = [C.c_void_p, C.POINTER(Info)]
    L.pv_batch_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pv_batch_enable_timing.argtypes = [C.c_void_p, C.c_int]
    L.pv_batch_kernel_times.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pv_batch_plan_spans.argtypes = [C.POINTER(Config), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(SpanInfo), C.c_int64]
    L.pv_batch_plan_spans.restype = C.c_int64
    L.pv_batch_span.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SpanInfo)]
    L.pv_batch_run_span.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                    C.c_void_p]
    L.pv_hostio_create_segmented.argtypes = [C.POINTER(Config), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int,
                                             C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.pv_hostio_staging_bytes.argtypes = [C.c_void_p]
    L.pv_hostio_staging_bytes.restype = C.c_int64
    L.pv_hostio_create.argtypes = [C.POINTER(Config), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int, C.c_int32,
                                   C.c_int32, C.POINTER(C.c_void_p)]
    L.pv_hostio_destroy.argtypes = [C.c_void_p]
    L.pv_hostio_out_frames.argtypes = [C.c_void_p]
    L.pv_hostio_out_frames.restype = C.c_int64
    L.pv_hostio_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pv_debug_atan2f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
    L.pv_debug_polar.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
    L.pv_debug_sqrt_sweep.argtypes = [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_int]
    L.pv_debug_chain_census.argtypes = [C.c_int]
    L.pv_debug_chain_census_count.argtypes = [C.c_int] * 6
    L.pv_debug_chain_census_count.restype = C.c_int64
    L.pv_debug_chain_rung.argtypes = [C.POINTER(Config), C.c_int, C.POINTER(ChainRung)]
    L.pv_debug_resample_rung.argtypes = [C.POINTER(Config), C.c_int, C.c_int32, C.POINTER(ResampleRung)]
    L.pv_host_alloc.argtypes = [C.c_size_t]
    L.pv_host_alloc.restype = C.c_void_p
    L.pv_host_free.argtypes = [C.c_void_p]
    L.pv_pool_create.argtypes = [C.POINTER(Config), C.c_int32, C.c_int, C.POINTER(C.c_void_p)]
    L.pv_pool_destroy.argtypes = [C.c_void_p]
    L.pv_pool_capacity.argtypes = [C.c_void_p]
    L.pv_pool_capacity.restype = C.c_int32
    L.pv_pool_open.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.pv_pool_close.argtypes = [C.c_void_p, C.c_int32]
    L.pv_pool_feed.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, fpp, C.c_void_p]
    L.pv_pool_available.argtypes = [C.c_void_p, C.c_int32]
    L.pv_pool_available.restype = C.c_int32
    L.pv_pool_retrieve.argtypes = [C.c_void_p, C.c_int32, fpp, C.c_int32]
    L.pv_pool_retrieve.restype = C.c_int32
    L.pv_pool_get_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Info)]
    L.pv_pool_last_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pv_pool_last_launches.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.pv_pool_plan_feed.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pv_pool_feed_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    L.pv_pool_create_mixed.argtypes = [C.POINTER(Config), C.POINTER(PoolRange), C.c_int32, C.c_int, C.POINTER(C.c_void_p)]
    L.pv_pool_open_with.argtypes = [C.c_void_p, C.c_float, C.c_float, C.POINTER(C.c_int32)]
    L.pv_pool_snapshot_bytes.argtypes = [C.c_void_p, C.c_int32]
    L.pv_pool_snapshot_bytes.restype = C.c_int64
    L.pv_pool_save.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pv_pool_restore.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pv_pool_blob_info.argtypes = [C.c_void_p, C.c_int64, C.POINTER(BlobDesc)]
    i64p = C.POINTER(C.c_int64)
    L.pv_mbatch_layout.argtypes = [C.POINTER(Config), C.POINTER(MixedStream), C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, i64p, i64p]
    L.pv_mbatch_create.argtypes = [C.POINTER(Config), C.POINTER(MixedStream), C.c_int32, C.c_int32, C.c_int32, C.c_int,
                                   C.POINTER(C.c_void_p)]
    L.pv_mbatch_destroy.argtypes = [C.c_void_p]
    L.pv_mbatch_nstreams.argtypes = [C.c_void_p]
    L.pv_mbatch_nstreams.restype = C.c_int32
    for name in ("pv_mbatch_out_frames", "pv_mbatch_in_offset", "pv_mbatch_out_offset"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int32]
        getattr(L, name).restype = C.c_int64
    for name in ("pv_mbatch_in_floats", "pv_mbatch_out_floats"):
        getattr(L, name).argtypes = [C.c_void_p]
        getattr(L, name).restype = C.c_int64
    for name in ("pv_mbatch_launches", "pv_mbatch_kernel_launches"):
        getattr(L, name).argtypes = [C.c_void_p]
        getattr(L, name).restype = C.c_int32
    L.pv_mbatch_get_info.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Info)]
    L.pv_mbatch_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pv_mbatch_redraw.argtypes = [C.c_void_p, C.POINTER(MixedStream)]
    f64p = C.POINTER(C.c_double)
    L.pv_mbatch_last_build_timing.argtypes = [C.c_void_p, f64p, f64p, f64p]
    L.pv_mbatch_debug_descriptors.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_int64]
    L.pv_mbatch_debug_descriptors.restype = C.c_int64
    L.pv_mbatch_pcm_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i64p, i64p]
    L.pv_mbatch_run_pcm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pv_mbatch_run_pcm_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pv_mbatch_debug_pcm_kernel.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pv_debug_pcm_ingest.argtypes =[C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_int]
    L.pv_debug_pcm_egress.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int]
    for name, lead in (("pv_debug_batch", [C.c_int32]), ("pv_debug", []), ("pv_debug_pool", [C.c_int32]),
                       ("pv_debug_mbatch", [C.c_int32])):
        # (the batch's info call takes no stream: its rows share one range)
        getattr(L, name + "_plane_info").argtypes = [C.c_void_p] + ([] if name == "pv_debug_batch" else lead) + [
            C.POINTER(PlaneInfo)]
        getattr(L, name + "_planes").argtypes = [C.c_void_p] + lead + [C.c_int32, C.c_int64] + [C.c_void_p] * 7
    L.pv_debug_batch_chain_runs.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.pv_formant_env_comp.argtypes = [C.c_float, C.c_float, C.POINTER(C.c_float)]
    L.pv_set_formant.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.pv_batch_set_formant.argtypes = [C.c_void_p, C.c_int, C.c_float]
    L.pv_pool_set_formant.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_float]
    L.pv_pool_get_formant.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    L.pv_mbatch_set_formant.argtypes = [C.c_void_p, C.c_void_p]
    L.pv_pool_set_voice.argtypes = [C.c_void_p, C.c_int32, C.c_int]
    L.pv_pool_get_voice.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int)]
    L.pv_mbatch_set_voice.argtypes = [C.c_void_p, C.c_void_p]
    L.pv_debug_whisper_phases.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int]
    # (AUDIOMOD_PV_LIB may name a library built before the carrier setting -- the parent leg of tools/carrier_bench.py --
    # which has none of these; using the setting on it then raises AttributeError)
    if hasattr(L, "pv_pool_set_carrier"):
        L.pv_pool_set_carrier.argtypes = [C.c_void_p, C.c_int32, C.c_int]
        L.pv_pool_get_carrier.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int)]
        L.pv_plan_carrier.argtypes = [C.c_int32, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
        L.pv_debug_carrier.argtypes = [C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int]
    L.pv_set_arithmetic.argtypes = [C.c_int]
    L.pv_get_arithmetic.restype = C.c_int
    _lib = L
    return L


ARITH_FAST, ARITH_EXACT = 0, 1
DESC_WDEN, DESC_OTAB = 0, 1  # pv_mbatch_debug_descriptors (PV_MB_DESC_*)


def set_arithmetic(arith):
    """Process-wide, read at engine creation (include/audiomod_pv.h pv_set_arithmetic): ARITH_FAST (default) lets the
    many-stream batch path fuse / regroup the synthesis side's arithmetic within the 1e-4 RMS contract; ARITH_EXACT keeps
    the reference's operation order everywhere.  Returns the previous setting."""
    L = lib()
    prev = L.pv_get_arithmetic()
    _check(L.pv_set_arithmetic(int(arith)), "pv_set_arithmetic")
    return prev


def get_arithmetic():
    return lib().pv_get_arithmetic()


CENSUS_SETS = ("batch", "pool", "pmix", "mb")  # PV_CENSUS_SET_*: the four sets of the fused kernel
CENSUS_NC = (256, 512, 1024, 2048)


def chain_census(on=True):
    """Clears the process-wide census of the launchers' choices (include/audiomod_pv.h pv_debug_chain_census) and
    switches it on or off."""
    _check(lib().pv_debug_chain_census(1 if on else 0), "pv_debug_chain_census")


def chain_census_read():
    """The non-zero keys of the census as three dicts: fused kernel {(set, nc, plain_core, res, fast): launches},
    slot-table resampler {(set, fast, interpolated): launches}, slot-table analysis {(set, nc, split): launches}; `set`
    is one of CENSUS_SETS."""
    count = lib().pv_debug_chain_census_count
    chain, res, ana = {}, {}, {}
    for i, name in enumerate(CENSUS_SETS):
        for nc in CENSUS_NC:
            for core in (-1, 0, 1, 2, 3):
                for r in (0, 1):
                    for f in (0, 1):
                        n = count(0, i, nc, core, r, f)
                        if n > 0:
                            chain[(name, nc, core, r, f)] = n
            for split in (0, 1):
                n = count(2, i, nc, split, 0, 0)
                if n > 0:
                    ana[(name, nc, split)] = n
        for f in (0, 1):
            for interp in (0, 1):
                n = count(1, i, f, interp, 0, 0)
                if n > 0:
                    res[(name, f, interp)] = n
    return chain, res, ana


PHASE_FORMS = ("ring", "step", "fused", "stream")  # PV_PHASE_FORM_*: the forms of the phase-locked stage


def phase_census_read():
    """The non-zero keys of the census' fourth kind, the phase-locked stage: {(set, form, b): launches} with `set` one
    of CENSUS_SETS ("batch" counts the batch path and the single-stream engine), `form` one of PHASE_FORMS and b the
    ring's depth (4 / 8) or, for "step" and "stream", the peaks one lane holds (1 / 3)."""
    count = lib().pv_debug_chain_census_count
    out = {}
    for i, name in enumerate(CENSUS_SETS):
        for f, form in enumerate(PHASE_FORMS):
            for b in (1, 3, 4, 8):
                n = count(3, i, f, b, 0, 0)
                if n > 0:
                    out[(name, form, b)] = n
    return out


def chain_rung(arith, channels=2, **config):
    """Host only (works without a GPU): the rung of the fused ladder a configuration gets under `arith` (ARITH_FAST /
    ARITH_EXACT), as a dict of nc, plain_core, resample, fast, wave_bound and reciprocal_wden (include/audiomod_pv.h
    pv_debug_chain_rung)."""
    cfg = make_config(channels, **config)
    r = ChainRung()
    _check(lib().pv_debug_chain_rung(C.byref(cfg), int(arith), C.byref(r)), "pv_debug_chain_rung")
    return {k: getattr(r, k) for k, _ in r._fields_}


ANALYSIS_KERNELS = ("generic", "wave", "split", "stream")  # PV_ANA_KERNEL_*
ANALYSIS_NC = (128, 256, 512, 1024, 2048, 4096)


def analysis_census_read():
    """The non-zero keys of the census' sixth kind, the analysis kernel of all four sets: {(set, kernel, nc): launches}
    with `set` one of CENSUS_SETS ("batch" counts the batch path and the single-stream engine), `kernel` one of
    ANALYSIS_KERNELS and nc half the fft size."""
    count = lib().pv_debug_chain_census_count
    out = {}
    for i, name in enumerate(CENSUS_SETS):
        for k, kernel in enumerate(ANALYSIS_KERNELS):
            for nc in ANALYSIS_NC:
                n = count(5, i, k, nc, 0, 0)
                if n > 0:
                    out[(name, kernel, nc)] = n
    return out


CEPSTRAL_KERNELS = ("generic", "wave", "slot")  # PV_CEP_KERNEL_*: the cepstral formant stage's kernels


def cepstral_census_read():
    """The non-zero keys of the census' kind PV_CENSUS_CEPSTRAL, the cepstral formant stage of all four sets: {(set, kernel, nc):
    launches} with `set` one of CENSUS_SETS ("batch" counts the batch path and the single-stream engine, mode
    formant_cepstral and the formant setting alike), `kernel` one of CEPSTRAL_KERNELS and nc half the fft size."""
    count = lib().pv_debug_chain_census_count
    out = {}
    for i, name in enumerate(CENSUS_SETS):
        for k, kernel in enumerate(CEPSTRAL_KERNELS):
            for nc in ANALYSIS_NC:
                n = count(7, i, k, nc, 0, 0)
                if n > 0:
                    out[(name, kernel, nc)] = n
    return out


def formant_env_comp(pitch, formant):
    """Host only: the env_comp (float32) of a stream shifted by `pitch` semitones with the formant setting at `formant`
    semitones (include/audiomod_pv.h "Formant setting"): the pitch scale itself at 0."""
    v = C.c_float(0)
    _check(lib().pv_formant_env_comp(float(pitch), float(formant), C.byref(v)), "pv_formant_env_comp")
    return np.float32(v.value)


def _formant_args(st):
    """(on, value) of the C ABI for a setting given as semitones or None (off)"""
    return (0, 0.0) if st is None else (1, float(st))


RES_RUNGS = ("ref4", "vec8", "vec16", "mfma", "vec2", "vec4")  # PV_RES_RUNG_*: the resampling kernels


def resample_census_read():
    """The non-zero keys of the census' fifth kind, the resampling kernel of all four sets: {(set, rung, interpolated,
    over_64k): launches} with `set` one of CENSUS_SETS ("batch" counts the batch path, the single-stream engine and the
    host-staged engine), `rung` one of RES_RUNGS and over_64k whether the launch asked for more than 64 KB of LDS."""
    count = lib().pv_debug_chain_census_count
    out = {}
    for i, name in enumerate(CENSUS_SETS):
        for r, rung in enumerate(RES_RUNGS):
            for interp in (0, 1):
                for big in (0, 1):
                    n = count(4, i, r, interp, big, 0)
                    if n > 0:
                        out[(name, rung, interp, big)] = n
    return out


def resample_rung(arith, rows, channels=2, **config):
    """Host only (works without a GPU): the resampling kernel a batch of `rows` rows of a configuration gets under
    `arith`, by the launcher's own function (include/audiomod_pv.h pv_debug_resample_rung): a dict of resample, res_num,
    res_den, filt_len, oversample, interp, tab_bytes, lds_floats, rung (a name of RES_RUNGS, None where nothing is
    resampled), lds_bytes, refused and, for a refused configuration, the reason engine creation gives."""
    L = lib()
    cfg = make_config(channels, **config)
    r = ResampleRung()
    st = L.pv_debug_resample_rung(C.byref(cfg), int(arith), int(rows), C.byref(r))
    if st != 0 and not r.refused:
        _check(st, "pv_debug_resample_rung")
    out = {k: getattr(r, k) for k, _ in r._fields_}
    out["rung"] = RES_RUNGS[r.rung] if r.rung >= 0 else None
    out["reason"] = L.pv_last_error().decode() if r.refused else ""
    return out


STEP_INIT, STEP_PROP, STEP_LOCK = 0, 1, 2  # PV_STEP_*


def _plane_info(name, h, lead):
    i = PlaneInfo()
    _check(getattr(lib(), name + "_plane_info")(h, *lead, C.byref(i)), name + "_plane_info")
    return {k: getattr(i, k) for k, _ in i._fields_}


def _planes(name, h, lead, info, channel, t):
    """One slice of one row through the plane tap (include/audiomod_pv.h pv_debug_*_planes), as a dict: mag, phase
    [hs + 1]; with a peak search npk, mode, peaks [npk] and, for a locked step, rot [npk]; with a chain, for any other
    step, outphase [hs].  What the step does not have is None."""
    hs, cap = info["hs"], max(info["peak_capacity"], 1)
    mag, phase = np.zeros(hs + 1, np.float32), np.zeros(hs + 1, np.float32)
    npk, mode = C.c_int32(-1), C.c_int32(-1)
    peaks, rot, outphase = np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(hs, np.float32)
    _check(getattr(lib(), name + "_planes")(h, *lead, int(channel), int(t), mag.ctypes.data, phase.ctypes.data,
                                            C.byref(npk), peaks.ctypes.data, C.byref(mode), rot.ctypes.data,
                                            outphase.ctypes.data), name + "_planes")
    out = dict(mag=mag, phase=phase, npk=None, mode=None, peaks=None, rot=None, outphase=None)
    if info["has_peaks"]:
        n = npk.value
        out.update(npk=n, mode=mode.value, peaks=peaks[:n].copy(), rot=rot[:n].copy() if mode.value == STEP_LOCK else None)
    if info["has_chain"] and not (info["has_peaks"] and mode.value == STEP_LOCK):
        out["outphase"] = outphase
    return out


def _check(st, what):
    if st != 0:
        L = lib()
        raise PvError(f"{what}: {L.pv_strerror(st).decode()} ({L.pv_last_error().decode()})")


def make_config(channels, mode="normal_pitchshift", semitones=0.0, time_ratio=1.0, coremode=1, fftsize=2048,
                sample_rate=48000, hopsize=0):
    m = MODES[mode] if isinstance(mode, str) else int(mode)
    return Config(sample_rate, channels, time_ratio, semitones, m, coremode, fftsize, hopsize)


def plan_simulate(calls, max_slices=1 << 22, **kw):
    """Host planner only (works without a GPU): per-call availability and per-slice increments."""
    L = lib()
    cfg = make_config(**kw)
    n = np.ascontiguousarray(calls, dtype=np.int32)
    avail = np.zeros(len(n), np.int32)
    shift = np.zeros(max_slices, np.int32)
    phase = np.zeros(max_slices, np.int32)
    ns = C.c_int64(0)
    info = Info()
    st = L.pv_plan_simulate(C.byref(cfg), n.ctypes.data, len(n), avail.ctypes.data, shift.ctypes.data,
                            phase.ctypes.data, max_slices, C.byref(ns), C.byref(info))
    _check(st, "pv_plan_simulate")
    k = min(ns.value, max_slices)
    return avail, shift[:k], phase[:k], info.as_dict()


def plan_table(which, max_len=1 << 20, **kw):
    """The planner's window (0), Speex filter table (1) or vocoder carrier (2: first max_len samples); host only."""
    cfg = make_config(**kw)
    out = np.zeros(max_len, np.float32)
    n = lib().pv_plan_table(C.byref(cfg), which, out.ctypes.data, max_len)
    if n < 0:
        _check(int(-n), "pv_plan_table")
    return out[:min(n, max_len)].copy()


def whisper_phases(n):
    """First n phases WHISPER mode draws in a fresh reference process (host only)."""
    out = np.zeros(n, np.float32)
    _check(lib().pv_plan_whisper_phases(n, out.ctypes.data), "pv_plan_whisper_phases")
    return out


VOICES = {"robotic": 0, "whisper": 1}  # PV_VOICE_*
CENSUS_VOICE = 8  # PV_CENSUS_VOICE


def _voice_value(v):
    """a voice as the C ABI takes it: a name of VOICES, or the number itself (passed on unchecked)"""
    return VOICES[v] if isinstance(v, str) else int(v)


def whisper_device_phases(counts, device=0):
    """Diagnostics: the voice setting's generator kernel alone (pv_debug_whisper_phases).  One stream from the fresh
    state, one launch per entry of `counts` drawing that many phases, the state carried on the device between them;
    all phases concatenated, float32.  Equals whisper_phases(sum(counts)) bit for bit."""
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    assert counts.ndim == 1
    out = np.zeros(max(int(counts.sum()), 1), np.float32)
    _check(lib().pv_debug_whisper_phases(counts.ctypes.data, len(counts), out.ctypes.data, device), "pv_debug_whisper_phases")
    return out[:int(counts.sum())]


CARRIERS = {"none": 0, "rosenberg": 1, "chord": 2}  # PV_CARRIER_*


def _carrier_value(c):
    """a carrier as the C ABI takes it: a name of CARRIERS, or the number itself (passed on unchecked)"""
    return CARRIERS[c] if isinstance(c, str) else int(c)


def plan_carrier(sample_rate, carrier, first, count):
    """`count` samples of the vocoder carrier ("rosenberg" / "chord") from absolute sample index `first`: the closed
    form (pv_plan_carrier; host only).  Equals plan_table(2, mode="vocoder" / "vocoder_chord") from `first` on."""
    out = np.zeros(max(int(count), 1), np.float32)
    _check(lib().pv_plan_carrier(int(sample_rate), _carrier_value(carrier), int(first), int(count), out.ctypes.data),
           "pv_plan_carrier")
    return out[:max(int(count), 0)]


def carrier_device(sample_rate, carrier, firsts, counts, device=0):
    """Diagnostics: the carrier setting's generator kernel alone (pv_debug_carrier).  One launch writes the windows
    (firsts[i], counts[i]); all of them concatenated, float32.  Window i equals plan_carrier(sample_rate, carrier,
    firsts[i], counts[i]) bit for bit."""
    firsts = np.ascontiguousarray(firsts, dtype=np.int64)
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    assert firsts.ndim == 1 and counts.shape == firsts.shape
    total = int(counts.astype(np.int64).sum())
    out = np.zeros(max(total, 1), np.float32)
    _check(lib().pv_debug_carrier(int(sample_rate), _carrier_value(carrier), firsts.ctypes.data, counts.ctypes.data,
                                  len(firsts), out.ctypes.data, device), "pv_debug_carrier")
    return out[:total]


def voice_census_read():
    """The non-zero keys of the census' kind PV_CENSUS_VOICE, the generator's launches: {(set, nc): count}."""
    L = lib()
    out = {}
    for si, name in enumerate(("batch", "pool", "pmix", "mb")):
        for nc in (128, 256, 512, 1024, 2048, 4096):
            n = L.pv_debug_chain_census_count(CENSUS_VOICE, si, nc, 0, 0, 0)
            if n > 0:
                out[(name, nc)] = n
    return out


def plan_spans(nstreams, frames, launches_per_span=1, channels=2, block=480, flush=True, **config):
    """Host only (works without a GPU): the spans of Batch(nstreams, frames, ...) cut every `launches_per_span`
    launches, as a list of dicts (include/audiomod_pv.h pv_batch_span_info): first_launch, launches, slice_begin /
    slice_end, in_begin / in_end (input frames of a row the span may read), out_begin / out_end (output frames it
    writes)."""
    cfg = make_config(channels, **config)
    L = lib()
    args = (C.byref(cfg), int(nstreams), int(frames), int(block), 1 if flush else 0, int(launches_per_span))
    n = L.pv_batch_plan_spans(*args, None, 0)
    if n < 0:
        _check(int(-n), "pv_batch_plan_spans")
    arr = (SpanInfo * max(n, 1))()
    got = L.pv_batch_plan_spans(*args, arr, n)
    if got < 0:
        _check(int(-got), "pv_batch_plan_spans")
    return [arr[i].as_dict() for i in range(min(n, got))]


def _pp(rows):
    fp = C.POINTER(C.c_float)
    return (fp * len(rows))(*[r.ctypes.data_as(fp) for r in rows])


class PhaseVocoder:
    """audiomod::phasevocoder with the same constructor arguments and entry points."""

    def __init__(self, sampleRate, numChannels, timeratio, pitchshift, mode=NORMAL_SHIFT, coremode=PHASE_LOCKED,
                 fftsize=2048, hopsize=0, device=0):
        self.L = lib()
        self.cfg = make_config(numChannels, mode, pitchshift, timeratio, coremode, fftsize, sampleRate, hopsize)
        self.channels = numChannels
        self.mode = self.cfg.mode
        self.h = C.c_void_p()
        _check(self.L.pv_create(C.byref(self.cfg), device, C.byref(self.h)), "pv_create")
        self.num_res_ = 0
        self.outready_ = False

    def close(self):
        if getattr(self, "h", None):
            self.L.pv_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def info(self):
        i = Info()
        _check(self.L.pv_get_info(self.h, C.byref(i)), "pv_get_info")
        return i.as_dict()

    def set_formant(self, st):
        """The formant setting for the slices of later calls: semitones the formants move by (0: they stay, whatever
        the pitch does), or None for off.  Modes normal_pitchshift and time_stretch only."""
        _check(self.L.pv_set_formant(self.h, *_formant_args(st)), "pv_set_formant")

    def plane_info(self):
        """Diagnostics: which slices of a row the plane tap can read now, and which planes exist (pv_plane_info)"""
        return _plane_info("pv_debug", self.h, ())

    def planes(self, channel, t):
        """Diagnostics: slice t of a channel's planes (see _planes); waits for the engine's stream"""
        return _planes("pv_debug", self.h, (), self.plane_info(), channel, t)

    # ---- offline interface (modbase_offline)
    def processInData(self, inData):
        x = np.ascontiguousarray(inData, dtype=np.float32)
        assert x.ndim == 2 and x.shape[0] == self.channels
        rows = [x[c] for c in range(self.channels)]
        _check(self.L.pv_feed(self.h, _pp(rows), x.shape[1]), "pv_feed")
        self.num_res_ = self.L.pv_available(self.h)

    def getOutSamples(self):
        return self.num_res_

    def getOutData(self, num_out_samples):
        n = min(num_out_samples, self.num_res_)
        out = np.zeros((self.channels, max(n, 1)), np.float32)
        got = 0
        if n > 0:
            rows = [out[c] for c in range(self.channels)]
            got = self.L.pv_retrieve(self.h, _pp(rows), n)
        self.outready_ = True
        return out[:, :got]

    # ---- real-time interface (modbase)
    def processBlock(self, bufferData):
        """In place on bufferData (float32 [channels, n]); check outputReady() afterwards."""
        assert bufferData.dtype == np.float32 and bufferData.flags.c_contiguous
        n = bufferData.shape[1]
        if self.mode == NORMAL_STRETCH:  # the reference's processBlock ignores this mode (phasevocoder.cc:134-144)
            self.outready_ = True
            return
        rows = [bufferData[c] for c in range(self.channels)]
        _check(self.L.pv_feed(self.h, _pp(rows), n), "pv_feed")
        self.num_res_ = self.L.pv_available(self.h)
        if self.num_res_ >= n:
            self.L.pv_retrieve(self.h, _pp(rows), n)
            self.outready_ = True
        else:
            self.outready_ = False

    def outputReady(self):
        return self.outready_


def run_offline(x, block=480, flush=True, device=0, **kw):
    """The reference CLI's offline loop (main/main.cc:471-510) on the GPU streaming engine."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    ch, frames = x.shape
    cfg = make_config(ch, **kw)
    pv = PhaseVocoder(cfg.sample_rate, ch, cfg.time_ratio, cfg.pitch_semitones, cfg.mode, cfg.coremode, cfg.fftsize,
                      cfg.hopsize, device)
    outs, counts, produced = [], [], 0
    for i in range(0, frames, block):
        pv.processInData(x[:, i:i + block])
        got = pv.getOutSamples()
        outs.append(pv.getOutData(got))
        counts.append(got)
        produced += got
    if flush:
        z = np.zeros((ch, block), np.float32)
        while produced < frames:
            pv.processInData(z)
            got = pv.getOutSamples()
            y = pv.getOutData(got)
            counts.append(got)
            w = got if frames - produced > got else frames - produced
            outs.append(y[:, :w])
            produced += w
    pv.close()
    return np.concatenate(outs, axis=1), counts


def run_realtime(x, block=480, device=0, **kw):
    """The reference's processBlock/outputReady loop (main/main.cc:561-572)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    ch, frames = x.shape
    cfg = make_config(ch, **kw)
    pv = PhaseVocoder(cfg.sample_rate, ch, cfg.time_ratio, cfg.pitch_semitones, cfg.mode, cfg.coremode, cfg.fftsize,
                      cfg.hopsize, device)
    outs, counts = [], []
    for i in range(0, frames, block):
        blk = np.ascontiguousarray(x[:, i:i + block]).copy()
        pv.processBlock(blk)
        if pv.outputReady():
            outs.append(blk)
            counts.append(blk.shape[1])
        else:
            counts.append(-1)
    pv.close()
    out = np.concatenate(outs, axis=1) if outs else np.zeros((ch, 0), np.float32)
    return out, counts


class Batch:
    """nstreams independent streams, device-resident in and out (torch CUDA tensors)."""

    def __init__(self, nstreams, frames, channels=2, block=480, flush=True, device=0, **kw):
        self.L = lib()
        self.cfg = make_config(channels, **kw)
        self.nstreams, self.frames, self.channels, self.device = nstreams, frames, channels, device
        self.h = C.c_void_p()
        _check(self.L.pv_batch_create(C.byref(self.cfg), nstreams, frames, block, 1 if flush else 0, device,
                                      C.byref(self.h)), "pv_batch_create")
        self.out_frames = self.L.pv_batch_out_frames(self.h)
        self.slices = self.L.pv_batch_slices(self.h)
        self.launches = self.L.pv_batch_launches(self.h)
        self.pipelined = bool(self.L.pv_batch_pipelined(self.h))  # chain kernel on a second stream (overlapped)

    def close(self):
        if getattr(self, "h", None):
            self.L.pv_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def info(self):
        i = Info()
        _check(self.L.pv_batch_get_info(self.h, C.byref(i)), "pv_batch_get_info")
        return i.as_dict()

    def set_formant(self, st):
        """The formant setting (see PhaseVocoder.set_formant), one value for every stream, for the launches enqueued
        after the call; returns self."""
        _check(self.L.pv_batch_set_formant(self.h, *_formant_args(st)), "pv_batch_set_formant")
        return self

    def plane_info(self):
        """Diagnostics: which slices of a row the plane tap can read now, and which planes exist (pv_plane_info)"""
        return _plane_info("pv_debug_batch", self.h, ())

    def planes(self, stream, channel, t):
        """Diagnostics: slice t of the planes of a stream's channel (see _planes); waits for the device"""
        return _planes("pv_debug_batch", self.h, (int(stream),), self.plane_info(), channel, t)

    def chain_runs(self, launch):
        """Diagnostics, host only: (runs, warm-up entries) of the fused kernel's run lists for launch `launch` (0 ...
        self.launches - 1), as creation laid them out (pv_debug_batch_chain_runs); launches nothing"""
        runs, warm = C.c_int32(0), C.c_int32(0)
        _check(self.L.pv_debug_batch_chain_runs(self.h, int(launch), C.byref(runs), C.byref(warm)),
               "pv_debug_batch_chain_runs")
        return runs.value, warm.value

    def alloc_out(self):
        import torch
        return torch.empty((self.nstreams, self.channels, self.out_frames), dtype=torch.float32,
                           device=f"cuda:{self.device}")

    def run(self, d_in, d_out=None, stream=None):
        """d_in: torch float32 CUDA tensor [nstreams, channels, frames], contiguous.  Asynchronous."""
        import torch
        assert d_in.is_cuda and d_in.dtype == torch.float32 and d_in.is_contiguous()
        assert tuple(d_in.shape) == (self.nstreams, self.channels, self.frames)
        if d_out is None:
            d_out = self.alloc_out()
        assert d_out.is_cuda and d_out.is_contiguous() and tuple(d_out.shape) == (self.nstreams, self.channels,
                                                                                 self.out_frames)
        s = stream if stream is not None else torch.cuda.current_stream(d_in.device)
        _check(self.L.pv_batch_run(self.h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                   C.c_void_p(s.cuda_stream)), "pv_batch_run")
        return d_out

    def span(self, first, n):
        """What launches [first, first + n) cover per row (a dict, see plan_spans)."""
        i = SpanInfo()
        _check(self.L.pv_batch_span(self.h, int(first), int(n), C.byref(i)), "pv_batch_span")
        return i.as_dict()

    def run_span(self, first, n, d_in_win, d_out_win=None, stream=None):
        """Runs launches [first, first + n) on windows of the rows.  d_in_win: float32 CUDA tensor [nstreams, channels,
        in_pitch] whose rows hold input frames [in_begin, in_end) of span(first, n) from offset 0; d_out_win
        [nstreams, channels, out_pitch] receives output frames [out_begin, out_end) likewise (allocated when None).
        Pitches are multiples of 4.  first == 0 starts afresh; any other span must follow the previous one.
        Asynchronous; both windows may be reused in stream order afterwards.  The spans of a job, concatenated, are
        run()'s output bit for bit.  enable_timing() does not cover spans."""
        import torch
        sp = self.span(first, n)
        assert d_in_win.is_cuda and d_in_win.dtype == torch.float32 and d_in_win.is_contiguous()
        assert tuple(d_in_win.shape[:2]) == (self.nstreams, self.channels) and d_in_win.dim() == 3
        if d_out_win is None:
            pitch = max((sp["out_end"] - sp["out_begin"] + 3) // 4 * 4, 4)
            d_out_win = torch.empty((self.nstreams, self.channels, pitch), dtype=torch.float32, device=d_in_win.device)
        assert d_out_win.is_cuda and d_out_win.dtype == torch.float32 and d_out_win.is_contiguous()
        assert tuple(d_out_win.shape[:2]) == (self.nstreams, self.channels) and d_out_win.dim() == 3
        s = stream if stream is not None else torch.cuda.current_stream(d_in_win.device)
        _check(self.L.pv_batch_run_span(self.h, int(first), int(n), C.c_void_p(d_in_win.data_ptr()),
                                        int(d_in_win.shape[2]), C.c_void_p(d_out_win.data_ptr()),
                                        int(d_out_win.shape[2]), C.c_void_p(s.cuda_stream)), "pv_batch_run_span")
        return d_out_win

    def enable_timing(self, every=1):
        """every = 0/False: off; n: HIP events around the kernels of every n-th chunk (of run(), not of run_span())."""
        _check(self.L.pv_batch_enable_timing(self.h, int(every)), "pv_batch_enable_timing")

    def kernel_times(self):
        """{kernel: (total_ms, launches)} since enable_timing; synchronise the stream first."""
        ms = (C.c_double * len(KERNELS))()
        n = (C.c_int64 * len(KERNELS))()
        _check(self.L.pv_batch_kernel_times(self.h, ms, n), "pv_batch_kernel_times")
        return {KERNELS[k]: (ms[k], n[k]) for k in range(len(KERNELS))}


def _mixed_streams(streams):
    """(frames, semitones, time_ratio) tuples as the C ABI's array"""
    arr = (MixedStream * max(len(streams), 1))()
    for i, (frames, semitones, time_ratio) in enumerate(streams):
        arr[i] = MixedStream(int(frames), float(time_ratio), float(semitones))
    return arr


def mbatch_layout(streams, channels=2, block=480, flush=True, **config):
    """Host only (works without a GPU): how MixedBatch packs `streams`, a list of (frames, semitones, time_ratio).
    Returns a dict of out_frames, slices, in_offsets, out_offsets (one entry per stream) and in_floats, out_floats."""
    cfg = make_config(channels, **config)
    n = len(streams)
    a = [np.zeros(max(n, 1), np.int64) for _ in range(4)]
    fin, fout = C.c_int64(0), C.c_int64(0)
    _check(lib().pv_mbatch_layout(C.byref(cfg), _mixed_streams(streams), n, block, 1 if flush else 0, a[0].ctypes.data,
                                  a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, C.byref(fin), C.byref(fout)),
           "pv_mbatch_layout")
    keys = ("out_frames", "slices", "in_offsets", "out_offsets")
    out = {k: [int(x) for x in v[:n]] for k, v in zip(keys, a)}
    out.update(in_floats=fin.value, out_floats=fout.value)
    return out


class MixedBatch:
    """Streams of different length, pitch and time ratio on the device-resident throughput path (include/audiomod_pv.h
    pv_mbatch_*).  `streams` is a list of (frames, semitones, time_ratio); every other setting is shared.  Stream i's
    output is bit for bit what Batch(1, frames_i, semitones=..., time_ratio=..., ...) writes.  Input and output are
    packed 1-D float32 CUDA tensors: stream i's [channels, frames_i] at in_offsets[i] (torch.cat of the flattened
    clips), its [channels, out_frames_i] at out_offsets[i] (split())."""

    def __init__(self, streams, channels=2, block=480, flush=True, device=0, **config):
        self.L = lib()
        config.pop("semitones", None), config.pop("time_ratio", None)  # per stream
        self.cfg = make_config(channels, **config)
        self.streams = [(int(f), float(s), float(r)) for f, s, r in streams]
        self.channels, self.device = channels, device
        self.h = C.c_void_p()
        _check(self.L.pv_mbatch_create(C.byref(self.cfg), _mixed_streams(self.streams), len(self.streams), block,
                                       1 if flush else 0, device, C.byref(self.h)), "pv_mbatch_create")
        self._refresh()

    def _refresh(self):
        """the layout the object has now (after creation and after every redraw)"""
        n = self.L.pv_mbatch_nstreams(self.h)
        self.out_frames = [self.L.pv_mbatch_out_frames(self.h, i) for i in range(n)]
        self.in_offsets = [self.L.pv_mbatch_in_offset(self.h, i) for i in range(n)]
        self.out_offsets = [self.L.pv_mbatch_out_offset(self.h, i) for i in range(n)]
        self.in_floats = self.L.pv_mbatch_in_floats(self.h)
        self.out_floats = self.L.pv_mbatch_out_floats(self.h)
        self.launches = self.L.pv_mbatch_launches(self.h)  # launch groups per run
        self.kernel_launches = self.L.pv_mbatch_kernel_launches(self.h)  # kernels per run

    def redraw(self, streams):
        """New (frames, semitones, time_ratio) for every stream, in place: afterwards the object is what
        MixedBatch(streams, ...) with the constructor's other arguments would be -- out_frames, the offsets and the
        buffer sizes are refreshed, and pack / alloc_out / run / split follow the new layout.  Raises PvError on a
        refusal, after which the object is unchanged and usable.  Synchronises the device."""
        streams = [(int(f), float(s), float(r)) for f, s, r in streams]
        if len(streams) != len(self.streams):
            raise PvError("MixedBatch.redraw: %d streams for an object of %d" % (len(streams), len(self.streams)))
        _check(self.L.pv_mbatch_redraw(self.h, _mixed_streams(streams)), "pv_mbatch_redraw")
        self.streams = streams
        self._refresh()

    def set_formant(self, values):
        """The formant setting per stream: a list of semitones with None (or NaN) for off, or None for all off.
        Synchronises the device; kernel_launches is refreshed.  A redraw() resets every stream to off."""
        if values is None:
            _check(self.L.pv_mbatch_set_formant(self.h, None), "pv_mbatch_set_formant")
        else:
            if len(values) != len(self.streams):
                raise PvError("MixedBatch.set_formant: %d values for an object of %d" % (len(values), len(self.streams)))
            v = np.array([np.nan if x is None else float(x) for x in values], np.float32)
            _check(self.L.pv_mbatch_set_formant(self.h, v.ctypes.data), "pv_mbatch_set_formant")
        self._refresh()

    def set_voice(self, voices):
        """The voice per stream: a list of "robotic" / "whisper", or None for all robotic (pv_mbatch_set_voice; an
        object of mode robotic).  Stream i with the whisper voice equals Batch(1, frames_i, mode="whisper", ...)."""
        if voices is None:
            _check(self.L.pv_mbatch_set_voice(self.h, None), "pv_mbatch_set_voice")
        else:
            if len(voices) != len(self.streams):
                raise PvError("MixedBatch.set_voice: %d values for an object of %d" % (len(voices), len(self.streams)))
            v = np.array([_voice_value(x) for x in voices], np.int32)
            _check(self.L.pv_mbatch_set_voice(self.h, v.ctypes.data), "pv_mbatch_set_voice")
        self._refresh()

    def last_build_timing(self):
        """The last creation or redraw in microseconds: dict(plan_us, host_us, device_us) -- planning, the other host
        work up to and including the uploads, the wait for the device build (0 after a creation)."""
        v = [C.c_double(0) for _ in range(3)]
        _check(self.L.pv_mbatch_last_build_timing(self.h, *[C.byref(x) for x in v]), "pv_mbatch_last_build_timing")
        return dict(plan_us=v[0].value, host_us=v[1].value, device_us=v[2].value)

    def debug_descriptors(self, i, which):
        """Diagnostics: stream i's denominators (which = DESC_WDEN) or resampler output table (DESC_OTAB) as a uint32
        array, copied back from the device."""
        size = self.L.pv_mbatch_debug_descriptors(self.h, int(i), int(which), None, 0)
        _check(int(-size) if size < 0 else 0, "pv_mbatch_debug_descriptors")
        out = np.zeros(size // 4, np.uint32)
        if size:
            got = self.L.pv_mbatch_debug_descriptors(self.h, int(i), int(which), out.ctypes.data, size)
            _check(int(-got) if got < 0 else 0, "pv_mbatch_debug_descriptors")
            assert got == size
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.pv_mbatch_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def info(self, i):
        inf = Info()
        _check(self.L.pv_mbatch_get_info(self.h, int(i), C.byref(inf)), "pv_mbatch_get_info")
        return inf.as_dict()

    def plane_info(self, i):
        """Diagnostics: which slices of stream i the plane tap can read now, and which planes exist (pv_plane_info)"""
        return _plane_info("pv_debug_mbatch", self.h, (int(i),))

    def planes(self, i, channel, t):
        """Diagnostics: slice t of the planes of stream i's channel (see _planes); waits for the device"""
        return _planes("pv_debug_mbatch", self.h, (int(i),), self.plane_info(i), channel, t)

    def alloc_out(self):
        import torch
        return torch.empty(max(self.out_floats, 1), dtype=torch.float32, device=f"cuda:{self.device}")[:self.out_floats]

    def pack(self, clips):
        """The packed input tensor of a list of [channels, frames_i] arrays or tensors (host or device)."""
        import torch
        parts = []
        for (frames, _, _), x in zip(self.streams, clips):
            t = x.to(torch.float32) if torch.is_tensor(x) else torch.tensor(np.asarray(x), dtype=torch.float32)
            assert tuple(t.shape) == (self.channels, frames)
            parts.append(t.reshape(-1).to(f"cuda:{self.device}"))
        return torch.cat(parts)

    def run(self, d_in, d_out=None, stream=None):
        """d_in: packed 1-D float32 CUDA tensor of in_floats elements.  Asynchronous."""
        import torch
        assert d_in.is_cuda and d_in.dtype == torch.float32 and d_in.is_contiguous() and d_in.dim() == 1
        assert d_in.numel() == self.in_floats
        if d_out is None:
            d_out = self.alloc_out()
        assert d_out.is_cuda and d_out.dtype == torch.float32 and d_out.is_contiguous() and d_out.dim() == 1
        assert d_out.numel() == self.out_floats
        s = stream if stream is not None else torch.cuda.current_stream(d_in.device)
        _check(self.L.pv_mbatch_run(self.h, C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()),
                                    C.c_void_p(s.cuda_stream)), "pv_mbatch_run")
        return d_out

    def split(self, d_out):
        """[channels, out_frames_i] views of the packed output, one per stream."""
        return [d_out[o:o + self.channels * f].view(self.channels, f) for o, f in zip(self.out_offsets, self.out_frames)]

    # -- the PCM wire (include/audiomod_pv.h pv_mbatch_run_pcm): clips as WAV files hold them, converted on the device
    def _bits(self, bits):
        """None (16 bits for every clip), one depth for all, or one per stream: the list and the C ABI's argument"""
        n = len(self.streams)
        if bits is None:
            return [16] * n, None
        lst = [int(bits)] * n if np.isscalar(bits) else [int(b) for b in bits]
        assert len(lst) == n
        return lst, (C.c_int32 * n)(*lst)

    def pcm_layout(self, bits=None):
        """Host only: dict of in_offsets, out_offsets (bytes, one per stream; multiples of 16) and in_bytes, out_bytes
        for input depths `bits` (8 / 16 / 24 / 32 per stream; output is always int16)."""
        n = len(self.streams)
        _, arr = self._bits(bits)
        a = [np.zeros(n, np.int64) for _ in range(2)]
        nin, nout = C.c_int64(0), C.c_int64(0)
        _check(self.L.pv_mbatch_pcm_layout(self.h, arr, a[0].ctypes.data, a[1].ctypes.data, C.byref(nin), C.byref(nout)),
               "pv_mbatch_pcm_layout")
        return dict(in_offsets=[int(x) for x in a[0]], out_offsets=[int(x) for x in a[1]], in_bytes=nin.value,
                    out_bytes=nout.value)

    def pack_pcm_host(self, clips, bits=None):
        """The PCM input buffer as a numpy uint8 array: clips are integer arrays [frames_i][channels] -- uint8 values
        for 8 bits, int16 for 16, sign-extended int32 for 24 and 32 -- written interleaved, little-endian, at the
        layout's offsets (the padding between clips is zero)."""
        lst, _ = self._bits(bits)
        lay = self.pcm_layout(bits)
        buf = np.zeros(lay["in_bytes"], np.uint8)
        for (frames, _, _), x, b, off in zip(self.streams, clips, lst, lay["in_offsets"]):
            buf[off:off + frames * self.channels * (b // 8)] = pcm_bytes(np.asarray(x).reshape(frames, self.channels), b)
        return buf

    def pack_pcm(self, clips, bits=None):
        """pack_pcm_host's buffer as a 1-D uint8 CUDA tensor."""
        import torch
        return torch.from_numpy(self.pack_pcm_host(clips, bits)).to(f"cuda:{self.device}")

    def alloc_pcm_out(self):
        import torch
        n = self.pcm_layout()["out_bytes"]
        return torch.zeros(max(n, 16), dtype=torch.uint8, device=f"cuda:{self.device}")[:n]

    def run_pcm(self, d_pcm_in, bits=None, d_pcm_out=None, stream=None):
        """d_pcm_in: 1-D uint8 CUDA tensor in pcm_layout(bits)'s layout; returns the 1-D uint8 output tensor (int16
        samples, split_pcm()).  Ingest kernel, the run, egress kernel on one stream.  Asynchronous."""
        import torch
        _, arr = self._bits(bits)
        lay = self.pcm_layout(bits)
        assert d_pcm_in.is_cuda and d_pcm_in.dtype == torch.uint8 and d_pcm_in.is_contiguous() and d_pcm_in.dim() == 1
        assert d_pcm_in.numel() == lay["in_bytes"]
        if d_pcm_out is None:
            d_pcm_out = self.alloc_pcm_out()
        assert d_pcm_out.is_cuda and d_pcm_out.dtype == torch.uint8 and d_pcm_out.is_contiguous() and d_pcm_out.dim() == 1
        assert d_pcm_out.numel() == lay["out_bytes"]
        s = stream if stream is not None else torch.cuda.current_stream(d_pcm_in.device)
        _check(self.L.pv_mbatch_run_pcm(self.h, arr, C.c_void_p(d_pcm_in.data_ptr()), C.c_void_p(d_pcm_out.data_ptr()),
                                        C.c_void_p(s.cuda_stream)), "pv_mbatch_run_pcm")
        return d_pcm_out

    def split_pcm(self, d_pcm_out):
        """int16 [out_frames_i, channels] views of run_pcm's (or, for a numpy array, run_pcm_host's) output."""
        offs = self.pcm_layout()["out_offsets"]
        if isinstance(d_pcm_out, np.ndarray):
            return [d_pcm_out[o:o + 2 * self.channels * f].view("<i2").reshape(f, self.channels)
                    for o, f in zip(offs, self.out_frames)]
        import torch
        return [d_pcm_out[o:o + 2 * self.channels * f].view(torch.int16).view(f, self.channels)
                for o, f in zip(offs, self.out_frames)]

    def run_pcm_host(self, h_pcm_in, bits=None, h_pcm_out=None):
        """Host buffers (numpy uint8 arrays or CPU uint8 tensors; page-locked ones are copied at PCIe rate): one copy
        in, the run, one copy out, synchronous.  Returns h_pcm_out (a numpy array unless one was passed)."""
        _, arr = self._bits(bits)
        lay = self.pcm_layout(bits)
        if h_pcm_out is None:
            h_pcm_out = np.zeros(max(lay["out_bytes"], 1), np.uint8)[:lay["out_bytes"]]

        def ptr(x, nbytes):
            if isinstance(x, np.ndarray):
                assert x.dtype == np.uint8 and x.flags.c_contiguous and x.size == nbytes
                return x.ctypes.data
            assert (not x.is_cuda) and x.is_contiguous() and x.numel() * x.element_size() == nbytes
            return x.data_ptr()

        _check(self.L.pv_mbatch_run_pcm_host(self.h, arr, C.c_void_p(ptr(h_pcm_in, lay["in_bytes"])),
                                             C.c_void_p(ptr(h_pcm_out, lay["out_bytes"]))), "pv_mbatch_run_pcm_host")
        return h_pcm_out


def pcm_bytes(x, bits):
    """Integer samples (uint8 values for 8 bits, int16 for 16, sign-extended 24- or 32-bit values otherwise) as the
    little-endian byte string of a WAV file's data chunk, in the array's own (C) order: a flat uint8 array."""
    x = np.ascontiguousarray(x)
    if bits == 8:
        return x.astype(np.uint8).reshape(-1)
    if bits == 16:
        return x.astype("<i2").reshape(-1).view(np.uint8)
    b = x.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)
    if bits == 24:
        return np.ascontiguousarray(b[:, :3]).reshape(-1)
    assert bits == 32
    return b.reshape(-1)


def debug_pcm_ingest(x, bits, device=0):
    """Diagnostics: the ingest kernel on one clip.  x: integer samples [frames][channels] (see pcm_bytes); returns the
    float32 [channels][frames] the kernel writes."""
    x = np.asarray(x)
    frames, ch = x.shape
    raw = np.ascontiguousarray(pcm_bytes(x, bits))
    out = np.zeros((ch, frames), np.float32)
    _check(lib().pv_debug_pcm_ingest(raw.ctypes.data, bits, ch, frames, out.ctypes.data, device), "pv_debug_pcm_ingest")
    return out


def debug_pcm_egress(planar, device=0):
    """Diagnostics: the egress kernel on one clip.  planar: float32 [channels][frames]; returns int16 [frames][channels]."""
    planar = np.ascontiguousarray(planar, np.float32)
    ch, frames = planar.shape
    out = np.zeros((frames, ch), np.int16)
    _check(lib().pv_debug_pcm_egress(planar.ctypes.data, ch, frames, out.ctypes.data, device), "pv_debug_pcm_egress")
    return out


class HostIO:
    """nstreams independent streams whose input and output live in HOST memory (what the reference's callers hold:
    main/main.cc:152-162,484-491), float32 or int16 on the wire; groups of streams are staged through the GPU with
    copy-in, kernels and copy-out overlapped (include/audiomod_pv.h pv_hostio_*).

    launches_per_segment=k stages by TIME instead (pv_hostio_create_segmented): one batch of all streams run in
    segments of k launches through three window slots, so the device holds three windows of audio whatever `frames`
    is; streams_per_group is then unused.  None (the default) is the grouped object.  Same bits either way."""

    def __init__(self, nstreams, frames, channels=2, block=480, flush=True, device=0, streams_per_group=16,
                 wire="f32", launches_per_segment=None, **kw):
        self.L = lib()
        self.cfg = make_config(channels, **kw)
        self.nstreams, self.frames, self.channels = nstreams, frames, channels
        self.wire = {"f32": 0, "i16": 1}[wire]
        self.dtype = np.float32 if self.wire == 0 else np.int16
        self.h = C.c_void_p()
        self.launches_per_segment = launches_per_segment
        if launches_per_segment is None:
            _check(self.L.pv_hostio_create(C.byref(self.cfg), nstreams, frames, block, 1 if flush else 0, device,
                                           streams_per_group, self.wire, C.byref(self.h)), "pv_hostio_create")
        else:
            _check(self.L.pv_hostio_create_segmented(C.byref(self.cfg), nstreams, frames, block, 1 if flush else 0,
                                                     device, int(launches_per_segment), self.wire, C.byref(self.h)),
                   "pv_hostio_create_segmented")
        self.out_frames = self.L.pv_hostio_out_frames(self.h)
        self._pinned = []

    def staging_bytes(self):
        """Device bytes of the staging buffers (grouped: three groups' whole streams; segmented: three windows)."""
        return self.L.pv_hostio_staging_bytes(self.h)

    def pinned(self, shape):
        """numpy array of this job's wire type in page-locked host memory (freed with the object)"""
        n = int(np.prod(shape)) * np.dtype(self.dtype).itemsize
        p = self.L.pv_host_alloc(max(n, 1))
        if not p:
            raise PvError("pv_host_alloc failed")
        self._pinned.append(p)
        buf = (C.c_char * max(n, 1)).from_address(p)
        return np.frombuffer(buf, dtype=self.dtype, count=int(np.prod(shape))).reshape(shape)

    def run(self, host_in, host_out=None):
        assert host_in.dtype == self.dtype and host_in.flags.c_contiguous
        assert tuple(host_in.shape) == (self.nstreams, self.channels, self.frames)
        if host_out is None:
            host_out = self.pinned((self.nstreams, self.channels, self.out_frames))
        assert host_out.dtype == self.dtype and host_out.flags.c_contiguous
        _check(self.L.pv_hostio_run(self.h, host_in.ctypes.data, host_out.ctypes.data), "pv_hostio_run")
        return host_out

    def close(self):
        if getattr(self, "h", None):
            self.L.pv_hostio_destroy(self.h)
            self.h = None
        for p in getattr(self, "_pinned", []):
            self.L.pv_host_free(p)
        self._pinned = []

    def __del__(self):
        self.close()


def blob_info(blob):
    """Host only (works without a GPU): validates a blob of StreamPool.save() and describes it (pv_pool_blob_info): format
    version, the stream's configuration, the slot's pitch and time ratio, the arithmetic setting, slices processed,
    frames of pending output and the payload size.  Raises PvError for anything that is not a valid blob."""
    b = bytes(blob)
    d = BlobDesc()
    _check(lib().pv_pool_blob_info(C.c_char_p(b), len(b), C.byref(d)), "pv_pool_blob_info")
    out = {k: getattr(d, k) for k, _ in d._fields_ if k != "cfg"}
    out["cfg"] = {k: getattr(d.cfg, k) for k, _ in Config._fields_}
    return out


class StreamPool:
    """Up to `capacity` independent live streams of one configuration (include/audiomod_pv.h pv_pool_*).  A slot
    behaves bit for bit like a PhaseVocoder / pv_engine of the same configuration fed the same blocks; one feed()
    serves any subset of the open slots with one launch sequence.  One host thread per pool.

    pitch_range=(lo, hi) and / or ratio_range=(lo, hi) make a mixed pool (pv_pool_create_mixed): each slot then takes
    its own pitch / time ratio within them at open(semitones=..., time_ratio=...), and behaves like a PhaseVocoder
    created with those values.  A range not given is the configuration's own value."""

    def __init__(self, capacity, channels=2, device=0, pitch_range=None, ratio_range=None, **config):
        self.L = lib()
        self.cfg = make_config(channels, **config)
        self.channels = channels
        self.device = device
        self.h = C.c_void_p()
        if pitch_range is None and ratio_range is None:
            _check(self.L.pv_pool_create(C.byref(self.cfg), int(capacity), device, C.byref(self.h)), "pv_pool_create")
        else:
            lo, hi = pitch_range if pitch_range is not None else (self.cfg.pitch_semitones,) * 2
            rlo, rhi = ratio_range if ratio_range is not None else (self.cfg.time_ratio,) * 2
            rng = PoolRange(lo, hi, rlo, rhi)
            _check(self.L.pv_pool_create_mixed(C.byref(self.cfg), C.byref(rng), int(capacity), device, C.byref(self.h)),
                   "pv_pool_create_mixed")
        self.capacity = self.L.pv_pool_capacity(self.h)

    def close_pool(self):
        if getattr(self, "h", None):
            self.L.pv_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close_pool()

    def open(self, semitones=None, time_ratio=None, voice=None, carrier=None):
        """A fresh stream in the lowest free slot, at the given pitch / time ratio (default: the configuration's);
        returns the slot.  voice: set_voice() for the new slot, carrier: set_carrier() (a pool of mode robotic)."""
        s = self._open(semitones, time_ratio)
        try:
            if voice is not None:
                self.set_voice(s, voice)
            if carrier is not None:
                self.set_carrier(s, carrier)
        except Exception:
            self.close(s)
            raise
        return s

    def _open(self, semitones, time_ratio):
        s = C.c_int32(-1)
        if semitones is None and time_ratio is None:
            _check(self.L.pv_pool_open(self.h, C.byref(s)), "pv_pool_open")
        else:
            st = self.cfg.pitch_semitones if semitones is None else semitones
            tr = self.cfg.time_ratio if time_ratio is None else time_ratio
            _check(self.L.pv_pool_open_with(self.h, float(tr), float(st), C.byref(s)), "pv_pool_open_with")
        return s.value

    def close(self, slot):
        """Frees the slot; its pending output is discarded."""
        _check(self.L.pv_pool_close(self.h, int(slot)), "pv_pool_close")

    def feed(self, blocks):
        """blocks: {slot: float32 array [channels, n]} (n may differ per slot, and be 0)."""
        slots = np.array(list(blocks.keys()), np.int32)
        arrs = [np.ascontiguousarray(blocks[int(s)], dtype=np.float32) for s in slots]
        for a in arrs:
            assert a.ndim == 2 and a.shape[0] == self.channels
        n = np.array([a.shape[1] for a in arrs], np.int32)
        rows = [a[c] for a in arrs for c in range(self.channels)]
        _check(self.L.pv_pool_feed(self.h, len(slots), slots.ctypes.data, _pp(rows) if rows else None,
                                   n.ctypes.data), "pv_pool_feed")

    def plan_feed(self, slots, n):
        """Host only: the frames each of `slots` would have available after a feed of n[i] frames (for a slot without
        pending output: what feed_device returns for it); changes nothing.  int32 array."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        n = np.ascontiguousarray(n, dtype=np.int32)
        assert slots.ndim == 1 and n.shape == slots.shape
        out = np.zeros(len(slots), np.int32)
        _check(self.L.pv_pool_plan_feed(self.h, len(slots), slots.ctypes.data, n.ctypes.data, out.ctypes.data),
               "pv_pool_plan_feed")
        return out

    def feed_device(self, slots, x, n=None, out=None, stream=None):
        """feed() and retrieve-all for `slots` with input and output on the device (pv_pool_feed_device).  x: torch
        tensor [len(slots), channels, in_pitch], float32 or int16, on the pool's device, contiguous; entry i holds n[i]
        frames of slots[i] from offset 0 (n defaults to the pitch).  out: [len(slots), channels, out_pitch] of x's type
        (allocated from plan_feed when None).  Returns (out, out_frames): out_frames[i] frames of out[i] are valid, bit
        for bit what feed() + retrieve() deliver.  Asynchronous: enqueued on `stream` (default: the current one) and
        not waited for; x and out may be reused in stream order."""
        import torch
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        assert slots.ndim == 1
        assert x.is_cuda and x.device.index == self.device and x.is_contiguous() and x.dim() == 3
        assert x.dtype in (torch.float32, torch.int16) and tuple(x.shape[:2]) == (len(slots), self.channels)
        wire = 0 if x.dtype == torch.float32 else 1
        n = np.full(len(slots), x.shape[2], np.int32) if n is None else np.ascontiguousarray(n, dtype=np.int32)
        assert n.shape == slots.shape
        if out is None:
            pitch = max(int(self.plan_feed(slots, n).max(initial=0)), 1)
            out = torch.empty((len(slots), self.channels, pitch), dtype=x.dtype, device=x.device)
        assert out.is_cuda and out.device == x.device and out.is_contiguous() and out.dtype == x.dtype
        assert out.dim() == 3 and tuple(out.shape[:2]) == (len(slots), self.channels)
        s = stream if stream is not None else torch.cuda.current_stream(x.device)
        frames = np.zeros(len(slots), np.int32)
        _check(self.L.pv_pool_feed_device(self.h, len(slots), slots.ctypes.data, n.ctypes.data, C.c_void_p(x.data_ptr()),
                                          int(x.shape[2]), C.c_void_p(out.data_ptr()), int(out.shape[2]), wire,
                                          frames.ctypes.data, C.c_void_p(s.cuda_stream)), "pv_pool_feed_device")
        return out, frames

    def available(self, slot):
        return self.L.pv_pool_available(self.h, int(slot))

    def retrieve(self, slot, n):
        """Up to n frames of the slot's output, float32 [channels, got]."""
        out = np.zeros((self.channels, max(int(n), 1)), np.float32)
        got = 0
        if n > 0:
            got = self.L.pv_pool_retrieve(self.h, int(slot), _pp([out[c] for c in range(self.channels)]), int(n))
            if got < 0:
                raise PvError(f"pv_pool_retrieve: slot {slot} is not open")
        return out[:, :got]

    def info(self, slot):
        i = Info()
        _check(self.L.pv_pool_get_info(self.h, int(slot), C.byref(i)), "pv_pool_get_info")
        return i.as_dict()

    def plane_info(self, slot):
        """Diagnostics: which slices of a slot the plane tap can read now, and which planes exist (pv_plane_info)"""
        return _plane_info("pv_debug_pool", self.h, (int(slot),))

    def planes(self, slot, channel, t):
        """Diagnostics: slice t of the planes of a slot's channel (see _planes); waits for the pool's stream"""
        return _planes("pv_debug_pool", self.h, (int(slot),), self.plane_info(slot), channel, t)

    def last_timing(self):
        """(host_us, wait_us) of the last feed(): host work up to the wait for the device, and that wait (0 after a
        feed_device(), which does not wait)."""
        h, w = C.c_double(), C.c_double()
        _check(self.L.pv_pool_last_timing(self.h, C.byref(h), C.byref(w)), "pv_pool_last_timing")
        return h.value, w.value

    def snapshot_bytes(self, slot):
        """The exact size of the slot's blob in its current state."""
        n = self.L.pv_pool_snapshot_bytes(self.h, int(slot))
        if n < 0:
            raise PvError(f"pv_pool_snapshot_bytes: slot {slot} is not open")
        return n

    def save(self, slot):
        """The slot's stream as a blob (bytes) that restore() of a compatible pool -- this one included -- continues bit
        for bit (pv_pool_save).  A list of slots gives a list of blobs, saved with one kernel and one copy.  Leaves the
        slots as they are."""
        many = not np.isscalar(slot)
        slots = np.ascontiguousarray(slot if many else [slot], dtype=np.int32)
        cap = np.array([max(self.L.pv_pool_snapshot_bytes(self.h, int(s)), 1) for s in slots], np.int64)
        bufs = [np.empty(int(n), np.uint8) for n in cap]
        ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
        got = np.zeros(len(bufs), np.int64)
        _check(self.L.pv_pool_save(self.h, len(slots), slots.ctypes.data, ptrs, cap.ctypes.data, got.ctypes.data),
               "pv_pool_save")
        blobs = [b[:int(n)].tobytes() for b, n in zip(bufs, got)]
        return blobs if many else blobs[0]

    def restore(self, blob):
        """Opens a fresh slot (the lowest free one) that continues the stream saved in `blob`; returns the slot
        (pv_pool_restore).  A list of blobs gives a list of slots, all or none."""
        many = not isinstance(blob, (bytes, bytearray, memoryview))
        blobs = [bytes(b) for b in (blob if many else [blob])]
        ptrs = (C.c_char_p * len(blobs))(*blobs)
        sizes = np.array([len(b) for b in blobs], np.int64)
        slots = np.full(len(blobs), -1, np.int32)
        _check(self.L.pv_pool_restore(self.h, len(blobs), ptrs, sizes.ctypes.data, slots.ctypes.data), "pv_pool_restore")
        return [int(s) for s in slots] if many else int(slots[0])

    def fork(self, slot):
        """A second slot of this pool with the slot's history: both return the same bits from here on (a blob does not
        carry the formant setting, so the new slot gets the slot's setting here)."""
        s = self.restore(self.save(int(slot)))
        st = self.get_formant(slot)
        if st is not None:  # (a restored slot has the setting off, and a pool outside its scope refuses the call)
            self.set_formant(s, st)
        return s

    def set_formant(self, slot, st):
        """The slot's formant setting (see PhaseVocoder.set_formant) for the slices of later feeds: semitones, or None
        for off.  Host state only; a slot opens, and is restored, with the setting off."""
        _check(self.L.pv_pool_set_formant(self.h, int(slot), *_formant_args(st)), "pv_pool_set_formant")

    def get_formant(self, slot):
        """The slot's formant setting: semitones, or None when off."""
        on, v = C.c_int(0), C.c_float(0)
        _check(self.L.pv_pool_get_formant(self.h, int(slot), C.byref(on), C.byref(v)), "pv_pool_get_formant")
        return float(v.value) if on.value else None

    def set_voice(self, slot, voice):
        """The slot's voice, "robotic" or "whisper" (pv_pool_set_voice): a pool of mode robotic, a slot that has
        processed no slice yet.  A whisper slot is from then on bit for bit a PhaseVocoder of mode whisper."""
        _check(self.L.pv_pool_set_voice(self.h, int(slot), _voice_value(voice)), "pv_pool_set_voice")

    def get_voice(self, slot):
        v = C.c_int(0)
        _check(self.L.pv_pool_get_voice(self.h, int(slot), C.byref(v)), "pv_pool_get_voice")
        return {n: k for k, n in VOICES.items()}[v.value]

    def set_carrier(self, slot, carrier):
        """The slot's carrier, "none", "rosenberg" or "chord" (pv_pool_set_carrier): a pool of mode robotic, a slot that
        has processed no slice yet.  A carrier slot is from then on bit for bit a PhaseVocoder of mode vocoder /
        vocoder_chord with the slot's pitch and time ratio."""
        _check(self.L.pv_pool_set_carrier(self.h, int(slot), _carrier_value(carrier)), "pv_pool_set_carrier")

    def get_carrier(self, slot):
        v = C.c_int(0)
        _check(self.L.pv_pool_get_carrier(self.h, int(slot), C.byref(v)), "pv_pool_get_carrier")
        return {n: k for k, n in CARRIERS.items()}[v.value]

    def last_launches(self):
        """Kernels launched by the last feed() or feed_device(); 1 after a save() or restore() of any number of slots."""
        n = C.c_int32(0)
        _check(self.L.pv_pool_last_launches(self.h, C.byref(n)), "pv_pool_last_launches")
        return n.value
