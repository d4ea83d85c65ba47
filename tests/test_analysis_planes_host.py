"""What the analysis-plane signals do to the oracle, step by step (CPU only).

tests/analysis_signals.py makes the inputs; this file asserts on the oracle's plane trace
(oracle_py.Oracle.plane_trace) that each of them reaches the situation tests/test_analysis_planes_gpu.py relies on, with
literals per fft size.  None is a skip: a signal that stops reaching its situation fails here first.

situation(name) condenses stream 0's trace of a case into the figures the literals below are about; what they mean is
said where they are computed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import analysis_signals as A
from tests.test_phase_forms_host import list_capacity, run_lengths


def situation(name, j=0):
    c = A.BY_NAME[name]
    _, _, info = A.oracle(name, j)
    p, fft, hs = info["planes"], c.fft, c.fft // 2
    steps, flush = len(p["npk"]), info["flush_step"]
    all_in, none_in, sound = A.pass_census(p, fft)
    mixed = ~all_in & ~none_in
    s = sound[:, None]
    nz = (p["re"] != 0) | (p["im"] != 0)
    with np.errstate(under="ignore", over="ignore"):
        sq = p["re"] * p["re"] + p["im"] * p["im"]   # float32, as the conversion squares them
    tiny = np.float32(2.0 ** -126)
    comp = max(float(np.abs(p["re"]).max()), float(np.abs(p["im"]).max()))
    k = p["npk"]
    return dict(
        steps=steps, flush=flush,
        # passes of frames with sound in them: all bins in range / some / none; frames with a pass of the first kind
        # beside one that is not; frames without sound
        p_in=int((all_in & s).sum()), p_mixed=int((mixed & s).sum()), p_out=int((none_in & s).sum()),
        f_split=int((all_in.any(axis=1) & (~all_in).any(axis=1) & sound).sum()), f_silent=int((~sound).sum()),
        # bins with a non-zero component whose sum of squares is subnormal / zero; bins with a magnitude
        sub=int((nz & (sq > 0) & (sq < tiny)).sum()), zsq=int((nz & (sq == 0)).sum()), mags=int((p["mag"] > 0).sum()),
        top=round(float(np.log2(comp)), 1) if comp > 0 else None,
        finite=bool(np.isfinite(p["mag"]).all() and np.isfinite(A.oracle(name, j)[0]).all()),
        kmin=int(k[:flush].min()), kmax=int(k.max()), odd=int((k % 2 == 1).sum()), even=int((k % 2 == 0).sum()),
        k0=int((k == 0).sum()), k1=int((k == 1).sum()), modes=run_lengths(p["mode"]))


def peak_lists(name, j=0):
    p = A.oracle(name, j)[2]["planes"]
    return [tuple(p["peaks"][t, :p["npk"][t]]) for t in range(len(p["npk"]))]


def full_frames(name):
    """the steps whose frame lies wholly inside the input (before the flush pads it with zeros)"""
    c = A.BY_NAME[name]
    info = A.oracle(name, 0)[2]
    return [t for t in range(info["slices"]) if t * info["hop_in"] + c.fft <= A.frames_of(c.fft)]


# ---- the trace itself ----------------------------------------------------------------------------------------------
def test_the_plane_trace_is_off_by_default_and_changes_nothing():
    x = A.streams("ordinary_1024")[0]
    o = O.Oracle(1, fftsize=1024, **A.SHIFT)
    o.process(x[:, :4800])
    with pytest.raises(RuntimeError):
        o.plane_trace()
    assert o.L.pvo_enable_plane_trace(o.h) == -1   # not once steps have been recorded
    o.close()
    plain, counts, _ = O.run_offline(x, block=A.BLOCK, fftsize=1024, **A.SHIFT)
    want, wc, info = A.oracle("ordinary_1024", 0)
    assert np.array_equal(plain.view(np.uint32), want.view(np.uint32)) and tuple(counts) == wc
    p = info["planes"]
    k, m = info["trace"]
    assert np.array_equal(p["npk"], k) and np.array_equal(p["mode"], m) and len(k) == info["slices"]


def test_the_planes_are_what_the_oracle_computes_from_them():
    """mag and phase from re and im by the conversion's own operations; the peak list from mag by the reference's walk;
    the first step's output phases are its analysis phases; a locked step's are its phases turned by its rotations"""
    for name in ("ordinary_512", "holes_1024", "corners_4096"):
        p = A.oracle(name, 0)[2]["planes"]
        hs = A.BY_NAME[name].fft // 2
        assert np.array_equal(np.sqrt(p["re"] * p["re"] + p["im"] * p["im"]).view(np.uint32), p["mag"].view(np.uint32))
        near = np.abs(np.arctan2(p["im"].astype(np.float64), p["re"].astype(np.float64)) - p["phase"]) <= 4e-7
        assert near.all()
        for t in range(len(p["npk"])):
            mag, b, want = p["mag"][t], 2, []
            while b + 2 < hs:
                if mag[b] > mag[b - 1] and mag[b] > mag[b - 2] and mag[b] > mag[b + 1] and mag[b] > mag[b + 2]:
                    want.append(b)
                    b += 3
                else:
                    b += 1
            assert list(p["peaks"][t, :p["npk"][t]]) == want, (name, t)
            assert not p["peaks"][t, p["npk"][t]:].any()
            if p["mode"][t] != 2:
                assert not p["rot"][t].any()
        assert p["mode"][0] == 0 and np.array_equal(p["outphase"][0].view(np.uint32), p["phase"][0, :hs].view(np.uint32))
        t = int(np.flatnonzero(p["mode"] == 2)[0])
        pk, n = p["peaks"][t], p["npk"][t]
        for i in (0, n // 2, n - 1):
            b = pk[i]
            want = np.float32(O.lib().pvo_princarg(float(np.float32(p["phase"][t, b] + p["rot"][t, i]))))
            assert want.view(np.uint32) == p["outphase"][t, b].view(np.uint32), (name, t, i)


# ---- levels ----------------------------------------------------------------------------------------------------------
# Literals of stream 0 per fft size: the steps of a row and how many of them come before the flush; per level case
# (p_in, p_mixed, p_out, f_split, f_silent, kmin, kmax, top) of situation().
LEVEL_KEYS = ("p_in", "p_mixed", "p_out", "f_split", "f_silent", "kmin", "kmax", "top")
LEVEL_EXPECT = {
    256: dict(steps=499, flush=461,
              ordinary=(480, 0, 0, 0, 19, 14, 25, 3.3),
              mixed=(151, 329, 0, 0, 19, 14, 25, -32.7),
              out=(0, 0, 480, 0, 19, 14, 25, -49.7),
              subnormal=(0, 0, 480, 0, 19, 6, 20, -66.7),
              zero=(0, 0, 480, 0, 19, 0, 0, -96.7),
              loud=(370, 110, 0, 0, 19, 14, 25, 63.3),
              dc=(480, 0, 0, 0, 19, 14, 25, 5.1),
              holes=(464, 0, 0, 0, 35, 0, 26, 3.3)),
    512: dict(steps=250, flush=221,
              ordinary=(240, 0, 0, 0, 10, 34, 52, 4.0),
              mixed=(38, 202, 0, 0, 10, 34, 52, -32.0),
              out=(0, 0, 240, 0, 10, 34, 52, -50.0),
              subnormal=(0, 0, 240, 0, 10, 24, 46, -66.0),
              zero=(0, 0, 240, 0, 10, 0, 0, -96.0),
              loud=(166, 74, 0, 0, 10, 34, 52, 63.2),
              dc=(240, 0, 0, 0, 10, 33, 51, 6.0),
              holes=(224, 0, 0, 0, 26, 0, 52, 4.0)),
    1024: dict(steps=124, flush=100,
               ordinary=(238, 0, 0, 0, 5, 88, 105, 5.0),
               mixed=(60, 178, 0, 48, 5, 88, 105, -31.0),
               out=(0, 0, 238, 0, 5, 88, 105, -50.0),
               subnormal=(0, 0, 238, 0, 5, 70, 92, -65.0),
               zero=(0, 0, 238, 0, 5, 0, 0, -95.0),
               loud=(200, 38, 0, 38, 5, 88, 105, 63.2),
               dc=(238, 0, 0, 0, 5, 88, 105, 7.0),
               holes=(208, 0, 0, 0, 20, 0, 105, 5.0)),
    2048: dict(steps=62, flush=40,
               ordinary=(240, 0, 0, 0, 2, 166, 184, 6.0),
               mixed=(88, 149, 3, 49, 2, 166, 184, -30.0),
               out=(0, 0, 240, 0, 2, 166, 184, -50.0),
               subnormal=(0, 0, 240, 0, 2, 152, 173, -64.0),
               zero=(0, 0, 240, 0, 2, 0, 0, -94.0),
               loud=(225, 15, 0, 15, 2, 166, 184, 63.1),
               dc=(240, 0, 0, 0, 2, 166, 194, 8.0),
               holes=(180, 0, 0, 0, 17, 0, 190, 6.0)),
    4096: dict(steps=61, flush=42,
               ordinary=(480, 0, 0, 0, 1, 347, 377, 7.1),
               mixed=(228, 246, 6, 59, 1, 347, 377, -28.9),
               out=(0, 0, 480, 0, 1, 347, 377, -49.9),
               subnormal=(0, 0, 480, 0, 1, 335, 367, -62.9),
               zero=(0, 0, 480, 0, 1, 0, 0, -92.9),
               loud=(450, 30, 0, 30, 1, 347, 377, 63.2),
               dc=(480, 0, 0, 0, 1, 346, 386, 9.0),
               holes=(360, 0, 0, 0, 16, 0, 377, 7.1)),
    8192: dict(steps=50, flush=40,
               ordinary=(800, 0, 0, 0, 0, 717, 746, 8.0),
               mixed=(455, 341, 4, 49, 0, 717, 746, -28.0),
               out=(0, 0, 800, 0, 0, 717, 746, -50.0),
               subnormal=(0, 0, 800, 0, 0, 701, 735, -62.0),
               zero=(0, 0, 800, 0, 0, 0, 0, -92.0),
               loud=(790, 10, 0, 10, 0, 717, 746, 63.1),
               dc=(800, 0, 0, 0, 0, 717, 778, 10.0),
               holes=(560, 0, 0, 0, 15, 0, 750, 7.7)),
}


@pytest.mark.parametrize("fft", A.FFTS)
def test_the_level_cases_reach_their_situations(fft):
    sit = {lv: situation(f"{lv}_{fft}") for lv in A.LEVELS}
    for lv in A.LEVELS:
        print(fft, lv, sit[lv])
    want = LEVEL_EXPECT[fft]
    for lv in A.LEVELS:
        assert (sit[lv]["steps"], sit[lv]["flush"]) == (want["steps"], want["flush"]), lv
        assert tuple(sit[lv][k] for k in LEVEL_KEYS) == want[lv], lv
    # ... and what the literals must amount to, so that nobody edits them into something else
    passes = max(fft // 512, 1)
    o = sit["ordinary"]
    sounding = passes * (o["steps"] - o["f_silent"])
    # ordinary: every pass of every frame with sound in it is in range; there are flush frames
    assert o["p_in"] == sounding and o["p_mixed"] == 0 and o["p_out"] == 0
    assert 0 < o["flush"] < o["steps"] and o["sub"] == 0 and o["zsq"] == 0
    # mixed: passes with both kinds of bin; with two passes or more, frames with a pass in range beside one that is not
    m = sit["mixed"]
    assert m["p_mixed"] > 0 and m["p_in"] > 0
    if passes > 1:
        assert m["f_split"] > 0
    # out: no bin but the parked DC one in range, in any frame with sound
    u = sit["out"]
    assert u["p_out"] == sounding and u["p_in"] == 0 and u["p_mixed"] == 0 and u["top"] < -48 and u["mags"] > 0
    # subnormal squares: the peak lists differ from the ordinary case's
    b = sit["subnormal"]
    assert b["sub"] > 1000 and b["mags"] > 0
    assert peak_lists(f"subnormal_{fft}") != peak_lists(f"ordinary_{fft}")
    # zero squares: components, but no magnitude, no peak, per-bin steps
    z = sit["zero"]
    assert z["zsq"] > 1000 and z["mags"] == 0 and z["kmax"] == 0 and z["modes"] == f"I1 P{z['steps'] - 1}"
    # loud: the largest component in [2^63, 2^63.4], so something is out of range at the top, and everything is finite
    ld = sit["loud"]
    assert 63.0 <= ld["top"] <= 63.4 and ld["finite"] and 0 < ld["p_mixed"] and ld["p_in"] + ld["p_mixed"] == sounding
    if passes > 1:
        assert ld["f_split"] > 0
    # dc offset: the ordinary level
    d = sit["dc"]
    assert d["p_in"] == sounding and d["top"] > o["top"] + 1.5
    # holes: frames without sound, the ordinary level elsewhere, per-bin steps in mid-stream
    h = sit["holes"]
    assert h["f_silent"] >= o["f_silent"] + 15 and h["p_mixed"] == 0 and h["p_out"] == 0
    assert "P" in h["modes"].split(" ", 2)[2].rsplit(" ", 1)[0]
    x = A.streams(f"holes_{fft}")[0]
    hop = A.oracle(f"holes_{fft}", 0)[2]["hop_in"]
    partly = [t for t in range(h["flush"]) if 0 < np.count_nonzero(x[0, t * hop:t * hop + fft] == 0) - np.count_nonzero(
        A.streams(f"ordinary_{fft}")[0][0, t * hop:t * hop + fft] == 0) < fft]
    assert len(partly) >= 4, partly   # frames that the hole's edges cut


def test_both_streams_of_a_pair_differ_by_half_a_turn():
    """the second stream of a pair is the negated first: the same magnitudes and lists, other phases"""
    a, b = (A.oracle("ordinary_1024", j)[2]["planes"] for j in (0, 1))
    assert np.array_equal(a["mag"], b["mag"]) and np.array_equal(a["peaks"], b["peaks"])
    assert not np.array_equal(a["phase"], b["phase"])


# ---- the peak search's corners ---------------------------------------------------------------------------------------
# per fft size and case: (kmin, kmax, steps with an odd count, with an even count, with none, with one) of stream 0
CORNER_KEYS = ("kmin", "kmax", "odd", "even", "k0", "k1")
CORNER_EXPECT = {
    256: dict(corners=(21, 26, 263, 236, 19, 1), outer=(18, 26, 242, 257, 19, 3), dcnyq=(15, 20, 244, 255, 19, 9),
              single=(0, 17, 464, 35, 35, 30), comb=(42, 42, 2, 497, 19, 0)),
    512: dict(corners=(43, 51, 122, 128, 10, 0), outer=(38, 45, 119, 131, 10, 4), dcnyq=(40, 41, 124, 126, 10, 9),
              single=(0, 35, 224, 26, 26, 30), comb=(84, 84, 2, 248, 10, 0)),
    1024: dict(corners=(88, 102, 54, 70, 5, 0), outer=(84, 100, 66, 58, 5, 5), dcnyq=(73, 83, 118, 6, 5, 9),
               single=(0, 83, 104, 20, 20, 30), comb=(170, 170, 4, 120, 5, 0)),
    2048: dict(corners=(176, 199, 29, 33, 2, 1), outer=(179, 194, 35, 27, 2, 0), dcnyq=(161, 176, 34, 28, 2, 10),
               single=(0, 161, 45, 17, 17, 29), comb=(340, 340, 2, 60, 2, 0)),
    4096: dict(corners=(366, 392, 26, 35, 1, 0), outer=(352, 382, 36, 25, 1, 2), dcnyq=(325, 340, 34, 27, 1, 9),
               single=(0, 339, 45, 16, 16, 29), comb=(682, 682, 5, 56, 1, 0)),
    8192: dict(corners=(728, 765, 23, 27, 0, 0), outer=(740, 767, 23, 27, 0, 0), dcnyq=(667, 667, 49, 1, 0, 8),
               single=(0, 637, 33, 17, 15, 11), comb=(1364, 1364, 5, 45, 0, 0)),
}


@pytest.mark.parametrize("fft", A.FFTS)
def test_the_corner_cases_reach_their_situations(fft):
    hs = fft // 2
    sit = {cn: situation(f"{cn}_{fft}") for cn in A.CORNERS}
    for cn in A.CORNERS:
        print(fft, cn, sit[cn])
        assert tuple(sit[cn][k] for k in CORNER_KEYS) == CORNER_EXPECT[fft][cn], cn
    # corners: every listed bin is in the list of every full frame, in both streams
    want = set(A.corner_bins(fft))
    assert {2, hs - 3} <= want and (fft < 1024 or {252, 255, 258, 300, 303} <= want)
    assert fft != 4096 or {1020, 1023, 1026} <= want
    full = full_frames(f"corners_{fft}")
    assert len(full) >= 30
    for j in (0, 1):
        lists = peak_lists(f"corners_{fft}", j)
        assert all(want <= set(lists[t]) for t in full), [sorted(want - set(lists[t])) for t in full][:3]
    # outer: maxima at bins 1 and hs - 2, absent from the lists, and nothing admissible within their reach
    p = A.oracle(f"outer_{fft}", 0)[2]["planes"]
    lists = peak_lists(f"outer_{fft}")
    for t in full_frames(f"outer_{fft}"):
        mag = p["mag"][t]
        assert mag[1] > mag[0] and mag[1] > mag[2] and mag[1] > mag[3]
        assert mag[hs - 2] > max(mag[hs - 4], mag[hs - 3], mag[hs - 1], mag[hs])
        assert 5 <= min(lists[t]) and max(lists[t]) <= hs - 6, (t, lists[t][0], lists[t][-1])
    # dcnyq: maxima at DC and at half the sample rate
    p = A.oracle(f"dcnyq_{fft}", 0)[2]["planes"]
    lists = peak_lists(f"dcnyq_{fft}")
    for t in full_frames(f"dcnyq_{fft}"):
        mag = p["mag"][t]
        assert mag[0] > mag[1] > mag[2] and mag[hs] > mag[hs - 1] > mag[hs - 2]
        assert 4 <= min(lists[t]) and max(lists[t]) <= hs - 4, (t, lists[t][0], lists[t][-1])
    # single: steps with exactly one peak, the line's, and steps without any; locked steps among the former
    s = sit["single"]
    p = A.oracle(f"single_{fft}", 0)[2]["planes"]
    ones = np.flatnonzero(p["npk"] == 1)
    assert s["k1"] >= 10 and s["k0"] >= 15 and set(p["peaks"][ones, 0]) == {hs // 2}
    assert np.any(p["mode"][ones] == 2)
    # odd and even counts both occur in every case but the comb, whose list is full: list_capacity(fft) in every full frame
    assert all(sit[cn]["odd"] > 0 and sit[cn]["even"] > 0 for cn in A.CORNERS)
    c = sit["comb"]
    assert c["kmin"] == c["kmax"] == list_capacity(fft)


# ---- addressing --------------------------------------------------------------------------------------------------------
# case: (streams, hop, steps of a row, steps before the flush)
ADDRESS_EXPECT = {
    "stretch_1024": (2, 85, 119, 119), "stretch_4096": (2, 341, 48, 48), "hop300_1024": (2, 300, 41, 35),
    "rows3_1024": (3, 101, 124, 100), "rows9_1024": (9, 101, 124, 100), "rows3_4096": (3, 406, 61, 42),
}


@pytest.mark.parametrize("case", A.ADDRESS_CASES, ids=lambda c: c.name)
def test_the_addressing_cases_reach_their_situations(case):
    xs = A.streams(case.name)
    info = A.oracle(case.name, 0)[2]
    got = (len(xs), info["hop_in"], info["slices"], info["flush_step"])
    assert got == ADDRESS_EXPECT[case.name], got
    assert len(xs) in (2, 3, 9) and len({x.tobytes() for x in xs}) == len(xs)   # every row its own signal
    assert info["hop_in"] != {1024: 101, 4096: 406}[case.fft] or len(xs) > 2
    phases = {A.oracle(case.name, j)[2]["planes"]["phase"][:4].tobytes() for j in range(len(xs))}
    assert len(phases) == len(xs)   # ... and its own planes


def test_the_flush_frames_are_in_the_trace():
    """steps past the input's end read zeros: partly silent frames, then silent ones, at every size where the flush of
    the pitch shift reaches that far"""
    for fft in (256, 512, 1024, 2048, 4096):
        s = situation(f"ordinary_{fft}")
        assert s["flush"] < s["steps"] and s["f_silent"] >= 1 and s["modes"].endswith(f"P{s['f_silent']}")


def test_the_analysis_census_has_its_keys_and_no_others():
    """PV_CENSUS_ANALYSIS_KERNEL (kind 5): set x kernel x nc in 128 ... 4096; anything else is no key, and PV_CENSUS_ANALYZE
    (kind 2) keeps the keys it had.  Without a launch every count is 0."""
    from audiomod_amd import engine as E
    count = E.lib().pv_debug_chain_census_count
    assert E.ANALYSIS_KERNELS == ("generic", "wave", "split", "stream") and E.ANALYSIS_NC == (128, 256, 512, 1024, 2048, 4096)
    for s in range(len(E.CENSUS_SETS)):
        for k in range(len(E.ANALYSIS_KERNELS)):
            assert all(count(5, s, k, nc, 0, 0) >= 0 for nc in E.ANALYSIS_NC)
            assert [count(5, s, k, nc, 0, 0) for nc in (0, 64, 100, 8192, -1)] == [-1] * 5
        assert [count(2, s, nc, 0, 0, 0) >= 0 for nc in (128, 256, 2048, 4096)] == [False, True, True, False]
    assert count(5, 0, 4, 256, 0, 0) == -1 and count(5, 0, -1, 256, 0, 0) == -1 and count(5, 4, 0, 256, 0, 0) == -1
    assert count(6, 0, 0, 256, 0, 0) == -1
    if not os.environ.get("AUDIOMOD_PV_CHAIN_CENSUS"):   # (switched on for the whole process otherwise: left alone)
        E.chain_census(True)
        try:
            assert E.analysis_census_read() == {}
        finally:
            E.chain_census(False)


def test_the_plane_tap_refuses_null_objects():
    from audiomod_amd import engine as E
    L, i = E.lib(), E.PlaneInfo()
    import ctypes as C
    for name, lead in (("pv_debug_batch", ()), ("pv_debug", ()), ("pv_debug_pool", (0,)), ("pv_debug_mbatch", (0,))):
        assert getattr(L, name + "_plane_info")(None, *lead, C.byref(i)) != 0


# ---- the trace buffer itself, outside Python --------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_the_plane_trace_under_sanitizers(tmp_path):
    """tests/native/oracle_trace_sanitize.c with the oracle, as one stand-alone program under ASan + UBSan: its second
    half switches the plane trace on, lets the buffers grow and reads them back whole, in part and past the end"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "oracle_trace_sanitize")
    cmd = ["gcc", "-O1", "-g", "-std=gnu99", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function", f"-I{root}/oracle",
           os.path.join(root, "tests/native/oracle_trace_sanitize.c"), os.path.join(root, "oracle/pv_oracle.c"), "-o", exe,
           "-lm"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and ("asan" in b.stderr.lower() or "ubsan" in b.stderr.lower()):
        pytest.skip("sanitizer runtimes not installed")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and " 0 failures" in r.stdout and "plane trace:" in r.stdout, r.stdout + r.stderr
