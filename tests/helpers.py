import ast
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def e2e_cases():
    return sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLD, "e2e_*.npz")))


def load_e2e(name):
    z = np.load(os.path.join(GOLD, f"e2e_{name}.npz"))
    x = z["x_i16"].astype(np.float32) / np.float32(32768.0)
    meta = ast.literal_eval(str(z["meta"]))
    return x, z["y"], [int(v) for v in z["counts"]], meta


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def rel_rms(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)))


# --- error shape: per-sample and per-window bounds sized by the reference alone -------------------------------------
WINDOW = 256       # one resampler tile (kTileOut, audiomod_amd/csrc/pv_kernels.h)
WINDOW_STEP = 128
# max abs error of the synthesis' sine / cosine, from DESIGN.md section 1: v_sin_f32 / v_cos_f32 as used (PV_ARITH_FAST),
# 1.5 ulp at 1 for pv_sincos.h (PV_ARITH_EXACT).  Keys are the engine's ARITH_FAST / ARITH_EXACT.
TRIG_DELTA = {0: 4.8e-7, 1: 1.2e-7}
SHAPE_MARGIN = 8.0   # times the floor (the oracle against itself with nudged sines and cosines)
SHAPE_ULPS = 4.0     # plus this many ulps of the expected output's peak
FLOOR_SEED = 1


def parity_shape(got, want):
    """How `got` differs from `want`, over the samples that are finite in `want`: whole-output RMS, the largest
    absolute error, and the worst RMS over windows of WINDOW samples stepped by WINDOW_STEP within one channel (a
    shorter output is one window) -- each of the last two with the (channel, sample) where it occurs.  inf everywhere
    if the shapes differ or the non-finite positions do not coincide (as the suite's rms() has it)."""
    a = np.asarray(got, np.float64)
    b = np.asarray(want, np.float64)
    bad = dict(rms=float("inf"), max_abs=float("inf"), max_at=None, win_rms=float("inf"), win_at=None)
    if a.shape != b.shape:
        return bad
    a = a.reshape(-1, a.shape[-1]) if a.ndim != 2 else a
    b = b.reshape(a.shape)
    fin = np.isfinite(b)
    if not np.array_equal(np.isfinite(a), fin):
        return bad
    with np.errstate(invalid="ignore"):
        d = np.where(fin, a - b, 0.0)
    out = dict(rms=0.0, max_abs=0.0, max_at=None, win_rms=0.0, win_at=None)
    if not fin.any():
        return out
    out["rms"] = float(np.sqrt(np.sum(d * d) / fin.sum()))
    ad = np.abs(d)
    c, i = np.unravel_index(int(np.argmax(ad)), ad.shape)
    out["max_abs"], out["max_at"] = float(ad[c, i]), (int(c), int(i))
    n = d.shape[1]
    w = min(WINDOW, n)
    starts = np.arange(0, n - w + 1, WINDOW_STEP)
    if starts[-1] != n - w:
        starts = np.append(starts, n - w)  # the tail is covered too
    sq = np.concatenate([np.zeros((d.shape[0], 1)), np.cumsum(d * d, axis=1)], axis=1)
    cnt = np.concatenate([np.zeros((d.shape[0], 1)), np.cumsum(fin, axis=1)], axis=1)
    s = sq[:, starts + w] - sq[:, starts]
    k = cnt[:, starts + w] - cnt[:, starts]
    wr = np.sqrt(np.maximum(s, 0.0) / np.maximum(k, 1.0))
    c, j = np.unravel_index(int(np.argmax(wr)), wr.shape)
    out["win_rms"], out["win_at"] = float(wr[c, j]), (int(c), int(starts[j]))
    return out


def peak_ulp(want):
    """One ulp (float32) of the largest finite magnitude in `want`; the smallest normal's for an all-zero output."""
    w = np.asarray(want, np.float32)
    fin = np.isfinite(w)
    peak = np.float32(np.max(np.abs(w[fin]))) if fin.any() else np.float32(0)
    peak = max(peak, np.finfo(np.float32).tiny)
    return float(np.spacing(np.float32(peak)))


def shape_report(got, want, floor):
    """(ok, text, ratios): `got` against `want` under the error-shape bar -- for max abs and for the worst window,
    metric(got, want) <= SHAPE_MARGIN * metric(floor) + SHAPE_ULPS * ulp(peak(want)); `floor` is parity_shape(oracle
    with nudged sines / cosines, oracle).  ratios: metric / floor metric (inf over a zero floor, 0 for no error)."""
    s = parity_shape(got, want)
    u = peak_ulp(want)
    ok, parts, ratios = True, [], {}
    for key, at in (("max_abs", "max_at"), ("win_rms", "win_at")):
        bound = SHAPE_MARGIN * floor[key] + SHAPE_ULPS * u
        good = s[key] <= bound
        ok = ok and good
        ratios[key] = 0.0 if s[key] == 0 else (s[key] / floor[key] if floor[key] > 0 else float("inf"))
        parts.append(f"{key} {s[key]:.3e} at {s[at]} (floor {floor[key]:.3e}, bound {bound:.3e}, "
                     f"ratio {ratios[key]:.2f}){'' if good else ' EXCEEDED'}")
    return ok, f"rms {s['rms']:.3e}; " + "; ".join(parts), ratios


def oracle_floor(run, x, arith, want=None, seed=FLOOR_SEED, **kw):
    """The noise floor of one case: the oracle (run = oracle_py.run_offline / run_realtime) with every synthesis sine /
    cosine nudged by TRIG_DELTA[arith], against the oracle itself (`want`, if the caller has it already)."""
    nudged = run(x, trig_nudge=TRIG_DELTA[arith], nudge_seed=seed, **kw)[0]
    if want is None:
        want = run(x, **kw)[0]
    return parity_shape(nudged, want)


def assert_shape(label, got, want, floor, arith):
    """Asserts the error-shape bar and, where AUDIOMOD_PARITY_SHAPE_LOG names a file, appends the case's figures to
    it first (how profiles/r05/parity_shape.txt was written)."""
    ok, text, ratios = shape_report(got, want, floor)
    log = os.environ.get("AUDIOMOD_PARITY_SHAPE_LOG")
    if log:
        with open(log, "a") as fh:
            fh.write(f"{label} [{'exact' if arith else 'fast'}] max_abs/floor {ratios['max_abs']:.2f} "
                     f"win_rms/floor {ratios['win_rms']:.2f} | {text} | {'ok' if ok else 'EXCEEDED'}\n")
    assert ok, f"{label}: {text}"
