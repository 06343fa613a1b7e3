"""Restatement of the exposure compensation (include/dvo_amd.h, "Exposure compensation") in numpy and Python integers.

estimate_ref    the whole record of one pair at one level, vectorised, on top of covisibility_ref.covis_ref(info=True): outcomes and
                landing pixels are that function's, every fp32 operation of steps 3..5 is np.float32's, the sums are int64 sums of
                int64 values (exact: they stay below 2^63) and the solve runs on Python integers, whose float() is correctly rounded
estimate_brute  the same record from an independent loop over the pixels in Python floats, every operation rounded to float32 on its
                own, the sums Python integers from the start
solve_ref       rules 7 and 8 from six integers
adjust_ref      level 0's adjusted intensity plane
exposure_pair   the 160x120 sensor-regime pair of the tests with the current frame's texture mapped I -> g I + b before noise,
                rounding and clipping

A "planes" argument is (I, Z, K): intensity and depth plane of the level (float32 [h, w], NaN = no depth) and its intrinsics.  T is a
4x4 row-major matrix, reference -> current (the estimate); None is the identity.  Options: a dict of dvo_amd_exposure_options'
fields."""
import math

import numpy as np

from covisibility_ref import covis_ref

F = np.float32
DEFAULTS = dict(level=0, near_z=0.1, depth_sigmas=20.0, min_intensity=4.0, max_intensity=251.0, scale=16.0, trim=12.0, refits=4,
                min_pairs=64, min_gain=0.25, max_gain=4.0)
MAX_PASSES = 9
COVIS = ("valid", "behind", "outside", "no_depth", "consistent", "occluded", "seen_through")
COUNTS = COVIS + ("masked", "saturated", "candidates", "used", "trimmed")
SUMS = ("n", "sx", "sy", "sxx", "sxy", "syy")
CONSISTENT = 4


def solve_ref(n, sx, sy, sxx, sxy, syy, options=None):
    """(gain, bias, r2, degenerate) of one pass from its six sums (Python integers of any size)"""
    o = dict(DEFAULTS, **(options or {}))
    n, sx, sy, sxx, sxy, syy = (int(v) for v in (n, sx, sy, sxx, sxy, syy))
    if n < int(o["min_pairs"]):
        return 1.0, 0.0, 0.0, 1
    det = n * sxx - sx * sx
    if det <= 0:
        return 1.0, 0.0, 0.0, 2
    ng, nb, dety = n * sxy - sx * sy, sy * sxx - sx * sxy, n * syy - sy * sy
    gain = float(ng) / float(det)
    if not math.isfinite(gain) or not float(o["min_gain"]) <= gain <= float(o["max_gain"]):
        return 1.0, 0.0, 0.0, 3
    bias = (float(nb) / float(det)) / float(F(o["scale"]))
    r2 = 0.0 if dety <= 0 else (float(ng) / float(det)) * (float(ng) / float(dety))
    return gain, bias, r2, 0


def _finish(counts, pass_sums, o):
    """the record from the pass-independent counts and the six sums of every pass that ran"""
    out = dict(counts)
    out.update(gain_pass=[0.0] * MAX_PASSES, bias_pass=[0.0] * MAX_PASSES, used_pass=[0] * MAX_PASSES)
    for p, sums in enumerate(pass_sums):
        gain, bias, r2, code = solve_ref(*sums, options=o)
        out.update(gain=gain, bias=bias, r2=r2, degenerate=code, passes=p + 1, used=sums[0], trimmed=counts["candidates"] - sums[0])
        out.update(zip(SUMS, sums))
        out["gain_pass"][p], out["bias_pass"][p], out["used_pass"][p] = gain, bias, sums[0]
    return out


def estimate_ref(planes_ref, planes_cur, T=None, mask=None, options=None, info=False):
    """the record of dvo_amd_estimate_exposure as a dict of Python values (capi.ExposureEstimate.as_dict()'s keys); with info=True
    also 'x', 'y' (float32 planes on the reference's pixels), 'candidate' and 'used' (bool planes, the last pass's)"""
    o = dict(DEFAULTS, **(options or {}))
    (Ir, Zr, Kr), (Ic, Zc, Kc) = planes_ref, planes_cur
    Ir, Ic = np.asarray(Ir, F), np.asarray(Ic, F)
    T = np.eye(4) if T is None else np.asarray(T, np.float64)
    cov = covis_ref((Zr, Kr), (Zc, Kc), T, np.eye(4), dict(near_z=o["near_z"], depth_sigmas=o["depth_sigmas"]), info=True)
    assert np.array_equal(cov["T"], T[:3].astype(F), equal_nan=True)  # the float cast of T, no more
    consistent = cov["cls"] == CONSISTENT
    iu = np.where(consistent, cov["pu"], 0).astype(np.int64)
    iv = np.where(consistent, cov["pv"], 0).astype(np.int64)
    kept = np.ones(consistent.shape, bool) if mask is None else np.asarray(mask) != 0
    assert kept.shape == consistent.shape == Ir.shape
    masked = consistent & ~kept
    live = consistent & kept
    lo, hi, scale, trim = F(o["min_intensity"]), F(o["max_intensity"]), F(o["scale"]), F(o["trim"])
    with np.errstate(all="ignore"):
        x, y = Ic[iv, iu], Ir
        in_range = (x >= lo) & (x <= hi) & (y >= lo) & (y <= hi)
        candidate = live & in_range
        X, Y = np.rint(x * scale), np.rint(y * scale)
        assert X.dtype == F and Y.dtype == F
        X = np.where(candidate, X, F(0)).astype(np.int64)
        Y = np.where(candidate, Y, F(0)).astype(np.int64)
    counts = {k: cov[k] for k in COVIS}
    counts.update(masked=int(masked.sum()), saturated=int((live & ~in_range).sum()), candidates=int(candidate.sum()))
    pass_sums, gain, bias, used = [], 1.0, 0.0, candidate
    for p in range(int(o["refits"]) + 1):
        if p > 0:
            with np.errstate(all="ignore"):
                r = np.abs((F(gain) * x + F(bias)) - y)
            assert r.dtype == F
            used = candidate & (r <= trim)
        Xu, Yu = X[used], Y[used]
        sums = (int(used.sum()), int(Xu.sum()), int(Yu.sum()), int((Xu * Xu).sum()), int((Xu * Yu).sum()), int((Yu * Yu).sum()))
        pass_sums.append(sums)
        gain, bias, _, code = solve_ref(*sums, options=o)
        if code:
            break
    out = _finish(counts, pass_sums, o)
    if info:
        out.update(x=x, y=y, candidate=candidate, used_plane=used)
    return out


def _f(v):
    """a Python float rounded to float32 (double rounding is harmless for one +, -, * or / of float32 operands)"""
    with np.errstate(all="ignore"):
        return float(F(v))


def _op(op, a, b):
    """one IEEE operation on two float32 values, rounded to float32"""
    with np.errstate(all="ignore"):
        a, b = F(a), F(b)
        return float(a * b if op == "*" else a + b if op == "+" else a - b if op == "-" else a / b)


def estimate_brute(planes_ref, planes_cur, T=None, mask=None, options=None):
    """the same record from a loop over the reference's pixels; nothing of covisibility_ref is used"""
    o = dict(DEFAULTS, **(options or {}))
    (Ir, Zr, Kr), (Ic, Zc, Kc) = planes_ref, planes_cur
    hr, wr = np.shape(Zr)
    hc, wc = np.shape(Zc)
    fxr, fyr, oxr, oyr = [_f(k) for k in Kr]
    fx, fy, ox, oy = [_f(k) for k in Kc]
    M = np.eye(4) if T is None else np.asarray(T, np.float64)
    Tf = [[_f(M[r][c]) for c in range(4)] for r in range(3)]
    near, sig = _f(o["near_z"]), _f(o["depth_sigmas"])
    lo, hi, scale, trim = _f(o["min_intensity"]), _f(o["max_intensity"]), _f(o["scale"]), _f(o["trim"])
    n = dict.fromkeys(COVIS + ("masked", "saturated", "candidates"), 0)
    cand = []  # (x, y, X, Y) per candidate
    for v in range(hr):
        tyv = _op("/", _op("-", float(v), oyr), fyr)
        for u in range(wr):
            z = float(Zr[v][u])
            if not math.isfinite(z):
                continue
            n["valid"] += 1
            px, py = _op("*", _op("/", _op("-", float(u), oxr), fxr), z), _op("*", tyv, z)
            q = [_op("+", _op("+", _op("+", _op("*", Tf[r][0], px), _op("*", Tf[r][1], py)), _op("*", Tf[r][2], z)), Tf[r][3]) for r in range(3)]
            if not q[2] >= near:
                n["behind"] += 1
                continue
            pu = _op("+", _op("+", _op("/", _op("*", q[0], fx), q[2]), ox), 0.5)
            pv = _op("+", _op("+", _op("/", _op("*", q[1], fy), q[2]), oy), 0.5)
            pu = math.floor(pu) if math.isfinite(pu) else pu
            pv = math.floor(pv) if math.isfinite(pv) else pv
            if not (0 <= pu <= wc - 1 and 0 <= pv <= hc - 1):
                n["outside"] += 1
                continue
            zc = float(Zc[int(pv)][int(pu)])
            if zc != zc:
                n["no_depth"] += 1
                continue
            s = _op("-", q[2], 0.4)
            tol = _op("*", sig, _op("+", _f(0.0012), _op("*", _f(0.0019), _op("*", s, s))))
            d = _op("-", zc, q[2])
            if d < -tol:
                n["occluded"] += 1
                continue
            if d > tol:
                n["seen_through"] += 1
                continue
            n["consistent"] += 1
            if mask is not None and not mask[v][u]:
                n["masked"] += 1
                continue
            x, y = float(Ic[int(pv)][int(pu)]), float(Ir[v][u])
            if not (lo <= x <= hi and lo <= y <= hi):
                n["saturated"] += 1
                continue
            n["candidates"] += 1
            cand.append((x, y, round(_op("*", x, scale)), round(_op("*", y, scale))))  # (round: to nearest, ties to even, as rintf)
    pass_sums, gain, bias = [], 1.0, 0.0
    for p in range(int(o["refits"]) + 1):
        sums = [0] * 6
        g, b = _f(gain), _f(bias)
        for x, y, X, Y in cand:
            if p > 0 and not abs(_op("-", _op("+", _op("*", g, x), b), y)) <= trim:
                continue
            for i, t in enumerate((1, X, Y, X * X, X * Y, Y * Y)):
                sums[i] += t
        pass_sums.append(tuple(sums))
        gain, bias, _, code = solve_ref(*sums, options=o)
        if code:
            break
    return _finish(n, pass_sums, o)


def adjust_ref(I, gain, bias):
    """((float) gain * I) + (float) bias in float32, product and sum rounded separately"""
    with np.errstate(all="ignore"):
        out = (F(gain) * np.asarray(I, F)) + F(bias)
    assert out.dtype == F
    return out


def exposure_pair(synth, g=1.0, b=0.0, w=160, h=120, scale=0.5, edit=None):
    """((I_ref, Z_ref), (I_cur, Z_cur), T_gt, K): the sensor-regime pair with a motion of scale * XI_GT_PAIR whose current frame was
    exposed as I -> g I + b before noise, rounding and clipping.  edit(I): a change of the current's float texture after that."""
    T_gt = synth.se3_exp(scale * synth.XI_GT_PAIR)
    ref = synth.raw_to_float(*synth.sensor_frame(w, h, None, synth.SEED, 0))
    I, Z = synth.render(w, h, T_gt, synth.SEED, 1)
    I = (g * I.astype(np.float64) + b).astype(F)
    grey, raw_z = synth.sensor_from_analytic(I, Z, synth.SEED, 1)
    Ic, Zc = synth.raw_to_float(grey, raw_z)
    if edit is not None:
        Ic = edit(Ic)
    return ref, (Ic, Zc), T_gt, synth.intrinsics_for(w, h)
