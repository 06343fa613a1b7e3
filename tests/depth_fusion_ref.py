"""Restatement of depth fusion (include/dvo_amd.h, "Depth fusion": dvo_amd_pyramid_fuse_depth / _many) in numpy.

fuse_ref     one keyframe with its frames, vectorised over the keyframe's pixels: the rigid inverse in float64 in the pinned
             order, every other operation in np.float32 in the pinned order, the frames walked in order
fuse_brute   the same rule as an independent loop over the pixels in Python floats, every operation rounded to float32 on its own

A "planes" argument is (Z, K): the level-0 depth plane (float32 [h, w], NaN = no depth) and its intrinsics (fx, fy, ox, oy).
T[k] is 4x4 (row-major numpy, as everywhere in the Python binding) and maps points of frame k's camera into the keyframe's camera:
for match(keyframe, frame k) the result's Transformation as returned.  Both return
    (fused float32 [h, w], observations uint8 [h, w], frame_counts [n] of dicts, keyframe_counts dict)."""
import math

import numpy as np

from covisibility_ref import rays

F = np.float32
BILINEAR, NEAREST = 0, 1
MAX_FRAMES = 255
FRAME_COUNTS = ("valid", "behind", "outside", "no_depth", "consistent", "occluded", "seen_through", "fused")
KEYFRAME_COUNTS = ("with_depth", "confirmed", "unconfirmed_kept", "unconfirmed_dropped")
DEFAULTS = dict(near_z=0.1, depth_sigmas=5.0, min_cos=0.5, sample=BILINEAR, min_observations=0, drop_unconfirmed=0)


def inverse_rows(T):
    """rows 0..2 of the rigid inverse (R^T, -R^T t) of T, float64 products summed in index order, cast to float32 [3, 4]"""
    T = np.asarray(T, np.float64)
    M = np.empty((3, 4), F)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                M[r, c] = F(T[c, r])
            M[r, 3] = F(-((T[0, r] * T[0, 3] + T[1, r] * T[1, 3]) + T[2, r] * T[2, 3]))
    return M


def sigma(z):
    s = z - F(0.4)
    return F(0.0012) + F(0.0019) * (s * s)


def fuse_ref(key, frames, Ts, options=None, info=None):
    """info: None, or a list that receives one dict per frame: 'cls' (int [h, w]: -1 no depth, else the index into FRAME_COUNTS of
    the pixel's outcome), 'fused' (bool), 'qz', 'px', 'py' (the projection before the floor), 'd', 'tol', 'c' and 'M'"""
    o = dict(DEFAULTS, **(options or {}))
    assert len(frames) == len(Ts) <= MAX_FRAMES and o["sample"] in (BILINEAR, NEAREST)
    near, sig, min_cos = F(o["near_z"]), F(o["depth_sigmas"]), F(o["min_cos"])
    Z0, K0 = key
    Z0 = np.asarray(Z0, F)
    h, w = Z0.shape
    tx, ty = rays(w, h, K0)
    tx, ty = np.broadcast_to(tx[None, :], (h, w)), np.broadcast_to(ty[:, None], (h, w))
    frame_counts = []
    with np.errstate(all="ignore"):
        has = np.isfinite(Z0)
        wgt = F(1) / (sigma(Z0) * sigma(Z0))
        sw, swz = wgt.copy(), wgt * Z0
        n_obs = np.zeros((h, w), np.int64)
        x, y = tx * Z0, ty * Z0
        for (Zk, Kk), T in zip(frames, Ts):
            Zk = np.asarray(Zk, F)
            hk, wk = Zk.shape
            fx, fy, ox, oy = [F(k) for k in Kk]
            M = inverse_rows(T)
            qx, qy, qz = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * Z0) + M[r, 3] for r in range(3)]
            behind = has & ~(qz >= near)
            live = has & ~behind
            px, py = (qx * fx) / qz + ox, (qy * fy) / qz + oy
            if o["sample"] == NEAREST:
                pu, pv = np.floor(px + F(0.5)), np.floor(py + F(0.5))
                inside = (pu >= F(0)) & (pu <= F(wk - 1)) & (pv >= F(0)) & (pv <= F(hk - 1))
                outside = live & ~inside
                live = live & inside
                iu, iv = np.where(live, pu, F(0)).astype(np.int64), np.where(live, pv, F(0)).astype(np.int64)
                Zs = Zk[iv, iu]
                nan = np.isnan(Zs)
            else:
                x0, y0 = np.floor(px), np.floor(py)
                inside = (x0 >= F(0)) & (x0 <= F(wk - 2)) & (y0 >= F(0)) & (y0 <= F(hk - 2))
                outside = live & ~inside
                live = live & inside
                a, b = px - x0, py - y0
                iu, iv = np.where(live, x0, F(0)).astype(np.int64), np.where(live, y0, F(0)).astype(np.int64)
                z00, z10, z01, z11 = Zk[iv, iu], Zk[iv, iu + 1], Zk[iv + 1, iu], Zk[iv + 1, iu + 1]
                nan = np.isnan(z00) | np.isnan(z10) | np.isnan(z01) | np.isnan(z11)
                top = z00 + a * (z10 - z00)
                bot = z01 + a * (z11 - z01)
                Zs = top + b * (bot - top)
            no_depth = live & nan
            live = live & ~nan
            d = Zs - qz
            tol = sig * sigma(qz)
            occluded = live & (d < -tol)
            seen = live & (d > tol)
            consistent = live & ~occluded & ~seen
            c = (M[2, 0] * tx + M[2, 1] * ty) + M[2, 2]
            fused = consistent & (c >= min_cos)
            z_obs = Z0 + d / c
            wk_ = F(1) / (sigma(Zs) * sigma(Zs))
            sw = np.where(fused, sw + wk_, sw)
            swz = np.where(fused, swz + wk_ * z_obs, swz)
            n_obs += fused
            assert all(v.dtype == F for v in (x, qz, px, d, tol, c, z_obs, wk_, sw, swz))
            masks = (has, behind, outside, no_depth, consistent, occluded, seen, fused)
            frame_counts.append({name: int(m.sum()) for name, m in zip(FRAME_COUNTS, masks)})
            if info is not None:
                cls = np.full((h, w), -1, np.int64)
                for k in range(1, 7):
                    cls[masks[k]] = k
                info.append(dict(cls=cls, fused=fused.copy(), qz=qz, px=px, py=py, d=d, tol=tol, c=c, M=M))
        fusedz = swz / sw
        confirmed = has & (n_obs >= int(o["min_observations"]))
        dropped = has & ~confirmed & bool(o["drop_unconfirmed"])
        kept = has & ~confirmed & ~dropped
        out = np.where(has & ~dropped, fusedz, F(np.nan)).astype(F)
    observations = np.where(has, n_obs, 0).astype(np.uint8)
    key_counts = dict(with_depth=int(has.sum()), confirmed=int(confirmed.sum()), unconfirmed_kept=int(kept.sum()),
                      unconfirmed_dropped=int(dropped.sum()))
    return out, observations, frame_counts, key_counts


def _f(v):
    """a Python float rounded to float32 (double rounding is harmless for one +, -, * or / of float32 operands)"""
    with np.errstate(all="ignore"):
        return float(F(v))


def _sigma(z):
    s = _f(z - _f(0.4))
    return _f(_f(0.0012) + _f(_f(0.0019) * _f(s * s)))


def _div(a, b):
    """a / b as IEEE does it, for Python floats"""
    with np.errstate(all="ignore"):
        return float(F(a) / F(b))


def fuse_brute(key, frames, Ts, options=None):
    o = dict(DEFAULTS, **(options or {}))
    near, sig, min_cos = _f(o["near_z"]), _f(o["depth_sigmas"]), _f(o["min_cos"])
    Z0, K0 = key
    h, w = np.shape(Z0)
    fx0, fy0, ox0, oy0 = [_f(k) for k in K0]
    Ms = [[[float(v) for v in row] for row in inverse_rows(T)] for T in Ts]
    out = np.full((h, w), np.nan, F)
    observations = np.zeros((h, w), np.uint8)
    frame_counts = [dict.fromkeys(FRAME_COUNTS, 0) for _ in frames]
    key_counts = dict.fromkeys(KEYFRAME_COUNTS, 0)
    for v in range(h):
        for u in range(w):
            z0 = float(Z0[v][u])
            if not math.isfinite(z0):
                continue
            key_counts["with_depth"] += 1
            tx, ty = _div(_f(u - ox0), fx0), _div(_f(v - oy0), fy0)
            wgt = _div(1.0, _f(_sigma(z0) * _sigma(z0)))
            sw, swz, n_obs = wgt, _f(wgt * z0), 0
            x, y = _f(tx * z0), _f(ty * z0)
            for k, ((Zk, Kk), M) in enumerate(zip(frames, Ms)):
                cnt = frame_counts[k]
                cnt["valid"] += 1
                hk, wk = np.shape(Zk)
                fx, fy, ox, oy = [_f(kk) for kk in Kk]
                q = [_f(_f(_f(_f(M[r][0] * x) + _f(M[r][1] * y)) + _f(M[r][2] * z0)) + M[r][3]) for r in range(3)]
                if not q[2] >= near:
                    cnt["behind"] += 1
                    continue
                px, py = _f(_div(_f(q[0] * fx), q[2]) + ox), _f(_div(_f(q[1] * fy), q[2]) + oy)
                if o["sample"] == NEAREST:
                    pu, pv = math.floor(_f(px + 0.5)) if math.isfinite(px) else px, math.floor(_f(py + 0.5)) if math.isfinite(py) else py
                    if not (0 <= pu <= wk - 1 and 0 <= pv <= hk - 1):
                        cnt["outside"] += 1
                        continue
                    Zs = float(Zk[int(pv)][int(pu)])
                    if math.isnan(Zs):
                        cnt["no_depth"] += 1
                        continue
                else:
                    x0, y0 = math.floor(px) if math.isfinite(px) else px, math.floor(py) if math.isfinite(py) else py
                    if not (0 <= x0 <= wk - 2 and 0 <= y0 <= hk - 2):
                        cnt["outside"] += 1
                        continue
                    a, b = _f(px - x0), _f(py - y0)
                    z00, z10, z01, z11 = [float(Zk[int(y0) + j][int(x0) + i]) for j in (0, 1) for i in (0, 1)]
                    if any(math.isnan(z) for z in (z00, z10, z01, z11)):
                        cnt["no_depth"] += 1
                        continue
                    top = _f(z00 + _f(a * _f(z10 - z00)))
                    bot = _f(z01 + _f(a * _f(z11 - z01)))
                    Zs = _f(top + _f(b * _f(bot - top)))
                d = _f(Zs - q[2])
                tol = _f(sig * _sigma(q[2]))
                if d < -tol:
                    cnt["occluded"] += 1
                    continue
                if d > tol:
                    cnt["seen_through"] += 1
                    continue
                cnt["consistent"] += 1
                c = _f(_f(_f(M[2][0] * tx) + _f(M[2][1] * ty)) + M[2][2])
                if not c >= min_cos:
                    continue
                cnt["fused"] += 1
                z_obs = _f(z0 + _div(d, c))
                wk_ = _div(1.0, _f(_sigma(Zs) * _sigma(Zs)))
                sw, swz, n_obs = _f(sw + wk_), _f(swz + _f(wk_ * z_obs)), n_obs + 1
            observations[v][u] = n_obs
            fusedz = _div(swz, sw)
            if n_obs >= int(o["min_observations"]):
                key_counts["confirmed"] += 1
                out[v][u] = fusedz
            elif o["drop_unconfirmed"]:
                key_counts["unconfirmed_dropped"] += 1
            else:
                key_counts["unconfirmed_kept"] += 1
                out[v][u] = fusedz
    return out, observations, frame_counts, key_counts
