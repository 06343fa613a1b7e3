"""Restatement of the loop-closure candidate search (include/dvo_amd.h: dvo_amd_covisibility,
dvo_amd_find_constraint_candidates) in numpy.

covis_ref    the seven counts of one ordered pair (a, b), vectorised: the transform in float64 in the pinned order, every other
             operation in np.float32 in the pinned order
covis_brute  the same rule as an independent pixel loop over Python floats, every operation rounded to float32 on its own
radius_ref   the radius stage
candidates_ref  the whole search from a table of overlaps

A "planes" argument is (Z, K): the depth plane of the level (float32 [h, w], NaN = no depth) and its intrinsics (fx, fy, ox, oy).
Poses are 4x4 camera -> world (row-major numpy, as everywhere in the Python binding).  Options: dict(near_z, depth_sigmas)."""
import numpy as np

F = np.float32
COUNTS = ("valid", "behind", "outside", "no_depth", "consistent", "occluded", "seen_through")
DEFAULTS = dict(level=3, near_z=0.1, depth_sigmas=20.0)


def relative_transform(T_a, T_b):
    """rows 0..2 of T_b^-1 * T_a, the inverse taken as rigid, float64 products summed in index order, cast to float32 [3, 4]"""
    A, B = np.asarray(T_a, np.float64), np.asarray(T_b, np.float64)
    T = np.empty((3, 4), F)
    with np.errstate(all="ignore"):
        for r in range(3):
            i0, i1, i2 = B[0, r], B[1, r], B[2, r]  # row r of Rb^T
            ti = -((i0 * B[0, 3] + i1 * B[1, 3]) + i2 * B[2, 3])
            for c in range(3):
                T[r, c] = F((i0 * A[0, c] + i1 * A[1, c]) + i2 * A[2, c])
            T[r, 3] = F(((i0 * A[0, 3] + i1 * A[1, 3]) + i2 * A[2, 3]) + ti)
    return T


def rays(w, h, K):
    fx, fy, ox, oy = [F(k) for k in K]
    return (np.arange(w, dtype=F) - ox) / fx, (np.arange(h, dtype=F) - oy) / fy


def covis_ref(planes_a, planes_b, T_a, T_b, options=None, info=False):
    """dict of the seven counts (Python ints); with info=True also 'cls' (int [h, w]: -1 no depth, else the index into COUNTS of
    the pixel's outcome), 'T', 'qz', 'proj_u', 'proj_v' (before the + 0.5 and the floor), 'pu', 'pv', 'd', 'tol'"""
    o = dict(DEFAULTS, **(options or {}))
    near, sig = F(o["near_z"]), F(o["depth_sigmas"])
    (Za, Ka), (Zb, Kb) = planes_a, planes_b
    Za, Zb = np.asarray(Za, F), np.asarray(Zb, F)
    ha, wa = Za.shape
    hb, wb = Zb.shape
    fx, fy, ox, oy = [F(k) for k in Kb]
    T = relative_transform(T_a, T_b)
    tx, ty = rays(wa, ha, Ka)
    with np.errstate(all="ignore"):
        z = Za
        x, y = tx[None, :] * z, ty[:, None] * z
        qx, qy, qz = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)]
        valid = np.isfinite(z)
        behind = valid & ~(qz >= near)
        live = valid & ~behind
        proj_u, proj_v = (qx * fx) / qz + ox, (qy * fy) / qz + oy
        pu, pv = np.floor(proj_u + F(0.5)), np.floor(proj_v + F(0.5))
        inside = (pu >= F(0)) & (pu <= F(wb - 1)) & (pv >= F(0)) & (pv <= F(hb - 1))
        outside = live & ~inside
        live = live & inside
        iu, iv = np.where(live, pu, F(0)).astype(np.int64), np.where(live, pv, F(0)).astype(np.int64)
        zb = Zb[iv, iu]
        no_depth = live & np.isnan(zb)
        live = live & ~np.isnan(zb)
        s = qz - F(0.4)
        tol = sig * (F(0.0012) + F(0.0019) * (s * s))
        d = zb - qz
        occluded = live & (d < -tol)
        seen = live & (d > tol)
        consistent = live & ~occluded & ~seen
    assert all(a.dtype == F for a in (x, y, qx, qy, qz, proj_u, pu, tol, d))
    masks = (valid, behind, outside, no_depth, consistent, occluded, seen)
    out = {name: int(m.sum()) for name, m in zip(COUNTS, masks)}
    if info:
        cls = np.full(Za.shape, -1, np.int64)
        for k in range(1, 7):
            cls[masks[k]] = k
        out.update(cls=cls, T=T, qz=qz, proj_u=proj_u, proj_v=proj_v, pu=pu, pv=pv, d=d, tol=tol)
    return out


def _f(v):
    """a Python float rounded to float32 (double rounding is harmless for one +, -, * or / of float32 operands)"""
    with np.errstate(all="ignore"):
        return float(F(v))


def covis_brute(planes_a, planes_b, T_a, T_b, options=None):
    """the same counts from a loop over the pixels of a in Python floats"""
    import math

    o = dict(DEFAULTS, **(options or {}))
    near, sig = _f(o["near_z"]), _f(o["depth_sigmas"])
    (Za, Ka), (Zb, Kb) = planes_a, planes_b
    ha, wa = np.shape(Za)
    hb, wb = np.shape(Zb)
    fxa, fya, oxa, oya = [_f(k) for k in Ka]
    fx, fy, ox, oy = [_f(k) for k in Kb]
    A = [[float(v) for v in row] for row in np.asarray(T_a, np.float64)]
    B = [[float(v) for v in row] for row in np.asarray(T_b, np.float64)]

    def mul(a, b):  # float64 product; inf * 0 and the like are NaN, as in IEEE arithmetic
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b))

    def add(a, b):
        with np.errstate(all="ignore"):
            return float(np.float64(a) + np.float64(b))

    T = [[0.0] * 4 for _ in range(3)]
    for r in range(3):
        inv = [B[0][r], B[1][r], B[2][r]]
        ti = -add(add(mul(inv[0], B[0][3]), mul(inv[1], B[1][3])), mul(inv[2], B[2][3]))
        for c in range(4):
            acc = add(add(mul(inv[0], A[0][c]), mul(inv[1], A[1][c])), mul(inv[2], A[2][c]))
            T[r][c] = _f(add(acc, ti) if c == 3 else acc)

    def f32(op, a, b):
        with np.errstate(all="ignore"):
            a, b = F(a), F(b)
            return float(a * b if op == "*" else a + b if op == "+" else a - b if op == "-" else a / b)

    n = dict.fromkeys(COUNTS, 0)
    for v in range(ha):
        tyv = f32("/", f32("-", float(v), oya), fya)
        for u in range(wa):
            z = float(Za[v][u])
            if not math.isfinite(z):
                continue
            n["valid"] += 1
            x, y = f32("*", f32("/", f32("-", float(u), oxa), fxa), z), f32("*", tyv, z)
            q = [f32("+", f32("+", f32("+", f32("*", T[r][0], x), f32("*", T[r][1], y)), f32("*", T[r][2], z)), T[r][3]) for r in range(3)]
            if not q[2] >= near:
                n["behind"] += 1
                continue
            pu = f32("+", f32("+", f32("/", f32("*", q[0], fx), q[2]), ox), 0.5)
            pv = f32("+", f32("+", f32("/", f32("*", q[1], fy), q[2]), oy), 0.5)
            pu = math.floor(pu) if math.isfinite(pu) else pu
            pv = math.floor(pv) if math.isfinite(pv) else pv
            if not (0 <= pu <= wb - 1 and 0 <= pv <= hb - 1):
                n["outside"] += 1
                continue
            zb = float(Zb[int(pv)][int(pu)])
            if zb != zb:
                n["no_depth"] += 1
                continue
            s = f32("-", q[2], 0.4)
            tol = f32("*", sig, f32("+", _f(0.0012), f32("*", _f(0.0019), f32("*", s, s))))
            d = f32("-", zb, q[2])
            n["occluded" if d < -tol else "seen_through" if d > tol else "consistent"] += 1
    return n


def overlap(counts):
    """consistent / valid in double, 0 when valid == 0"""
    return float(np.float64(counts["consistent"]) / np.float64(counts["valid"])) if counts["valid"] else 0.0


def radius_ref(poses, keyframe, max_distance):
    """indices k, ascending, with ((dx dx + dy dy) + dz dz) <= max_distance * max_distance in float32 over float32 translations"""
    t = np.stack([np.asarray(p, np.float64)[:3, 3] for p in poses]).astype(F)
    d = t - t[keyframe]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r = F(max_distance)
    assert d2.dtype == F
    return [int(k) for k in np.nonzero(d2 <= r * r)[0]]


def candidates_ref(poses, keyframe, max_distance, min_overlap, overlap_of):
    """(candidates, overlaps): the radius candidates c with max(overlap_of(keyframe, c), overlap_of(c, keyframe)) >= min_overlap"""
    found = radius_ref(poses, keyframe, max_distance)
    if not min_overlap > 0:
        return found, [float("nan")] * len(found)
    best = [max(overlap_of(keyframe, c), overlap_of(c, keyframe)) for c in found]
    keep = [i for i, o in enumerate(best) if o >= min_overlap]
    return [found[i] for i in keep], [best[i] for i in keep]
