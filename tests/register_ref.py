"""The registration rule of include/dvo_amd.h (dvo_amd_pyramid_create_raw_registered) restated twice:
register_ref    numpy, every operation on arrays of one dtype (float32: the rule; float64: the same formula in double, for the
                fidelity test) in the pinned order
register_brute  a loop over the depth pixels on Python floats rounded to float32 after every operation, with its own footprint
                walk and a dictionary as the depth buffer
Both return (plane, counters) with counters = {measurements, behind, outside, drawn, covered_pixels}."""
import math
import struct

import numpy as np

F = np.float32
COUNTERS = ("measurements", "behind", "outside", "drawn", "covered_pixels")


def register_ref(depth, depth_scale, K_depth, T, min_z, fill, size, K, dtype=np.float32):
    """depth: uint16 [dh, dw]; K_depth, K = (fx, fy, ox, oy) of the depth and of the colour camera; T: 4x4 depth camera -> colour
    camera (row-major numpy); size = (width, height) of the colour image."""
    D = dtype
    U = np.uint32 if D == np.float32 else np.uint64
    empty = U(0x7FC00000) if D == np.float32 else U(0x7FF8000000000000)
    depth = np.asarray(depth, np.uint16)
    dh, dw = depth.shape
    w, h = int(size[0]), int(size[1])
    fxd, fyd, oxd, oyd = [D(k) for k in K_depth]
    fx, fy, ox, oy = [D(k) for k in K]
    Tf = np.asarray(T, np.float64)[:3, :].astype(D)
    mx, my = D(fx / fxd), D(fy / fyd)
    scale, min_z = D(depth_scale), D(min_z)
    vv, uu = np.nonzero(depth)                                # scan order; the result does not depend on it
    stats = dict.fromkeys(COUNTERS, 0)
    stats["measurements"] = int(uu.size)
    zbuf = np.full(w * h, empty, U)
    with np.errstate(all="ignore"):
        z = depth[vv, uu].astype(D) * scale
        rx, ry = (uu.astype(D) - oxd) / fxd, (vv.astype(D) - oyd) / fyd
        X, Y = rx * z, ry * z
        cx, cy, cz = [((Tf[r, 0] * X + Tf[r, 1] * Y) + Tf[r, 2] * z) + Tf[r, 3] for r in range(3)]
        keep = cz > min_z                                     # False for NaN
        stats["behind"] = int((~keep).sum())
        z, cx, cy, cz = z[keep], cx[keep], cy[keep], cz[keep]
        uc, vc = (cx * fx) / cz + ox, (cy * fy) / cz + oy
        s = z / cz
        hx, hy = np.fmin(D(0.5) * (mx * s), D(4.0)), np.fmin(D(0.5) * (my * s), D(4.0))

        def axis(c, half, n):
            a, b = np.ceil(c - half), np.floor(c + half)
            nearest = (b < a) if fill else np.ones(c.shape, bool)
            a, b = np.where(nearest, np.floor(c + D(0.5)), a), np.where(nearest, np.floor(c + D(0.5)), b)
            last = D(n - 1)
            vis = (b >= 0) & (a <= last)
            lo = np.where(vis & (a > 0), a, 0).astype(np.int64)
            hi = np.where(vis & (b < last), b, n - 1).astype(np.int64)
            return vis, lo, hi

        vx, x0, x1 = axis(uc, hx, w)
        vy, y0, y1 = axis(vc, hy, h)
    draw = vx & vy
    stats["drawn"], stats["outside"] = int(draw.sum()), int((~draw).sum())
    x0, x1, y0, y1, word = x0[draw], x1[draw], y0[draw], y1[draw], np.ascontiguousarray(cz[draw]).view(U)
    for dy in range(int((y1 - y0).max()) + 1 if word.size else 0):
        for dx in range(int((x1 - x0).max()) + 1):
            m = (x0 + dx <= x1) & (y0 + dy <= y1)
            np.minimum.at(zbuf, (y0[m] + dy) * w + (x0[m] + dx), word[m])
    stats["covered_pixels"] = int((zbuf != empty).sum())
    return zbuf.view(D).reshape(h, w), stats


def _r(v):
    """round a Python float (a double) to float32; the sum, difference, product or quotient of two float32 values rounded to
    double and then to float32 is the correctly rounded float32 result (53 >= 2 * 24 + 2)"""
    with np.errstate(over="ignore"):
        return float(F(v))


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _floor(v):
    return float(math.floor(v)) if math.isfinite(v) else v


def _ceil(v):
    return float(math.ceil(v)) if math.isfinite(v) else v


def _fmin(a, b):
    """fminf: the other operand for a NaN"""
    if a != a:
        return b
    if b != b:
        return a
    return min(a, b)


def _mul(a, b):
    return _r(a * b)


def register_brute(depth, depth_scale, K_depth, T, min_z, fill, size, K):
    depth = np.asarray(depth, np.uint16)
    dh, dw = depth.shape
    w, h = int(size[0]), int(size[1])
    fxd, fyd, oxd, oyd = [_r(float(k)) for k in K_depth]
    fx, fy, ox, oy = [_r(float(k)) for k in K]
    Tf = [[_r(float(np.asarray(T, np.float64)[r, c])) for c in range(4)] for r in range(3)]
    mx, my = _r(fx / fxd), _r(fy / fyd)
    scale, min_z = _r(float(depth_scale)), _r(float(min_z))
    stats = dict.fromkeys(COUNTERS, 0)
    zbuf = {}

    def axis(c, half, n):
        """the covered pixels of one axis, or None"""
        a, b = _ceil(_r(c - half)), _floor(_r(c + half))
        if not fill or b < a:
            a = b = _floor(_r(c + 0.5))
        last = float(n - 1)
        if not (b >= 0.0 and a <= last):                      # False for NaN
            return None
        return range(int(a) if a > 0.0 else 0, (int(b) if b < last else n - 1) + 1)

    for v in range(dh):
        for u in range(dw):
            d = int(depth[v, u])
            if d == 0:
                continue
            stats["measurements"] += 1
            z = _mul(float(d), scale)
            rx, ry = _r(_r(float(u) - oxd) / fxd), _r(_r(float(v) - oyd) / fyd)
            X, Y = _mul(rx, z), _mul(ry, z)
            cx, cy, cz = [_r(_r(_r(_mul(Tf[r][0], X) + _mul(Tf[r][1], Y)) + _mul(Tf[r][2], z)) + Tf[r][3]) for r in range(3)]
            if not cz > min_z:
                stats["behind"] += 1
                continue
            uc, vc = _r(_r(_mul(cx, fx) / cz) + ox), _r(_r(_mul(cy, fy) / cz) + oy)
            s = _r(z / cz)
            hx, hy = _fmin(_mul(0.5, _mul(mx, s)), 4.0), _fmin(_mul(0.5, _mul(my, s)), 4.0)
            cols, rows = axis(uc, hx, w), axis(vc, hy, h)
            if cols is None or rows is None:
                stats["outside"] += 1
                continue
            stats["drawn"] += 1
            word = _bits(cz)
            for yy in rows:
                for xx in cols:
                    if zbuf.get((yy, xx), 0x7FC00000) > word:
                        zbuf[(yy, xx)] = word
    plane = np.full((h, w), 0x7FC00000, np.uint32)
    for (yy, xx), word in zbuf.items():
        plane[yy, xx] = word
    stats["covered_pixels"] = len(zbuf)
    return plane.view(F), stats


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_plane(a, b):
    """bit for bit, the NaN payload included: an empty pixel is 0x7FC00000 by the rule"""
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(bits(a), bits(b))
