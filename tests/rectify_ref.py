"""The two rules of the rectifying ingest (include/dvo_amd.h: "The undistortion rule", "The sampling rule") restated in numpy,
every operation in float32 in the pinned order, and the sampling rule once more as a per-pixel loop over Python floats that are
rounded to float32 after every operation (remap_brute) -- two independent statements the tests hold against each other and
against the library.  Nothing here imports the library."""
import math

import numpy as np

F = np.float32
NAN = F(np.nan)


def undistort_map_ref(size, K_out, src_size, K_src, dist, dtype=np.float32):
    """(map_x, map_y) [h, w] of the five-coefficient model, in `dtype` throughout (float32: the library's rule; float64: the same
    formula, against which the float32 error is capped).  src_size is not read: the map does not depend on it."""
    T = dtype
    w, h = size
    fx, fy, ox, oy = [T(F(k)) for k in K_out]          # the library receives floats: the float64 form starts from the same numbers
    fxs, fys, oxs, oys = [T(F(k)) for k in K_src]
    k1, k2, p1, p2, k3 = [T(F(k)) for k in dist]
    u = np.arange(w, dtype=T)[None, :].repeat(h, 0)
    v = np.arange(h, dtype=T)[:, None].repeat(w, 1)
    x = (u - ox) / fx
    y = (v - oy) / fy
    xx, yy = x * x, y * y
    r2 = xx + yy
    xy = x * y
    rad = ((k3 * r2 + k2) * r2 + k1) * r2 + T(1)
    two_p1, two_p2 = T(2) * p1, T(2) * p2
    xd = x * rad + ((two_p1 * xy) + p2 * (r2 + (xx + xx)))
    yd = y * rad + (p1 * (r2 + (yy + yy)) + (two_p2 * xy))
    mx = xd * fxs + oxs
    my = yd * fys + oys
    assert mx.dtype == T and my.dtype == T
    return mx, my


def grey_plane(image):
    """the grey value of every source pixel as the taps see it: the byte itself, or the integer rule of the raw ingest for B, G, R"""
    image = np.asarray(image, np.uint8)
    if image.ndim == 2:
        return image.copy()
    b, g, r = [image[..., c].astype(np.int64) for c in range(3)]
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)


def inside_ref(map_x, map_y, src_size):
    sw, sh = src_size
    mx, my = np.asarray(map_x, F), np.asarray(map_y, F)
    with np.errstate(invalid="ignore"):
        return (mx >= F(0)) & (mx < F(sw - 1)) & (my >= F(0)) & (my < F(sh - 1))


def remap_ref(image, depth, map_x, map_y, depth_scale, info=False):
    """(I, Z) float32 [h, w] of the output, and with info=True a dict of the intermediate planes as well"""
    g = grey_plane(image)
    depth = np.asarray(depth, np.uint16)
    sh, sw = depth.shape
    assert g.shape == (sh, sw)
    mx, my = np.asarray(map_x, F), np.asarray(map_y, F)
    ins = inside_ref(mx, my, (sw, sh))
    sx, sy = np.where(ins, mx, F(0)), np.where(ins, my, F(0))    # (outside pixels walk through with position 0 and are masked)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = sx - x0, sy - y0
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    ix1, iy1 = np.minimum(ix + 1, sw - 1), np.minimum(iy + 1, sh - 1)  # (only the masked pixels can need the clamp)
    assert (ix[ins] + 1 <= sw - 1).all() and (iy[ins] + 1 <= sh - 1).all()
    gf = g.astype(F)
    g00, g01, g10, g11 = gf[iy, ix], gf[iy, ix1], gf[iy1, ix], gf[iy1, ix1]
    top = g00 + ax * (g01 - g00)
    bot = g10 + ax * (g11 - g10)
    I = top + ay * (bot - top)
    px, py = np.floor(sx + F(0.5)), np.floor(sy + F(0.5))
    ipx, ipy = px.astype(np.int64), py.astype(np.int64)
    assert (ipx[ins] <= sw - 1).all() and (ipy[ins] <= sh - 1).all()
    raw = depth[np.minimum(ipy, sh - 1), np.minimum(ipx, sw - 1)]
    Z = np.where(raw == 0, NAN, raw.astype(F) * F(depth_scale))
    I = np.where(ins, I, F(0)).astype(F)
    Z = np.where(ins, Z, NAN).astype(F)
    assert ax.dtype == F and top.dtype == F and I.dtype == F and Z.dtype == F and (sx + F(0.5)).dtype == F
    if info:
        return I, Z, dict(inside=ins, n_inside=int(ins.sum()), x0=ix, y0=iy, ax=ax, ay=ay, px=ipx, py=ipy, raw=raw,
                          taps=np.stack([g00, g01, g10, g11]))
    return I, Z


def _r(v):
    """round a Python float (a double) to float32; the sum, difference or product of two float32 values rounded to double and
    then to float32 is the correctly rounded float32 result (53 >= 2 * 24 + 2)"""
    return float(F(v))


def remap_brute(image, depth, map_x, map_y, depth_scale):
    """the sampling rule pixel by pixel, on Python floats rounded to float32 after every operation: (I, Z, n_inside)"""
    image = np.asarray(image, np.uint8)
    depth = np.asarray(depth, np.uint16)
    sh, sw = depth.shape
    mx, my = np.asarray(map_x, F), np.asarray(map_y, F)
    h, w = mx.shape
    scale = _r(depth_scale)
    wmax, hmax = _r(sw - 1), _r(sh - 1)

    def tap(yy, xx):
        if image.ndim == 2:
            return float(int(image[yy, xx]))
        b, g, r = [int(c) for c in image[yy, xx]]
        return float((1868 * b + 9617 * g + 4899 * r + 8192) >> 14)

    I = np.zeros((h, w), F)
    Z = np.full((h, w), np.nan, F)
    n_inside = 0
    for v in range(h):
        for u in range(w):
            sx, sy = float(mx[v, u]), float(my[v, u])
            if not (sx >= 0.0 and sx < wmax and sy >= 0.0 and sy < hmax):   # False for NaN
                continue
            n_inside += 1
            x0, y0 = math.floor(sx), math.floor(sy)
            ax, ay = _r(sx - x0), _r(sy - y0)
            g00, g01, g10, g11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
            top = _r(g00 + _r(ax * _r(g01 - g00)))
            bot = _r(g10 + _r(ax * _r(g11 - g10)))
            I[v, u] = _r(top + _r(ay * _r(bot - top)))
            px, py = math.floor(_r(sx + 0.5)), math.floor(_r(sy + 0.5))
            raw = int(depth[py, px])
            if raw != 0:
                Z[v, u] = _r(float(raw) * scale)
    return I, Z, n_inside


def identity_maps(w, h):
    return (np.arange(w, dtype=F)[None, :].repeat(h, 0).copy(), np.arange(h, dtype=F)[:, None].repeat(w, 1).copy())


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_planes(a, b):
    """bit for bit, a NaN equal to any NaN (the payload of a NaN is not part of either rule)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])
