"""The numpy restatement of the map render rule (dvo_amd.h: dvo_amd_map_render), operation for operation in fp32, and a second,
independent form of it.

`render_ref(xyz, rgb, leaf, pose, view)` works on what KeyframeMap.extract() returns: it projects every voxel with array
operations and takes the minimum of (bits(cz) << 32) | rank over every footprint, voxel by voxel.
`render_brute` asks per pixel: which voxels' footprints contain me, and which of them has the least (depth bits, rank)?  It
projects voxel by voxel with fp32 scalars and compares the pixel with the float bounds of the footprint; it never forms a
clamped integer range.
Both return {"depth", "rgb", "intensity", "index", "stats", "info"}; "info" describes what the case exercised."""
from collections import namedtuple

import numpy as np

View = namedtuple("View", "width height fx fy ox oy near_z")
F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def make_view(width, height, K, near_z):
    fx, fy, ox, oy = [F(k) for k in K]
    return View(int(width), int(height), fx, fy, ox, oy, F(near_z))


def near_limit(leaf, K):
    """the smallest near_z the entry accepts: (leaf * max(fx, fy)) / 32 in fp32"""
    return (F(leaf) * max(F(K[0]), F(K[1]))) / F(32)


def default_near(leaf, K):
    return max(F(0.1), near_limit(leaf, K))


def inverse_pose(pose):
    """rule 2: the inverse of a rigid pose in double, every product and sum rounded on its own, cast to float: [3, 4]"""
    P = np.eye(4) if pose is None else np.asarray(pose, np.float64).reshape(4, 4)
    T = np.empty((3, 4), F)
    for r in range(3):
        for c in range(3):
            T[r, c] = F(P[c, r])
        T[r, 3] = F(-((P[0, r] * P[0, 3] + P[1, r] * P[1, 3]) + P[2, r] * P[2, 3]))
    return T


def grey(rgb):
    """the ingest's grey rule on packed 0x00RRGGBB"""
    c = np.asarray(rgb).astype(np.int64)
    return ((1868 * (c & 0xFF) + 9617 * ((c >> 8) & 0xFF) + 4899 * ((c >> 16) & 0xFF) + 8192) >> 14).astype(F)


def _resolve(zbuf, rgb, view):
    covered = zbuf != EMPTY
    index = np.where(covered, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(covered, (zbuf >> np.uint64(32)).astype(np.uint32), np.uint32(0x7FC00000)).astype(np.uint32).view(F)
    at = np.where(covered, index, 0)
    col = np.where(covered, rgb[at] if len(rgb) else 0, 0).astype(np.uint32)
    inten = np.where(covered, grey(col), F(0)).astype(F)
    shape = (view.height, view.width)
    return depth.reshape(shape), col.reshape(shape), inten.reshape(shape), index.reshape(shape), int(covered.sum())


def _axis(c, half, size):
    """rule 5 on one axis, arrays: (lo, hi as float, fallback, visible)"""
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = np.ceil(c - half), np.floor(c + half)
        fb = b < a
        mid = np.floor(c + F(0.5))
        a, b = np.where(fb, mid, a), np.where(fb, mid, b)
        vis = (b >= F(0)) & (a <= F(size - 1))
    return a, b, fb, vis


def render_ref(xyz, rgb, leaf, pose, view):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint32).reshape(-1)
    n, leaf = len(xyz), F(leaf)
    T = inverse_pose(pose)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)]
        cx, cy, cz = c
        ahead = cz >= view.near_z
        u = (cx * view.fx) / cz + view.ox
        v = (cy * view.fy) / cz + view.oy
        hx = F(0.5) * ((leaf * view.fx) / cz)
        hy = F(0.5) * ((leaf * view.fy) / cz)
    u0, u1, fbx, visx = _axis(u, hx, view.width)
    v0, v1, fby, visy = _axis(v, hy, view.height)
    drawn = ahead & visx & visy
    zbuf = np.full((view.height, view.width), EMPTY, np.uint64)
    cand = np.zeros((view.height, view.width), np.int64)
    words = (cz.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    lastx, lasty = F(view.width - 1), F(view.height - 1)
    max_side = clamped = 0
    for r in np.flatnonzero(drawn):
        x0 = int(u0[r]) if u0[r] > 0 else 0
        x1 = int(u1[r]) if u1[r] < lastx else view.width - 1
        y0 = int(v0[r]) if v0[r] > 0 else 0
        y1 = int(v1[r]) if v1[r] < lasty else view.height - 1
        clamped += bool(u0[r] < 0 or u1[r] > lastx or v0[r] < 0 or v1[r] > lasty)
        max_side = max(max_side, x1 - x0 + 1, y1 - y0 + 1)
        zbuf[y0:y1 + 1, x0:x1 + 1] = np.minimum(zbuf[y0:y1 + 1, x0:x1 + 1], words[r])
        cand[y0:y1 + 1, x0:x1 + 1] += 1
    depth, col, inten, index, covered = _resolve(zbuf.ravel(), rgb, view)
    stats = {"voxels": n, "behind_near": int((~ahead).sum()), "outside": int((ahead & ~drawn).sum()), "drawn": int(drawn.sum()),
             "covered_pixels": covered}
    info = {"fallback": int((drawn & (fbx | fby)).sum()), "max_side": max_side, "clamped": clamped, "candidates": cand,
            "multi": int((cand > 1).sum()), "coverage": covered / float(view.width * view.height)}
    return {"depth": depth, "rgb": col, "intensity": inten, "index": index, "stats": stats, "info": info}


def _axis_scalar(c, half):
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = F(np.ceil(c - half)), F(np.floor(c + half))
        if b < a:
            a = b = F(np.floor(c + F(0.5)))
    return a, b


def render_brute(xyz, rgb, leaf, pose, view):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint32).reshape(-1)
    n, leaf = len(xyz), F(leaf)
    T = inverse_pose(pose)
    lo = np.full((n, 2), np.inf, F)    # float bounds of the footprints of the voxels in front of near_z; (inf, -inf): none
    hi = np.full((n, 2), -np.inf, F)
    bits = np.zeros(n, np.uint64)
    behind = outside = 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r in range(n):
            p = [F(t) for t in xyz[r]]
            cx, cy, cz = [F(F(F(F(T[k, 0] * p[0]) + F(T[k, 1] * p[1])) + F(T[k, 2] * p[2])) + T[k, 3]) for k in range(3)]
            if not cz >= view.near_z:
                behind += 1
                continue
            u = F(F(F(cx * view.fx) / cz) + view.ox)
            v = F(F(F(cy * view.fy) / cz) + view.oy)
            a0, a1 = _axis_scalar(u, F(F(0.5) * F(F(leaf * view.fx) / cz)))
            b0, b1 = _axis_scalar(v, F(F(0.5) * F(F(leaf * view.fy) / cz)))
            if not (a1 >= 0 and a0 <= F(view.width - 1) and b1 >= 0 and b0 <= F(view.height - 1)):
                outside += 1
                continue
            lo[r], hi[r] = (a0, b0), (a1, b1)
            bits[r] = np.uint64(int(np.array(cz, F).view(np.uint32))) << np.uint64(32)
    words = bits | np.arange(n, dtype=np.uint64)
    zbuf = np.full(view.height * view.width, EMPTY, np.uint64)
    ties = 0
    for py in range(view.height):
        rows = (lo[:, 1] <= F(py)) & (F(py) <= hi[:, 1])
        if not rows.any():
            continue
        for px in range(view.width):
            inside = np.flatnonzero(rows & (lo[:, 0] <= F(px)) & (F(px) <= hi[:, 0]))
            if len(inside):
                w = words[inside]
                zbuf[py * view.width + px] = w.min()
                ties += int(((w >> np.uint64(32)) == (w.min() >> np.uint64(32))).sum() > 1)
    depth, col, inten, index, covered = _resolve(zbuf, rgb, view)
    stats = {"voxels": n, "behind_near": behind, "outside": outside, "drawn": n - behind - outside, "covered_pixels": covered}
    return {"depth": depth, "rgb": col, "intensity": inten, "index": index, "stats": stats, "info": {"ties": ties}}
