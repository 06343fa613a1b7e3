"""Restatement of the mask operations (include/dvo_amd.h, "Mask operations") in numpy.

combine_ref   the four boolean ops on one level
morph_ref     dilate / erode by a square window clipped to the plane, as a shifted-window any / all (rows, then columns: a
              square's any / all over a clipped window is the any / all of its rows' any / all)
morph_brute   the same rule as an independent pixel loop
warp_ref      the warp of one level, built on covisibility_ref.covis_ref(target, source, T, I): with an identity second pose that
              helper's pinned double arithmetic reduces to the float cast of T, and it returns the outcome and the landing pixel
              of every target pixel
level_radii   the per-level radii of a level-0 radius

A mask plane is uint8 or bool [h, w], non-zero = keep; every result is uint8 of 0 / 1."""
import numpy as np

from covisibility_ref import covis_ref

AND, OR, ANDNOT, NOT = 0, 1, 2, 3
DILATE, ERODE = 0, 1
MAX_RADIUS = 64
WARP_COUNTS = ("valid", "behind", "outside", "no_depth", "consistent", "occluded", "seen_through", "dropped_by_source")
WARP_DEFAULTS = dict(near_z=0.1, depth_sigmas=20.0, unseen_keep=1, inconsistent_keep=1)
CONSISTENT, OCCLUDED, SEEN_THROUGH = 4, 5, 6


def level_radii(r0, levels):
    return [(r0 + (1 << l) - 1) >> l for l in range(levels)]


def combine_ref(a, b, op):
    a = np.asarray(a) != 0
    if op == NOT:
        assert b is None
        return (~a).astype(np.uint8)
    b = np.asarray(b) != 0
    assert a.shape == b.shape
    return {AND: a & b, OR: a | b, ANDNOT: a & ~b}[op].astype(np.uint8)


def _shifted(m, r, axis, fill):
    """the 2 r + 1 copies of m shifted by -r..r along `axis`, `fill` where a copy has no pixel"""
    n = m.shape[axis]
    for s in range(-min(r, n), min(r, n) + 1):  # (a shift of n or more has no pixel anywhere)
        out = np.full(m.shape, fill, bool)
        src = [slice(None)] * 2
        dst = [slice(None)] * 2
        src[axis] = slice(max(0, s), n + min(0, s))
        dst[axis] = slice(max(0, -s), n - max(0, s))
        out[tuple(dst)] = m[tuple(src)]
        yield out


def morph_ref(m, op, r):
    """pixels outside the plane have no vote: they are False for any (dilate) and True for all (erode)"""
    m = np.asarray(m) != 0
    assert 0 <= r
    erode = op == ERODE
    for axis in (1, 0):
        acc = np.full(m.shape, erode, bool)
        for s in _shifted(m, r, axis, erode):
            acc = (acc & s) if erode else (acc | s)
        m = acc
    return m.astype(np.uint8)


def morph_brute(m, op, r):
    m = np.asarray(m) != 0
    h, w = m.shape
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            win = [bool(m[v, u]) for v in range(max(0, y - r), min(h, y + r + 1)) for u in range(max(0, x - r), min(w, x + r + 1))]
            out[y, x] = all(win) if op == ERODE else any(win)
    return out


def warp_ref(mask_source, planes_target, planes_source, T, options=None):
    """(plane uint8 [ht, wt], counts dict) of one level.  planes_*: (Z, K) as covisibility_ref takes them; mask_source: the mask's
    plane on the source's pixels; T: 4x4 row-major, target camera frame -> source camera frame"""
    o = dict(WARP_DEFAULTS, **(options or {}))
    info = covis_ref(planes_target, planes_source, T, np.eye(4), dict(near_z=o["near_z"], depth_sigmas=o["depth_sigmas"]), info=True)
    assert np.array_equal(info["T"], np.asarray(T, np.float64)[:3].astype(np.float32), equal_nan=True)  # the float cast of T, no more
    cls = info["cls"]
    ms = np.asarray(mask_source) != 0
    assert ms.shape == np.shape(planes_source[0])
    consistent = cls == CONSISTENT
    iu = np.where(consistent, info["pu"], 0).astype(np.int64)
    iv = np.where(consistent, info["pv"], 0).astype(np.int64)
    out = np.full(cls.shape, bool(o["unseen_keep"]))
    out[(cls == OCCLUDED) | (cls == SEEN_THROUGH)] = bool(o["inconsistent_keep"])
    gathered = ms[iv, iu]
    out[consistent] = gathered[consistent]
    counts = {k: info[k] for k in WARP_COUNTS[:7]}
    counts["dropped_by_source"] = int((consistent & ~gathered).sum())
    return out.astype(np.uint8), counts
