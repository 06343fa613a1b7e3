"""Shared pieces of tests/test_budget_selection.py and tests/test_budget_selection_adaptor.py: the numpy restatement of the
point-budget rules pinned in include/dvo_amd.h (saliency, candidates, the (key descending, index ascending) order, TOPK and
GRID), working from a pyramid's downloaded planes, and the frames whose keys tie, span the radix digits or empty whole cells."""
import numpy as np

import selection_mask_cases as cases


def saliency(pyramid, level: int, depth_weight: float) -> np.ndarray:
    """s of every pixel of a level, float32 [h, w]: every product and sum rounded by itself, in the pinned association; the
    depth term is not formed for depth_weight == 0"""
    ix, iy, zx, zy = (pyramid.plane(level, k) for k in (2, 3, 4, 5))
    with np.errstate(all="ignore"):
        s = ix * ix + iy * iy
        if depth_weight != 0.0:
            s = s + np.float32(depth_weight) * (zx * zx + zy * zy)
    assert s.dtype == np.float32
    return s


def keys_and_candidates(pyramid, level: int, ti: float = 0.0, td: float = 0.0, depth_weight: float = 0.0, within=None):
    """(key uint32 [h, w], candidate bool [h, w]); within: the level's plane of a mask (non-zero = keep) or None"""
    s = saliency(pyramid, level, depth_weight)
    cand = (cases.threshold_predicate(pyramid, level, ti, td) != 0) & ~np.isnan(s)
    if within is not None:
        cand &= np.asarray(within) != 0
    return np.ascontiguousarray(s).view(np.uint32), cand


def order(key: np.ndarray, cand: np.ndarray) -> np.ndarray:
    """the pixel indices of the candidates by (key descending, index ascending)"""
    idx = np.flatnonzero(cand.ravel())
    k = key.ravel()[idx].astype(np.int64)
    return idx[np.lexsort((idx, -k))]


def topk_plane(key: np.ndarray, cand: np.ndarray, budget: int) -> np.ndarray:
    o = order(key, cand)
    keep = len(o) if budget < 0 else min(int(budget), len(o))
    plane = np.zeros(key.size, np.uint8)
    plane[o[:keep]] = 1
    return plane.reshape(key.shape)


def grid_plane(key: np.ndarray, cand: np.ndarray, cell: int) -> np.ndarray:
    """every cell's first candidate in the order: the first time the cell shows up when the candidates are walked in order"""
    h, w = key.shape
    o = order(key, cand)
    cell_of = (o // w // cell) * ((w + cell - 1) // cell) + (o % w) // cell
    _, first = np.unique(cell_of, return_index=True)
    plane = np.zeros(key.size, np.uint8)
    plane[o[first]] = 1
    return plane.reshape(h, w)


def tie_group(key: np.ndarray, cand: np.ndarray, at_least: int = 3):
    """(a, b): positions [a, b) of the order hold one key and b - a >= at_least (the first such group): a budget K with
    a < K < b cuts through it.  None if no key is shared that often."""
    o = order(key, cand)
    k = key.ravel()[o]
    starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    ends = np.r_[starts[1:], len(k)]
    for a, b in zip(starts, ends):
        if b - a >= at_least:
            return int(a), int(b)
    return None


def raw_tie_frame(w: int = 32, h: int = 30, seed: int = 3):
    """uint8 grey of two values and uint16 depth of two planes that meet in the middle column, so that the derivatives --
    multiples of 0.5 on level 0 -- and with them the keys tie in large groups on every level, with and without the depth term; a
    block of depth 0 (no measurement) at the left edge that holds whole cells of 2, 3 and 7 pixels"""
    rng = np.random.default_rng(seed)
    grey = rng.integers(0, 2, size=(h, w)).astype(np.uint8) * 64
    depth = np.where(np.arange(w) < w // 2, 5000, 6000).astype(np.uint16)[None, :].repeat(h, axis=0)
    depth[14:28, 0:14] = 0
    return grey, depth


def nan_patch(Z: np.ndarray, x0: int = 28, y0: int = 28, size: int = 40) -> np.ndarray:
    """a copy of a depth plane with a square of NaN that holds whole cells of 2, 3 and 7 pixels on level 0"""
    Z = Z.copy()
    Z[y0:y0 + size, x0:x0 + size] = np.nan
    return Z


def ramp_frame(w: int = 32, h: int = 30):
    """I = 2x + 3y over depth 1: every interior pixel of every level has Ix = 2 * 2^l, Iy = 3 * 2^l, one key"""
    y, x = np.mgrid[0:h, 0:w]
    return (2.0 * x + 3.0 * y).astype(np.float32), np.ones((h, w), np.float32)


def digit_frame(w: int = 32, h: int = 30, seed: int = 17):
    """A float frame for the edges of the radix select.  Intensities of random sign and magnitude 2^-12 .. 2^12: the squared
    gradients span far more than 20 binades.  Rows 10..12 are one row, 0, ., a_m, ., 0, ., a_m+1 ... with a_m = 2 + m * 2^-22,
    so on row 11 Iy = 0 and Ix = +-(1 + m * 2^-23): keys that differ in their lowest mantissa bits only.  (20, 5) = 0 and
    (20, 7) = 4e19 put Ix = 2e19 at (20, 6), whose square is +inf."""
    rng = np.random.default_rng(seed)
    I = (rng.choice([-1.0, 1.0], size=(h, w)) * np.exp2(rng.uniform(-12.0, 12.0, size=(h, w)))).astype(np.float32)
    row = np.zeros(w, np.float32)
    for m in range(w // 4):
        row[4 * m + 2] = np.float32(2.0) + np.float32(m) * np.float32(2.0 ** -22)
    I[10:13, :] = row
    I[20, 5], I[20, 7] = 0.0, 4e19
    Z = np.full((h, w), 1.5, np.float32)
    return I, Z
