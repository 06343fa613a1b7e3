"""Shared pieces of tests/test_selection_mask.py and tests/test_selection_mask_adaptor.py: the level-0 mask with the edge cases a
mask pyramid can get wrong, the numpy restatement of the two reduction rules and of the threshold predicate, and a bit-for-bit
comparison of two tracking results."""
import numpy as np


def level0_mask(w: int, h: int) -> np.ndarray:
    """uint8 [h, w], non-zero = keep.  A cut-out rectangle that is aligned to nothing (odd corners: its edge cuts 2x2 blocks of
    every level), isolated dropped pixels, an isolated kept pixel inside the cut-out, a dropped patch in the bottom-right corner
    whose last-row / last-column pixel is kept, and keep bytes other than 1 (the planes are stored normalised)."""
    m = np.ones((h, w), np.uint8)
    y0, y1, x0, x1 = (3 * h) // 10 + 1, (5 * h) // 8 - 1, w // 3 - 2, (2 * w) // 3 + 3
    m[y0:y1, x0:x1] = 0
    m[(y0 + y1) // 2, (x0 + x1) // 2] = 1          # one kept pixel in the middle of the cut-out
    for y, x in ((1, 1), (2, w - 2), (h // 2, 2), (h - 2, w // 2 + 1), (5, w // 2)):
        m[y, x] = 0                                 # isolated dropped pixels
    m[h - 3:, w - 5:] = 0
    m[h - 1, w - 1] = 1                             # kept, in the last row and the last column
    m[0, :] *= 255                                  # any non-zero byte keeps
    m[:, 0] *= 7
    return m


def reduce_mask(m: np.ndarray, rule_any: bool) -> np.ndarray:
    """level l + 1 of a mask from level l: all / any of each 2x2 block; an odd trailing row or column has no parent"""
    h, w = m.shape[0] // 2, m.shape[1] // 2
    b = (m[:2 * h, :2 * w] != 0).reshape(h, 2, w, 2)
    return (b.any(axis=(1, 3)) if rule_any else b.all(axis=(1, 3))).astype(np.uint8)


def mask_pyramid(m0: np.ndarray, levels: int, rule_any: bool):
    out = [(m0 != 0).astype(np.uint8)]
    for _ in range(1, levels):
        out.append(reduce_mask(out[-1], rule_any))
    return out


def threshold_predicate(pyramid, level: int, ti: float, td: float) -> np.ndarray:
    """ValidPointAndGradientThresholdPredicate(ti, td) of every pixel of a level from its downloaded planes (point_selection.h:
    49-67), in float32 like the kernel; ti = td = -1 leaves validity only"""
    z, ix, iy, zx, zy = (pyramid.plane(level, k) for k in (1, 2, 3, 4, 5))
    ti, td = np.float32(ti), np.float32(td)
    valid = ~np.isnan(z) & ~np.isnan(zx) & ~np.isnan(zy)
    with np.errstate(invalid="ignore"):
        grad = (np.abs(ix) > ti) | (np.abs(iy) > ti) | (np.abs(zx) > td) | (np.abs(zy) > td)
    return (valid & grad).astype(np.uint8)


def same_result(a, b) -> bool:
    """two capi.Result bit for bit: transformation, information, log-likelihood, every level and iteration record"""
    eq = lambda x, y: np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)  # noqa: E731
    if not (eq(a.Transformation, b.Transformation) and eq(a.Information, b.Information) and eq(a.LogLikelihood, b.LogLikelihood)):
        return False
    if a.isNaN() != b.isNaN() or len(a.Levels) != len(b.Levels):
        return False
    for la, lb in zip(a.Levels, b.Levels):
        if any(la[k] != lb[k] for k in ("Id", "MaxValidPixels", "ValidPixels", "TerminationCriterion")):
            return False
        if len(la["Iterations"]) != len(lb["Iterations"]):
            return False
        for ia, ib in zip(la["Iterations"], lb["Iterations"]):
            if ia.keys() != ib.keys() or not all(eq(ia[k], ib[k]) for k in ia):
                return False
    return True


def pose_checksum(T) -> float:
    """the sum the examples print: the sixteen doubles of the C ABI's column-major transformation, added in that order"""
    s = 0.0
    for v in np.asarray(T, dtype=np.float64).T.ravel():
        s += float(v)
    return s
