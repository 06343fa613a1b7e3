"""Restatement of the residual-mask rule (include/dvo_amd.h, "Residual masks") in numpy, fp32, every operation rounded on its own.

evaluated_ref      the validity predicate of a level from its planes: z, zdx, zdy are no NaN
distance_ref       the Mahalanobis distance of residual pairs under a column-major 2x2 precision, in mahalanobis()'s order
residual_mask_ref  one level: the mask plane, the distance plane and the five counts from the predicate and a residual image
residual_image     the residual image (NaN = no residual) of a level from the oracle's compacted output

The residual stage itself is NOT restated here: the residual image comes from dvo_amd_residuals of a tracker configured with
thresholds (-1, -1) or from the oracle's compute_residuals(..., ti=-1, td=-1).  Both walk the validity selection two points at
a time and never reach an odd trailing point (Q3), so both leave NaN there and the rule calls that pixel invalid."""
import numpy as np

F = np.float32
COUNTS = ("evaluated", "invalid", "inlier", "outlier", "kept")
MAX_DISTANCE = F(9.2103)
UNEVALUATED, INVALID, INLIER, OUTLIER = -1, 1, 2, 3  # (the outcome of a pixel; the numbers are the count's index)


def evaluated_ref(z, zx, zy):
    return ~np.isnan(z) & ~np.isnan(zx) & ~np.isnan(zy)


def precision_cm(P):
    """a precision as the four floats of the C ABI: a 2x2 matrix goes in column-major, four numbers stay as they are"""
    P = np.asarray(P)
    return np.ascontiguousarray(P.T if P.shape == (2, 2) else P, F).ravel()


def distance_ref(r0, r1, P):
    """t0 = r0 P[0] + r1 P[1], t1 = r0 P[2] + r1 P[3], d = t0 r0 + t1 r1; float32 arrays: numpy rounds every product and sum"""
    r0, r1 = np.asarray(r0, F), np.asarray(r1, F)
    P = precision_cm(P)
    with np.errstate(invalid="ignore", over="ignore"):
        t0 = r0 * P[0] + r1 * P[1]
        t1 = r0 * P[2] + r1 * P[3]
        d = t0 * r0 + t1 * r1
    assert d.dtype == F
    return d


def residual_mask_ref(evaluated, residuals, P, max_distance=MAX_DISTANCE, invalid_keep=0, unevaluated_keep=0):
    """(plane uint8 [h, w], distance float32 [h, w], counts dict, outcome int8 [h, w]) of one level.  evaluated: bool [h, w];
    residuals: float32 [h, w, 2], NaN where there is no valid residual pair"""
    evaluated = np.asarray(evaluated, bool)
    res = np.asarray(residuals, F)
    assert res.shape == evaluated.shape + (2,)
    has = ~np.isnan(res[..., 0])
    assert np.array_equal(has, ~np.isnan(res[..., 1])) and not (has & ~evaluated).any()  # a residual only where the predicate holds
    d = distance_ref(res[..., 0], res[..., 1], P)
    with np.errstate(invalid="ignore"):
        inlier = has & (d <= F(max_distance))  # (a NaN distance of a valid pair -- an overflow -- is an outlier)
    outcome = np.full(evaluated.shape, UNEVALUATED, np.int8)
    outcome[evaluated] = INVALID
    outcome[has] = OUTLIER
    outcome[inlier] = INLIER
    plane = np.where(outcome == INLIER, 1, 0).astype(np.uint8)
    plane[outcome == INVALID] = 1 if invalid_keep else 0
    plane[outcome == UNEVALUATED] = 1 if unevaluated_keep else 0
    distance = np.where(has, d, F(np.nan)).astype(F)
    counts = dict(evaluated=int(evaluated.sum()), invalid=int((outcome == INVALID).sum()), inlier=int((outcome == INLIER).sum()),
                  outlier=int((outcome == OUTLIER).sum()), kept=int(plane.sum()))
    assert counts["evaluated"] == counts["invalid"] + counts["inlier"] + counts["outlier"]
    return plane, distance, counts, outcome


def residual_image(shape, index, valid, residuals):
    """the oracle's compacted output back in the image: index[k] = the pixel of the k-th selected point, valid[k] for the points it
    processed (an odd trailing point is not among them), residuals = the pairs of the valid ones in order"""
    h, w = shape
    img = np.full((h * w, 2), np.nan, F)
    valid = np.asarray(valid).astype(bool)
    at = np.asarray(index)[:len(valid)][valid]
    assert len(at) == len(residuals)
    img[at] = residuals
    return img.reshape(h, w, 2)


def same_bits(a, b):
    """two float32 arrays bit for bit, NaN positions equal (any NaN payload: the positions are what the rule pins)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a.view(np.uint32)[ok], b.view(np.uint32)[ok])
