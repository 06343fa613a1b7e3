"""Restatement of what pose scoring adds to the residual-mask rule (include/dvo_amd.h, "Pose scoring") in numpy.

q           q(x) = (uint32) floor(x * 1024.0f) in fp32, 0 for x < 0
pixel_cost  the cost plane of one hypothesis from its outcome and distance planes
score_ref   the six sums of one hypothesis
scores_ref  ... of many, as records
rank_ref    the ranking by total, ties to the lower index
grid_ref    the hypothesis grid as a loop over synth.se3_exp

The residual stage, the distance and the four outcomes (Q3 included) are NOT restated here: the outcome plane and the distance
plane of a hypothesis come from residual_mask_ref.residual_mask_ref fed with a residual image."""
import itertools

import numpy as np

import residual_mask_ref as rm

F = np.float32
FIELDS = ("evaluated", "invalid", "inlier", "outlier", "cost", "total")
MAX_DISTANCE = rm.MAX_DISTANCE


def q(x):
    """fp32 product (exact: a power of two), floor, uint32; negative x (a precision that is not positive semidefinite) gives 0"""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        p = np.maximum(x, F(0.0)) * F(1024.0)
    assert p.dtype == F
    return np.floor(np.where(np.isnan(p), F(0.0), p)).astype(np.uint32)


def pixel_cost(outcome, distance, max_distance=MAX_DISTANCE):
    """uint32 per pixel: q(d) for an inlier, q(max_distance) for an outlier (a NaN d included), 0 otherwise"""
    cost = np.zeros(outcome.shape, np.uint32)
    inlier = outcome == rm.INLIER
    cost[inlier] = q(distance[inlier])
    cost[outcome == rm.OUTLIER] = q(F(max_distance))
    return cost


def score_ref(outcome, distance, max_distance=MAX_DISTANCE, invalid_distance=-1.0):
    """the record of one hypothesis as a dict of python ints"""
    invalid, inlier, outlier = (int((outcome == c).sum()) for c in (rm.INVALID, rm.INLIER, rm.OUTLIER))
    cost = int(pixel_cost(outcome, distance, max_distance).astype(np.uint64).sum())
    charged = F(max_distance) if F(invalid_distance) < 0 else F(invalid_distance)
    return dict(evaluated=invalid + inlier + outlier, invalid=invalid, inlier=inlier, outlier=outlier, cost=cost,
                total=cost + invalid * int(q(charged)))


def scores_ref(evaluated, images, P, max_distance=MAX_DISTANCE, invalid_distance=-1.0):
    """one record per residual image (one per hypothesis) of a level whose validity predicate is `evaluated`"""
    out = []
    for image in images:
        _, distance, counts, outcome = rm.residual_mask_ref(evaluated, image, P, max_distance)
        s = score_ref(outcome, distance, max_distance, invalid_distance)
        assert all(s[k] == counts[k] for k in ("evaluated", "invalid", "inlier", "outlier"))
        out.append(s)
    return out


def as_ints(records):
    """device records (a structured array) as the dicts score_ref returns"""
    return [{k: int(r[k]) for k in FIELDS} for r in records]


def rank_ref(totals, k):
    return np.argsort(np.asarray(totals, np.uint64), kind="stable")[:k]


def grid_ref(se3_exp, T_centre, counts, steps):
    """Exp(xi) @ T_centre for xi over the grid, (vx, vy, vz, wx, wy, wz) with wz fastest; the middle entry is the centre itself"""
    axes = [[(i - (c - 1) // 2) * s for i in range(c)] for c, s in zip(counts, steps)]
    out = []
    for xi in itertools.product(*axes):
        out.append(np.array(T_centre, np.float64) if not any(xi) else se3_exp(np.array(xi)) @ np.asarray(T_centre, np.float64))
    return np.stack(out)
