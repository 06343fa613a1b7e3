"""The place index restated in numpy (include/dvo_amd.h, "Place index"): the descriptor as array code and as a per-pixel loop, the
dot products as an int64 matmul, 1 / sqrt(norm), the score, eligibility and the order of a query's result.  Nothing here calls the
library; tests/test_place_index.py compares the library with this, value for value and bit for bit."""
import math

import numpy as np

F = np.float32
MAX_K, MAX_DIM, INITIAL_CAPACITY = 64, 65536, 64
DEFAULTS = {"level": 3, "gain": 1.0}
QUERY_DEFAULTS = {"k": 5, "min_score": 0.0, "exclude_recent": 0}


def dim_of(w: int, h: int) -> int:
    return 64 * ((w * h + 63) // 64)


def _quantise(d):
    """step 3 on an array of d: 0 where d is not finite, else rint (ties to even) clamped to -127 .. 127"""
    finite = np.isfinite(d)
    with np.errstate(invalid="ignore"):
        q = np.minimum(F(127), np.maximum(F(-127), np.rint(np.where(finite, d, F(0)))))
    return np.where(finite, q, F(0)).astype(np.int8)


def descriptor(I, gain=1.0):
    """(q int8 [dim], nn int): steps 1 to 3 as array code.  The nine shifted planes are added in the order rows ascending, columns
    ascending, each only where it lies inside the plane: a pixel's fp32 sum takes exactly its own neighbours in that order."""
    I = np.ascontiguousarray(I, dtype=F)
    h, w = I.shape
    s, c = np.zeros((h, w), F), np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                v0, v1, u0, u1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
                if v0 >= v1 or u0 >= u1:
                    continue
                s[v0:v1, u0:u1] = s[v0:v1, u0:u1] + I[v0 + dy:v1 + dy, u0 + dx:u1 + dx]
                c[v0:v1, u0:u1] += F(1)
        m = s / c
        d = (I - m) * F(gain)
    q = np.zeros(dim_of(w, h), np.int8)
    q[:w * h] = _quantise(d).reshape(-1)
    return q, int(np.sum(q.astype(np.int64) ** 2))


def descriptor_loop(I, gain=1.0):
    """the same, pixel by pixel, as the rule is written"""
    I = np.ascontiguousarray(I, dtype=F)
    h, w = I.shape
    q = np.zeros(dim_of(w, h), np.int8)
    with np.errstate(all="ignore"):
        for v in range(h):
            for u in range(w):
                s, c = F(0), 0
                for y in range(max(v - 1, 0), min(v + 1, h - 1) + 1):
                    for x in range(max(u - 1, 0), min(u + 1, w - 1) + 1):
                        s = F(s + I[y, x])
                        c += 1
                m = F(s / F(c))
                d = F(F(I[v, u] - m) * F(gain))
                if np.isfinite(d):
                    q[v * w + u] = int(min(F(127), max(F(-127), np.rint(d))))
    return q, int(sum(int(x) * int(x) for x in q))


def describe(planes, gain=1.0):
    """(rows int8 [n, dim], norms int32 [n]) of a list of planes of one size"""
    got = [descriptor(I, gain) for I in planes]
    return np.stack([g[0] for g in got]), np.array([g[1] for g in got], np.int32)


def dots(Q, X):
    """exact dot products [len(Q), len(X)] (they fit an int32: dim <= 65536)"""
    return np.asarray(Q, np.int64) @ np.asarray(X, np.int64).T


def inv_norm(nn) -> float:
    """r: 1 / sqrt(nn) in double, both operations correctly rounded; 0 where nn == 0"""
    return 1.0 / math.sqrt(float(nn)) if nn > 0 else 0.0


def scores(dot_row, r_query, r):
    """((double)dot * r_query) * r_j: two products, each rounded on its own"""
    return (np.asarray(dot_row, np.int64).astype(np.float64) * np.float64(r_query)) * np.asarray(r, np.float64)


def query_row(dot_row, r_query, r, query_id, k, min_score=0.0, exclude_recent=0):
    """(candidates int32 [k], scores float64 [k], count) of one query over the whole index; query_id None: a frame, no exclusion"""
    s = scores(dot_row, r_query, r)
    j = np.arange(len(s))
    ok = s >= min_score
    if query_id is not None:
        ok &= np.abs(j - query_id) > exclude_recent
    j, s = j[ok], s[ok]
    order = np.lexsort((j, -s))[:k]  # descending score, then ascending id
    cand, score = np.full(k, -1, np.int32), np.full(k, np.nan, np.float64)
    cand[:len(order)], score[:len(order)] = j[order], s[order]
    return cand, score, len(order)


def query(X, norms, query_ids, k, min_score=0.0, exclude_recent=0):
    """dvo_amd_place_query restated: rows X with their norms, the queries are rows of the index"""
    r = np.array([inv_norm(n) for n in norms], np.float64)
    D = dots(X[list(query_ids)], X) if len(query_ids) else np.zeros((0, len(X)), np.int64)
    got = [query_row(D[i], r[q], r, int(q), k, min_score, exclude_recent) for i, q in enumerate(query_ids)]
    return _stack(got, k)


def query_frames(X, norms, Q, q_norms, k, min_score=0.0):
    """dvo_amd_place_query_frames restated: the queries are descriptors that are not in the index"""
    r = np.array([inv_norm(n) for n in norms], np.float64)
    D = dots(Q, X) if len(X) else np.zeros((len(Q), 0), np.int64)
    got = [query_row(D[i], inv_norm(q_norms[i]), r, None, k, min_score) for i in range(len(Q))]
    return _stack(got, k)


def _stack(got, k):
    if not got:
        return np.zeros((0, k), np.int32), np.zeros((0, k), np.float64), np.zeros(0, np.int32)
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got]), np.array([g[2] for g in got], np.int32)


TIE_D = (0.5, -0.5, 1.5, -1.5, 2.5, 126.5, 127.5, 200.0, -200.0)
TIE_Q = (0, 0, 2, -2, 2, 126, 127, 127, -127)  # ties to even, then the clamp
TIE_NON_FINITE = (np.nan, np.inf, -np.inf)


def tie_plane(non_finite=True):
    """(plane 3 x 48, [(pixel index, d, q)]): a plane whose arithmetic is exact (gain 1).  It is a row of 3 x 3 patches; patch i has
    the centre a = 1 + d and eight neighbours b = 1 - d / 8, so its sum is exactly 9, m = 1 and the centre's d = a - 1 -- binary
    fractions that fit 24 bits with room, partial sums included.  A centre's neighbourhood is its own patch.  With non_finite
    three more patches have the centre NaN, +Inf and -Inf: the centre's d is NaN, and its eight neighbours' d is NaN, -Inf and
    +Inf -- all of them must quantise to 0.  The width is a multiple of 4, as a pyramid's must be."""
    centres = list(TIE_D) + (list(TIE_NON_FINITE) if non_finite else [])
    I = np.ones((3, 48), F)
    expect = []
    for i, d in enumerate(centres):
        u = 3 * i + 1
        if np.isfinite(d):
            I[:, u - 1:u + 2] = F(1.0 - d / 8.0)
            I[1, u] = F(1.0 + d)
            expect.append((48 + u, d, TIE_Q[i]))
        else:
            I[1, u] = F(d)
            expect += [(v * 48 + x, None, 0) for v in range(3) for x in range(u - 1, u + 2)]
    return I, expect
