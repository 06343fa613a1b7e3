"""Helpers of test_pose_graph_solver_edges.py: the graphs that put the pose-graph linear solvers at their tile and front-tier
edges, the residual measures a solve is held to, their float64 Cholesky yardstick, and a numpy restatement of the tiled
factorization that can lose one product term.

The measures take a system (H, b) and a solution x, whoever computed them, and form r = b - H x in np.longdouble (64-bit
mantissa: the residual of a float64 solve is resolved to a per cent of itself or better at these sizes):
    eta   = |r|_inf / (|H|_inf |x|_inf + |b|_inf)          norm-wise backward error
    omega = max_i |r_i| / ((|H| |x|)_i + |b_i|)            component-wise backward error
The yardstick is scipy's float64 cho_factor / cho_solve on the same H and b, scored by the same measures; the solver under test
may be FACTOR times worse, the yardstick's eta floored at one ulp.  FACTOR = 8: two correct float64 Cholesky solves that sum in
different orders (64-wide tiles, MFMA k-blocks of 4, fused multiply-adds against LAPACK's blocking) differ by a small factor
that grows like sqrt(n) at worst; one lost product term is nine orders away (test_seeded_defect_fails_the_bars)."""
import functools
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_restatement as R  # noqa: E402

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the residuals need an extended-precision long double (x86)"
ULP = 2.2e-16
FACTOR = 8.0
DELTA = 5.0
TILE = 64            # kTile of dvo_graph.cpp
WIDE_PIVOTS = 192    # kWidePivots: 6 p above this takes the tiled path
SMALL_MAX_LD = 1024  # kSmallMaxLd: 6 (p + u) above this takes the tiled path


def _exp(xi):
    from dvo_slam_amd import synth

    return synth.se3_exp(xi)


# ---- graphs -------------------------------------------------------------------------------------------------------------------
def _graph_of_pairs(n_vertices, pairs, seed):
    """vertex 0 fixed; the truth on a ring; every pair an edge that measures the true relative pose with R.information;
    the estimate = the truth times a 0.02 perturbation"""
    rng = np.random.default_rng(seed)
    truth = R.ring_truth(n_vertices, seed=seed)
    edges = [(f, t, R.inverse(truth[f]) @ truth[t], R.information(rng)) for f, t in pairs]
    poses = [truth[0].copy()] + [T @ _exp(rng.normal(scale=0.02, size=6)) for T in truth[1:]]
    return R.Graph(poses, [True] + [False] * (n_vertices - 1), edges)


@functools.lru_cache(maxsize=None)
def complete_graph(m, seed=None):
    """one fixed vertex, m free ones, an edge between every pair: every 6 x 6 block of H is nonzero"""
    return _graph_of_pairs(m + 1, list(itertools.combinations(range(m + 1), 2)), 1000 + m if seed is None else seed)


def clique_pairs(k, pendants):
    """(n_vertices, pairs): vertex 0 (fixed) joined to vertex 1; a clique of the k vertices 1..k; behind it one group of
    vertices per entry of `pendants`, each a clique of its own whose every vertex is joined to every vertex of the big clique.
    Nested dissection makes the big clique the root front (k, 0) and each group (two or more of them) a child (size, k)."""
    clique = list(range(1, k + 1))
    pairs = [(0, 1)] + list(itertools.combinations(clique, 2))
    v = k + 1
    for size in pendants:
        group = list(range(v, v + size))
        v += size
        pairs += list(itertools.combinations(group, 2)) + [(c, q) for q in group for c in clique]
    return v, pairs


# name -> (k, pendants, the (pivots, updates) every front must have, children first)
FRONT_GRAPHS = {
    # (1, 169): the largest small front, ld 1020; (2, 169): 6 p = 12 but ld 1026, wide by ld only, under the wide root
    # (169, 0) whose 6 p = 1014 pads to 1024
    "ld1020-ld1026-under-p169": (169, (1, 2), [(1, 169), (2, 169), (169, 0)]),
    "root-p32": (32, (2, 2), [(2, 32), (2, 32), (32, 0)]),   # 6 p = 192: the widest small root
    "root-p33": (33, (2, 2), [(2, 33), (2, 33), (33, 0)]),   # 6 p = 198: wide, pivots padded to 256
    "root-p64": (64, (2, 2), [(2, 64), (2, 64), (64, 0)]),   # 6 p = 384: wide, six pivot tiles and no pad pivot
}


@functools.lru_cache(maxsize=None)
def front_graph(name):
    k, pendants, _ = FRONT_GRAPHS[name]
    nv, pairs = clique_pairs(k, pendants)
    return _graph_of_pairs(nv, pairs, 2000 + k)


def symbolic_of(g):
    from dvo_slam_amd import graph

    return graph.symbolic(len(g.poses), [(f, t) for f, t, _, _ in g.edges], g.fixed)


def front_layout(p, u):
    """(wide, ppad, ld) of a front with p pivot and u update vertices, as dvo_graph.cpp lays it out"""
    wide = 6 * p > WIDE_PIVOTS or 6 * (p + u) > SMALL_MAX_LD
    if not wide:
        return False, 6 * p, 6 * (p + u)
    ppad = -(-6 * p // TILE) * TILE
    return True, ppad, -(-(ppad + 6 * u) // TILE) * TILE


def census(g):
    """[(pivots, updates, parent)] of g's fronts in elimination order"""
    S = symbolic_of(g)
    return [(len(p), len(u), int(q)) for p, u, q in zip(S["pivots"], S["updates"], S["parent"])]


def non_pd_graph(m, s, neighbour_slots=None):
    """complete_graph(m) with every edge of the free vertex in slot s replaced by edges that carry no information on rotation
    and end in it (the `to` end: its rotation columns of J are then multiplied by the zero rows of the information alone), one
    from the vertex of each slot in `neighbour_slots` (None: one single edge, from slot 0, or from slot 1 when s = 0).  Rows
    6 s + 3 .. 6 s + 5 of H are exactly zero, stay exactly zero under elimination, and every other pivot is positive (the rest
    of H is positive definite): the first failed pivot is s's fourth."""
    g = complete_graph(m)
    v = g.free[s]
    if neighbour_slots is None:
        neighbour_slots = [1 if s == 0 else 0]
    edges = [e for e in g.edges if v not in e[:2]]
    for q in neighbour_slots:
        w = g.free[q]
        edges.append((w, v, R.inverse(g.poses[w]) @ g.poses[v] @ _exp([0.01, 0.0, 0.02, 0.0, 0.0, 0.0]),
                      np.diag([400.0, 400.0, 400.0, 0.0, 0.0, 0.0])))
    return R.Graph(g.poses, g.fixed, edges)


def ring_with_chords(m, seed=4096):
    """m free vertices: the cap graph (a ring with chords and keyframe stars, as test_pose_graph.py's)"""
    return R.ring_graph(m + 1, n_chords=40, star=8, seed=seed, noise=1e-3, drift=0.01)[0]


# ---- the measures -------------------------------------------------------------------------------------------------------------
def measures(H, b, x):
    """(eta, omega) of x as a solution of H x = b; H dense.  x and b may be matrices (one system per column): arrays come back"""
    Hl, bl, xl = np.asarray(H, dtype=LD), np.asarray(b, dtype=LD), np.asarray(x, dtype=LD)
    r = np.abs(bl - Hl @ xl)
    aHx = np.abs(Hl) @ np.abs(xl)
    Hn = np.abs(Hl).sum(axis=1).max()
    eta = r.max(axis=0) / (Hn * np.abs(xl).max(axis=0) + np.abs(bl).max(axis=0))
    omega = (r / (aHx + np.abs(bl))).max(axis=0)
    return (float(eta), float(omega)) if xl.ndim == 1 else (eta.astype(np.float64), omega.astype(np.float64))


def measures_blocks(rc, blocks, b, x):
    """measures() with H given as its stored 6 x 6 blocks (block_rc, blocks of debug_system_sparse): nothing n x n is formed"""
    n = len(b)
    xl, bl = np.asarray(x, dtype=LD), np.asarray(b, dtype=LD)
    Bl = np.asarray(blocks, dtype=LD)
    rows, cols = np.asarray(rc)[:, 0], np.asarray(rc)[:, 1]
    xb = xl.reshape(-1, 6)[cols]                                  # (k, 6): the x block each stored block meets
    Hx, aHx, rowsum = np.zeros((n // 6, 6), LD), np.zeros((n // 6, 6), LD), np.zeros((n // 6, 6), LD)
    np.add.at(Hx, rows, np.einsum("kij,kj->ki", Bl, xb))
    np.add.at(aHx, rows, np.einsum("kij,kj->ki", np.abs(Bl), np.abs(xb)))
    np.add.at(rowsum, rows, np.abs(Bl).sum(axis=2))
    r = np.abs(bl - Hx.reshape(-1))
    eta = r.max() / (rowsum.max() * np.abs(xl).max() + np.abs(bl).max())
    omega = (r / (aHx.reshape(-1) + np.abs(bl))).max()
    return float(eta), float(omega)


def cholesky_reference(H, b):
    """the yardstick's solution: scipy's float64 Cholesky on the very H and b the solver under test had"""
    import scipy.linalg

    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(H, lower=True), b)


def within_bars(got, ref):
    """got, ref: (eta, omega) of the solver under test and of the yardstick on one system"""
    return bool(got[0] <= FACTOR * max(ref[0], ULP) and got[1] <= FACTOR * ref[1])


def ratios(got, ref):
    """(eta / floored yardstick eta, omega / yardstick omega): what DESIGN.md records; the bars say both <= FACTOR"""
    return got[0] / max(ref[0], ULP), got[1] / ref[1]


def inverse_measure(H, Zc, columns=None):
    """per column of Zc, Zc[:, i] ~ inv(H)[:, columns[i]] (None: the whole inverse): |e_c - H z_c|_inf / (|H|_inf |z_c|_inf + 1),
    the residual in long double"""
    Hl, Zl = np.asarray(H, dtype=LD), np.asarray(Zc, dtype=LD)
    columns = np.arange(Zl.shape[1]) if columns is None else columns
    E = np.zeros(Zl.shape, LD)
    E[np.asarray(columns), np.arange(len(columns))] = 1
    r = np.abs(E - Hl @ Zl)
    Hn = np.abs(Hl).sum(axis=1).max()
    return (r.max(axis=0) / (Hn * np.abs(Zl).max(axis=0) + 1)).astype(np.float64)


def cholesky_inverse(H):
    import scipy.linalg

    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(H, lower=True), np.eye(H.shape[0]))


# ---- the tiled factorization restated, with a seedable defect ----------------------------------------------------------------
def tiled_cholesky_solve(H, b, drop=None):
    """H x = b the way the dense path does it: H padded with the identity to a multiple of TILE, then per tile column k the
    diagonal tile's Cholesky (k_potrf_panel), the tiles below it solved against it (k_trsm), and the trailing update
    A_ij -= A_ik A_jk^T of every tile j <= i behind it (k_syrk); two triangular solves (k_trsv).
    drop = (k, i, j, row, term): in that one trailing update, the entries of row `row` of tile (i, j) lose the product term
    `term` of their 64: the seeded defect."""
    import scipy.linalg

    n = H.shape[0]
    N = max(TILE, -(-n // TILE) * TILE)
    A = np.eye(N)
    A[:n, :n] = H
    T = N // TILE
    sl = lambda t: slice(t * TILE, (t + 1) * TILE)  # noqa: E731
    for k in range(T):
        A[sl(k), sl(k)] = np.linalg.cholesky(A[sl(k), sl(k)])
        for i in range(k + 1, T):
            A[sl(i), sl(k)] = scipy.linalg.solve_triangular(A[sl(k), sl(k)], A[sl(i), sl(k)].T, lower=True).T
        for i in range(k + 1, T):
            for j in range(k + 1, i + 1):
                U = A[sl(i), sl(k)] @ A[sl(j), sl(k)].T
                if drop is not None and drop[:3] == (k, i, j):
                    _, _, _, row, term = drop
                    U[row, :] -= A[i * TILE + row, k * TILE + term] * A[sl(j), k * TILE + term]
                A[sl(i), sl(j)] -= U
    L = np.tril(A)
    rhs = np.zeros(N)
    rhs[:n] = b
    y = scipy.linalg.solve_triangular(L, rhs, lower=True)
    return scipy.linalg.solve_triangular(L.T, y, lower=False)[:n]
