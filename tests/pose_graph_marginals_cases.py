"""Helpers of test_pose_graph_marginals.py: the graphs, the float64 reference Sigma = inv(H) on the restatement's own H (never the
library's), the block-relative distance of test_pose_graph._block_rel in vectorised form, and the restated H assembled
block-sparse for graphs whose dense H would not fit."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_restatement as R  # noqa: E402
import slam_graph  # noqa: E402

BAR = 1e-9          # the bar test_gpu_first_system_and_one_step_match_restatement sets for one undamped solve
CONDITION = 1e-11   # the reference must agree with itself to this on every graph used
DELTA = 5.0


def ring(m):
    """m free vertices, the graphs of test_pose_graph.test_gpu_full_optimization_matches_restatement"""
    return R.ring_graph(m + 1, n_chords=max(4, m // 30), star=8, seed=100 + m, drift=0.02)[0]


def slam1200():
    return slam_graph.slam_graph(1200, seed=1200)[0]


def slam3000():
    return slam_graph.slam_graph(3000, seed=3000, noise=1e-3, drift=0.01)[0]


def block_rel(A, B):
    """test_pose_graph._block_rel: max over 6x6 blocks of max|A - B| / max|B| (0 / 0 = 0, nonzero / 0 = inf).  A, B: matrices
    whose sides are multiples of 6, or stacks (k, 6, 6) of blocks."""
    A, B = np.asarray(A), np.asarray(B)
    if A.ndim == 2:
        r, c = A.shape[0] // 6, A.shape[1] // 6
        A = A.reshape(r, 6, c, 6).transpose(0, 2, 1, 3).reshape(-1, 6, 6)
        B = B.reshape(r, 6, c, 6).transpose(0, 2, 1, 3).reshape(-1, 6, 6)
    if len(A) == 0:
        return 0.0
    diff = np.abs(A - B)
    diff = np.where(np.isnan(diff), np.inf, diff)  # a NaN where a number is expected is infinitely far
    d, s = diff.max(axis=(1, 2)), np.abs(B).max(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, np.where(s > 0, d / s, np.inf))
    return float(q.max())


GRAPHS = {"ring30": lambda: ring(30), "ring200": lambda: ring(200), "ring573": lambda: ring(573), "slam1200": slam1200}


@functools.lru_cache(maxsize=3)
def dense_reference(name):
    """(graph, H, Z = np.linalg.inv(H)) of GRAPHS[name], H the restatement's (cached)"""
    g = GRAPHS[name]()
    H = R.linearise(g, DELTA)[0]
    return g, H, np.linalg.inv(H)


def self_distance(H, Z):
    """the condition on the inputs: distance between np.linalg.inv(H) and the Cholesky inverse"""
    import scipy.linalg

    Zc = scipy.linalg.cho_solve(scipy.linalg.cho_factor(H), np.eye(H.shape[0]))
    return block_rel(Zc, Z)


def sparse_H(g, delta=DELTA, poses=None):
    """the restatement's H as scipy CSC, from its own per-edge terms (R.jacobians, R.robust through R.edge_terms) summed the way
    R.linearise sums them"""
    import scipy.sparse

    poses = g.poses if poses is None else poses
    _, _, rho1 = R.edge_terms(poses, g.edges, delta)
    rows, cols, vals = [], [], []
    ii, jj = np.meshgrid(np.arange(6), np.arange(6), indexing="ij")
    for k, (f, t, Z, O) in enumerate(g.edges):
        Jf, Jt = R.jacobians(poses[f], poses[t], Z)
        W = rho1[k] * O
        blocks = [(g.slot.get(f), Jf), (g.slot.get(t), Jt)]
        for si, Ji in blocks:
            for sj, Jj in blocks:
                if si is None or sj is None:
                    continue
                rows.append((6 * si + ii).ravel())
                cols.append((6 * sj + jj).ravel())
                vals.append((Ji.T @ W @ Jj).ravel())
    n = 6 * len(g.free)
    return scipy.sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsc()


def block_columns(Hs, slots, permc_spec="COLAMD"):
    """Z[:, 6s:6s+6] for the slots, by scipy.sparse.linalg.splu: (n, 6 len(slots))"""
    import scipy.sparse.linalg

    lu = scipy.sparse.linalg.splu(Hs, permc_spec=permc_spec)
    n = Hs.shape[0]
    rhs = np.zeros((n, 6 * len(slots)))
    for i, s in enumerate(slots):
        rhs[6 * s:6 * s + 6, 6 * i:6 * i + 6] = np.eye(6)
    return lu.solve(rhs)


def requests(g, n_random=50, seed=0):
    """all diagonal blocks, both orders of every edge pair, n_random seeded pairs of vertices"""
    nv = len(g.poses)
    pairs = [(v, v) for v in range(nv)]
    for f, t, _, _ in g.edges:
        pairs += [(f, t), (t, f)]
    rng = np.random.default_rng(seed)
    pairs += [tuple(int(x) for x in rng.integers(0, nv, size=2)) for _ in range(n_random)]
    return pairs


def expected(g, Z, pairs):
    """the reference blocks of the pairs from a dense Z over the free slots: zeros where a fixed vertex is touched"""
    out = np.zeros((len(pairs), 6, 6))
    for k, (a, b) in enumerate(pairs):
        if g.fixed[a] or g.fixed[b]:
            continue
        sa, sb = g.slot.get(a), g.slot.get(b)
        out[k] = np.nan if sa is None or sb is None else Z[6 * sa:6 * sa + 6, 6 * sb:6 * sb + 6]
    return out
