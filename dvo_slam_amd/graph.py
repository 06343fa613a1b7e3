"""Pose-graph optimization over the C ABI (dvo_amd_optimize_graph): the keyframe graph's g2o::SparseOptimizer with VertexSE3 /
EdgeSE3, Levenberg-Marquardt (LocalMap::optimize) or dogleg (KeyframeGraph), with RobustKernelCauchy.  The semantics are pinned
in include/dvo_amd.h.  Poses are row-major 4x4 numpy arrays, as everywhere in this binding.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi

LEVENBERG, DOGLEG = 0, 1
ALGORITHMS = {"levenberg": LEVENBERG, "dogleg": DOGLEG}
DENSE, SPARSE = 0, 1
SOLVERS = {"dense": DENSE, "sparse": SPARSE}
TERMINATION = {0: "iterations exhausted", 1: "terminate", 2: "fail"}
MAX_FREE_VERTICES = 1024
MAX_FREE_VERTICES_SPARSE = 65536
BATCH_MAX_FREE_VERTICES = 32
ROTATION_VECTOR_SCALE = np.array([1.0, 1.0, 1.0, 2.0, 2.0, 2.0])  # S: quaternion-vector units -> rotation-vector units


class CGraphEdge(C.Structure):
    _fields_ = [("from_", C.c_int), ("to", C.c_int), ("measurement", C.c_double * 16), ("information", C.c_double * 36)]


class CGraphOptions(C.Structure):
    _fields_ = [("algorithm", C.c_int), ("max_iterations", C.c_int), ("max_trials", C.c_int), ("solver", C.c_int),
                ("robust_delta", C.c_double), ("initial_lambda", C.c_double), ("initial_delta", C.c_double)]


class CGraphIteration(C.Structure):
    _fields_ = [("objective", C.c_double), ("step_norm", C.c_double), ("lambda_", C.c_double), ("delta", C.c_double),
                ("trials", C.c_int), ("accepted", C.c_int)]


class CGraphStats(C.Structure):
    _fields_ = [("iterations", C.c_int), ("termination", C.c_int), ("n_free", C.c_int), ("cholesky_failures", C.c_int),
                ("initial_objective", C.c_double), ("final_objective", C.c_double), ("lambda_", C.c_double),
                ("delta", C.c_double)]


class CGraphMarginalStats(C.Structure):
    _fields_ = [("n_free", C.c_int), ("factorized", C.c_int), ("fixed_blocks", C.c_int), ("inactive_blocks", C.c_int),
                ("solved_columns", C.c_int), ("reserved", C.c_int)]


class CGraphBatchItem(C.Structure):
    _fields_ = [("n_vertices", C.c_int), ("poses", C.POINTER(C.c_double)), ("fixed", C.POINTER(C.c_int)),
                ("n_edges", C.c_int), ("edges", C.POINTER(CGraphEdge)), ("edge_chi2", C.POINTER(C.c_double)),
                ("edge_weight", C.POINTER(C.c_double)), ("stats", CGraphStats)]


_bound = False


def _lib():
    global _bound
    L = capi.lib()
    if not _bound:
        dp = C.POINTER(C.c_double)
        L.dvo_amd_default_graph_options.restype = None
        L.dvo_amd_default_graph_options.argtypes = [C.c_int, C.POINTER(CGraphOptions)]
        L.dvo_amd_optimize_graph.argtypes = [C.c_void_p, C.c_int, dp, C.POINTER(C.c_int), C.c_int, C.POINTER(CGraphEdge),
                                             C.POINTER(CGraphOptions), dp, dp, C.c_int, C.POINTER(CGraphIteration),
                                             C.POINTER(CGraphStats)]
        L.dvo_amd_graph_marginals.argtypes = [C.c_void_p, C.c_int, dp, C.POINTER(C.c_int), C.c_int, C.POINTER(CGraphEdge),
                                              C.POINTER(CGraphOptions), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), dp,
                                              C.POINTER(CGraphMarginalStats)]
        L.dvo_amd_debug_graph_timing.argtypes = [C.c_void_p, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dvo_amd_debug_graph_system.argtypes = [C.c_void_p, C.c_int, dp, C.POINTER(C.c_int), C.c_int, C.POINTER(CGraphEdge),
                                                 C.c_double, dp, dp, dp, dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        ip = C.POINTER(C.c_int)
        L.dvo_amd_debug_graph_system_sparse.argtypes = [C.c_void_p, C.c_int, dp, ip, C.c_int, C.POINTER(CGraphEdge), C.c_double,
                                                        C.c_int, ip, ip, dp, dp, dp, dp, ip, ip]
        L.dvo_amd_debug_graph_symbolic.argtypes = [C.c_int, ip, C.c_int, C.POINTER(CGraphEdge), C.c_int, ip, ip, ip, ip, ip,
                                                   ip, ip, ip, ip, ip, ip, ip, dp, dp]
        L.dvo_amd_debug_graph_sparse_timing.argtypes = [C.c_void_p, dp, dp, dp, dp, ip, ip, ip, dp, dp]
        L.dvo_amd_optimize_graphs_batch.argtypes = [C.c_void_p, C.c_int, C.POINTER(CGraphBatchItem), C.POINTER(CGraphOptions)]
        L.dvo_amd_debug_graph_batch_records.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(CGraphIteration), ip]
        _bound = True
    return L


def default_options(algorithm: str = "dogleg") -> CGraphOptions:
    o = CGraphOptions()
    _lib().dvo_amd_default_graph_options(ALGORITHMS[algorithm], C.byref(o))
    return o


class Result:
    """What optimize() returns: poses (list of 4x4), per-edge chi2 and weight (rho1), per-iteration records and the stats."""

    def __init__(self, poses, chi2, weight, iterations, stats: CGraphStats):
        self.poses = poses
        self.chi2 = chi2
        self.weight = weight
        self.iterations = iterations   # dict of arrays: objective, step_norm, lambda, delta, trials, accepted
        self.n_iterations = stats.iterations
        self.termination = TERMINATION.get(stats.termination, str(stats.termination))
        self.n_free = stats.n_free
        self.cholesky_failures = stats.cholesky_failures
        self.initial_objective = stats.initial_objective
        self.final_objective = stats.final_objective
        self.lambda_ = stats.lambda_
        self.delta = stats.delta


class PoseGraph:
    """g2o::SparseOptimizer with VertexSE3 / EdgeSE3: add_vertex, add_edge, optimize.  Edge ids are their order of insertion;
    removed edges keep their id (None in `edges`) and are left out of the next optimize()."""

    def __init__(self):
        self.poses = []
        self.fixed = []
        self.edges = []     # (from, to, Z 4x4, information 6x6) or None once removed
        self.last = None    # the last Result

    def add_vertex(self, pose=None, fixed: bool = False) -> int:
        self.poses.append(np.array(np.eye(4) if pose is None else pose, dtype=np.float64).reshape(4, 4))
        self.fixed.append(bool(fixed))
        return len(self.poses) - 1

    def set_fixed(self, vertex: int, fixed: bool = True):
        self.fixed[vertex] = bool(fixed)

    def add_edge(self, from_: int, to: int, measurement, information) -> int:
        Z = np.array(measurement, dtype=np.float64).reshape(4, 4)
        O = np.array(information, dtype=np.float64).reshape(6, 6)
        self.edges.append((int(from_), int(to), Z, O))
        return len(self.edges) - 1

    def live_edges(self):
        return [k for k, e in enumerate(self.edges) if e is not None]

    def add_constraints(self, proposals, vertex_of) -> list:
        """Add the surviving proposals of constraints.ConstraintProposalValidator.validate() as edges, the way
        KeyframeGraph::insertConstraint does (keyframe_graph.cpp:619-633): vertex 0 = the proposal's Reference keyframe, vertex 1
        = its Current one, measurement p.TrackingResult.Transformation, information p.TrackingResult.Information.
        vertex_of: keyframe -> vertex id (a dict keyed by keyframe id, or a callable).  Returns the new edge ids."""
        look = vertex_of if callable(vertex_of) else (lambda kf: vertex_of[kf.id])
        ids = []
        for p in proposals:
            r = p.TrackingResult
            ids.append(self.add_edge(look(p.Reference), look(p.Current), r.Transformation, r.Information))
        return ids

    def optimize(self, tracker: "capi.DenseTracker", algorithm: str = "dogleg", iterations: int | None = None,
                 robust_delta: float = 5.0, max_trials: int | None = None, initial_lambda: float | None = None,
                 initial_delta: float | None = None, update: bool = True, solver: str = "dense") -> Result:
        """Optimize in the tracker's context (dvo_amd_optimize_graph).  Defaults are the reference's (dvo_amd.h); update=True
        writes the optimized poses back into the graph.  solver: "dense" (at most MAX_FREE_VERTICES free vertices) or "sparse"
        (the multifrontal sparse Cholesky, at most MAX_FREE_VERTICES_SPARSE)."""
        L = _lib()
        o = default_options(algorithm)
        o.solver = SOLVERS[solver]
        if iterations is not None:
            o.max_iterations = int(iterations)
        if max_trials is not None:
            o.max_trials = int(max_trials)
        if initial_lambda is not None:
            o.initial_lambda = float(initial_lambda)
        if initial_delta is not None:
            o.initial_delta = float(initial_delta)
        o.robust_delta = float(robust_delta)
        live, nv, ne, P, fixed, ce = self._pack()
        chi2 = np.zeros(max(ne, 1))
        weight = np.zeros(max(ne, 1))
        cap = max(o.max_iterations, 1)
        its = (CGraphIteration * cap)()
        st = CGraphStats()
        dp = C.POINTER(C.c_double)
        rc = L.dvo_amd_optimize_graph(tracker._h, nv, P.ctypes.data_as(dp), fixed.ctypes.data_as(C.POINTER(C.c_int)), ne, ce,
                                      C.byref(o), chi2.ctypes.data_as(dp), weight.ctypes.data_as(dp), cap, its, C.byref(st))
        capi._check(rc, "dvo_amd_optimize_graph")
        poses = [P[v].T.copy() for v in range(nv)]
        n_it = min(st.iterations, cap)
        rec = {"objective": np.array([its[i].objective for i in range(n_it)]),
               "step_norm": np.array([its[i].step_norm for i in range(n_it)]),
               "lambda": np.array([its[i].lambda_ for i in range(n_it)]),
               "delta": np.array([its[i].delta for i in range(n_it)]),
               "trials": np.array([its[i].trials for i in range(n_it)], dtype=np.int64),
               "accepted": np.array([its[i].accepted for i in range(n_it)], dtype=np.int64)}
        w_full = np.full(len(self.edges), np.nan)
        c_full = np.full(len(self.edges), np.nan)
        w_full[live] = weight[:ne]
        c_full[live] = chi2[:ne]
        res = Result(poses, c_full, w_full, rec, st)
        res.robust_delta = o.robust_delta
        if update:
            self.poses = [T.copy() for T in poses]
        self.last = res
        return res

    def marginals(self, tracker: "capi.DenseTracker", pairs=None, solver: str = "dense", robust_delta: float = 5.0,
                  rotation: str = "quaternion"):
        """Blocks of Sigma = H^-1 at the current poses (dvo_amd_graph_marginals; the semantics are pinned in dvo_amd.h):
        (blocks (k, 6, 6) float64 row-major, stats).  pairs: (a, b) vertex pairs, block k = rows of a, columns of b; None means
        every vertex's diagonal block, in vertex order.  A block that touches a fixed vertex is zeros, one that touches an
        inactive vertex NaN; when stats.factorized == 0 every other block is NaN.  rotation="quaternion": the increment's own
        coordinates (tx, ty, tz, qx, qy, qz); "vector": S Sigma S with S = diag(1, 1, 1, 2, 2, 2), rotation-vector units
        (radians).  With solver="sparse" pairs that share no edge take the slow path (stats.solved_columns)."""
        if rotation not in ("quaternion", "vector"):
            raise ValueError("rotation must be 'quaternion' or 'vector'")
        L = _lib()
        o = default_options("dogleg")
        o.solver = SOLVERS[solver]
        o.robust_delta = float(robust_delta)
        live, nv, ne, P, fixed, ce = self._pack()
        if pairs is None:
            pairs = [(v, v) for v in range(nv)]
        pr = np.asarray(list(pairs), dtype=np.int32).reshape(-1, 2)
        k = len(pr)
        a, b = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        out = np.zeros((max(k, 1), 36))
        st = CGraphMarginalStats()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        rc = L.dvo_amd_graph_marginals(tracker._h, nv, P.ctypes.data_as(dp), fixed.ctypes.data_as(ip), ne, ce, C.byref(o), k,
                                       a.ctypes.data_as(ip) if k else None, b.ctypes.data_as(ip) if k else None,
                                       out.ctypes.data_as(dp) if k else None, C.byref(st))
        capi._check(rc, "dvo_amd_graph_marginals")
        blocks = np.ascontiguousarray(out[:k].reshape(k, 6, 6).transpose(0, 2, 1))  # column-major -> row-major
        if rotation == "vector":
            blocks = blocks * np.outer(ROTATION_VECTOR_SCALE, ROTATION_VECTOR_SCALE)
        return blocks, st

    def _pack(self):
        live = self.live_edges()
        nv, ne = len(self.poses), len(live)
        P = np.ascontiguousarray(np.stack([T.T for T in self.poses]) if nv else np.zeros((1, 4, 4)))
        fixed = np.ascontiguousarray(np.asarray(self.fixed, dtype=np.int32)) if nv else np.zeros(1, np.int32)
        ce = (CGraphEdge * max(ne, 1))()
        for i, k in enumerate(live):
            f, t, Z, O = self.edges[k]
            ce[i].from_, ce[i].to = f, t
            ce[i].measurement[:] = list(Z.T.reshape(-1))
            ce[i].information[:] = list(O.T.reshape(-1))
        return live, nv, ne, P, fixed, ce

    def debug_system(self, tracker: "capi.DenseTracker", robust_delta: float = 5.0, with_H: bool = True):
        """(diagnostic) the first linear system of optimize() on the current poses (dvo_amd_debug_graph_system):
        (H n x n, b, x of the undamped solve or None when a pivot failed, F, index of the failed pivot or -1).  with_H=False
        passes NULL for H (the entry's outputs are optional) and returns None in its place: at the dense cap H is 302 MB."""
        L = _lib()
        live, nv, ne, P, fixed, ce = self._pack()
        active = {v for k in live for v in self.edges[k][:2]}
        n = 6 * sum(1 for v in range(nv) if v in active and not self.fixed[v])
        H = np.zeros((max(n, 1), max(n, 1))) if with_H else None
        b, x = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        F, nf, fp = C.c_double(), C.c_int(), C.c_int()
        dp = C.POINTER(C.c_double)
        capi._check(L.dvo_amd_debug_graph_system(tracker._h, nv, P.ctypes.data_as(dp), fixed.ctypes.data_as(C.POINTER(C.c_int)),
                                                 ne, ce, float(robust_delta), H.ctypes.data_as(dp) if with_H else None,
                                                 b.ctypes.data_as(dp), x.ctypes.data_as(dp), C.byref(F), C.byref(nf),
                                                 C.byref(fp)),
                    "dvo_amd_debug_graph_system")
        assert 6 * nf.value == n
        return (H[:n, :n] if with_H else None), b[:n], (x[:n] if fp.value < 0 else None), F.value, fp.value

    def debug_system_sparse(self, tracker: "capi.DenseTracker", robust_delta: float = 5.0):
        """(diagnostic) the first linear system of optimize(solver="sparse") (dvo_amd_debug_graph_system_sparse):
        (block (row, col) slots k x 2, blocks k x 6 x 6, b, x of the undamped sparse solve or None when a pivot failed, F,
        the failed pivot or -1)"""
        L = _lib()
        live, nv, ne, P, fixed, ce = self._pack()
        active = {v for k in live for v in self.edges[k][:2]}
        m = sum(1 for v in range(nv) if v in active and not self.fixed[v])
        cap = m + 2 * ne
        rc, blocks = np.zeros((max(cap, 1), 2), np.int32), np.zeros((max(cap, 1), 6, 6))
        b, x = np.zeros(max(6 * m, 1)), np.zeros(max(6 * m, 1))
        F, nf, fp, nb = C.c_double(), C.c_int(), C.c_int(), C.c_int()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        capi._check(L.dvo_amd_debug_graph_system_sparse(tracker._h, nv, P.ctypes.data_as(dp), fixed.ctypes.data_as(ip), ne, ce,
                                                        float(robust_delta), cap, C.byref(nb), rc.ctypes.data_as(ip),
                                                        blocks.ctypes.data_as(dp), b.ctypes.data_as(dp), x.ctypes.data_as(dp),
                                                        C.byref(F), C.byref(nf), C.byref(fp)),
                    "dvo_amd_debug_graph_system_sparse")
        assert nf.value == m
        k, n = nb.value, 6 * m
        return rc[:k].copy(), blocks[:k].copy(), b[:n], (x[:n] if fp.value < 0 else None), F.value, fp.value

    def debug_symbolic(self):
        """(diagnostic) the sparse solver's symbolic phase on this graph's structure; see symbolic()"""
        live = self.live_edges()
        return symbolic(len(self.poses), [self.edges[k][:2] for k in live], self.fixed)

    def remove_outlier_edges(self, weight_threshold: float, n_max: int = -1) -> list:
        """KeyframeGraph::removeOutlierConstraints (keyframe_graph.cpp:643-675) on the weights (rho1) of the last optimize():
        edges with a robust kernel (every edge when that optimize() had robust_delta > 0, none otherwise) whose weight is below the threshold are
        removed lowest weight first, at most n_max of them (n_max < 0: all).  Equal weights go by edge id (the reference keys a
        std::map by the weight and so keeps only one edge per weight value).  Returns the removed edge ids in removal order."""
        if self.last is None:
            raise RuntimeError("remove_outlier_edges needs the weights of an optimize() first")
        if not self.last.robust_delta > 0:
            return []
        w = self.last.weight
        cand = [k for k in self.live_edges() if k < len(w) and np.isfinite(w[k]) and w[k] < weight_threshold]
        cand.sort(key=lambda k: (w[k], k))
        if n_max >= 0:
            cand = cand[:n_max]
        for k in cand:
            self.edges[k] = None
        return cand


def _skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def relative_jacobians(Xa, Xb):
    """(J_a, J_b): dvo_amd.h's J_from and J_to for an edge from a to b with Z = I, i.e. the derivatives of
    e = (t, q_xyz)(Xa^-1 Xb) with respect to the increments of a and b at 0"""
    Xa, Xb = np.asarray(Xa, dtype=np.float64), np.asarray(Xb, dtype=np.float64)
    Ra, ta = Xa[:3, :3], Xa[:3, 3]
    R = Ra.T @ Xb[:3, :3]
    t = Ra.T @ (Xb[:3, 3] - ta)
    # the unit quaternion of R with w >= 0 (the branch of largest magnitude, as Eigen's Quaternion(R))
    tr = np.trace(R)
    if tr > 0:
        s = np.sqrt(tr + 1.0) * 2.0
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0) * 2.0
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q /= np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    w, v = q[0], q[1:]
    Jb, Ja = np.zeros((6, 6)), np.zeros((6, 6))
    Jb[:3, :3] = R
    Jb[3:, 3:] = w * np.eye(3) + _skew(v)
    Ja[:3, :3] = -np.eye(3)
    Ja[:3, 3:] = 2.0 * _skew(t)
    Ja[3:, 3:] = -(w * np.eye(3) - _skew(v))
    return Ja, Jb


def relative_covariance(Xa, Xb, S_aa, S_ab, S_bb) -> np.ndarray:
    """First-order covariance of Delta = Xa^-1 Xb in the edge error's coordinates (t, q_xyz), from the marginal blocks of
    PoseGraph.marginals (rotation="quaternion"): J_a S_aa J_a^T + J_a S_ab J_b^T + J_b S_ab^T J_a^T + J_b S_bb J_b^T.  Host numpy
    only: what a candidate search gated by the uncertainty of the relative pose would call."""
    Ja, Jb = relative_jacobians(Xa, Xb)
    S_aa, S_ab, S_bb = (np.asarray(S, dtype=np.float64).reshape(6, 6) for S in (S_aa, S_ab, S_bb))
    cross = Ja @ S_ab @ Jb.T
    return Ja @ S_aa @ Ja.T + cross + cross.T + Jb @ S_bb @ Jb.T


def _records(its, n):
    return {"objective": np.array([its[i].objective for i in range(n)]),
            "step_norm": np.array([its[i].step_norm for i in range(n)]),
            "lambda": np.array([its[i].lambda_ for i in range(n)]),
            "delta": np.array([its[i].delta for i in range(n)]),
            "trials": np.array([its[i].trials for i in range(n)], dtype=np.int64),
            "accepted": np.array([its[i].accepted for i in range(n)], dtype=np.int64)}


def optimize_batch(tracker: "capi.DenseTracker", graphs, algorithm: str = "levenberg", iterations: int | None = None,
                   robust_delta: float = 5.0, max_trials: int | None = None, initial_lambda: float | None = None,
                   initial_delta: float | None = None, update: bool = True) -> list:
    """Optimize many small, independent PoseGraphs in one call (dvo_amd_optimize_graphs_batch): one workgroup per graph, one
    kernel launch for the whole batch, at most BATCH_MAX_FREE_VERTICES free vertices per graph.  One set of options for all of
    them, with the defaults of PoseGraph.optimize for the algorithm.  Returns one Result per graph, in order (their
    `iterations` is empty: the entry returns no per-iteration records); update=True writes the poses back into the graphs.
    Raises what PoseGraph.optimize raises when the call fails (capi.DvoAmdError with the status)."""
    L = _lib()
    o = default_options(algorithm)
    if iterations is not None:
        o.max_iterations = int(iterations)
    if max_trials is not None:
        o.max_trials = int(max_trials)
    if initial_lambda is not None:
        o.initial_lambda = float(initial_lambda)
    if initial_delta is not None:
        o.initial_delta = float(initial_delta)
    o.robust_delta = float(robust_delta)
    graphs = list(graphs)
    items = (CGraphBatchItem * max(len(graphs), 1))()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    keep = []
    for i, pg in enumerate(graphs):
        live, nv, ne, P, fixed, ce = pg._pack()
        chi2, weight = np.zeros(max(ne, 1)), np.zeros(max(ne, 1))
        keep.append((live, nv, ne, P, fixed, ce, chi2, weight))
        items[i].n_vertices, items[i].n_edges = nv, ne
        items[i].poses, items[i].fixed, items[i].edges = P.ctypes.data_as(dp), fixed.ctypes.data_as(ip), ce
        items[i].edge_chi2, items[i].edge_weight = chi2.ctypes.data_as(dp), weight.ctypes.data_as(dp)
    capi._check(L.dvo_amd_optimize_graphs_batch(tracker._h, len(graphs), items, C.byref(o)), "dvo_amd_optimize_graphs_batch")
    out = []
    for i, pg in enumerate(graphs):
        live, nv, ne, P, fixed, ce, chi2, weight = keep[i]
        poses = [P[v].T.copy() for v in range(nv)]
        w_full, c_full = np.full(len(pg.edges), np.nan), np.full(len(pg.edges), np.nan)
        w_full[live] = weight[:ne]
        c_full[live] = chi2[:ne]
        st = CGraphStats.from_buffer_copy(items[i].stats)
        res = Result(poses, c_full, w_full, _records(None, 0), st)
        res.robust_delta = o.robust_delta
        if update:
            pg.poses = [T.copy() for T in poses]
        pg.last = res
        out.append(res)
    return out


def debug_batch_records(tracker: "capi.DenseTracker", graph: int, capacity: int = 256) -> dict:
    """(diagnostic) the per-iteration records of graph `graph` of the tracker's last optimize_batch(), in the layout of
    Result.iterations (dvo_amd_debug_graph_batch_records)"""
    its = (CGraphIteration * max(capacity, 1))()
    n = C.c_int()
    capi._check(_lib().dvo_amd_debug_graph_batch_records(tracker._h, int(graph), int(capacity), its, C.byref(n)),
                "dvo_amd_debug_graph_batch_records")
    return _records(its, min(n.value, capacity))


def debug_timing(tracker: "capi.DenseTracker"):
    """(diagnostic) the last optimize() on the tracker: (first linearise ms, first factorization ms, padded n, factorizations)"""
    a, b, n, f = C.c_double(), C.c_double(), C.c_int(), C.c_int()
    capi._check(_lib().dvo_amd_debug_graph_timing(tracker._h, C.byref(a), C.byref(b), C.byref(n), C.byref(f)),
                "dvo_amd_debug_graph_timing")
    return a.value, b.value, n.value, f.value


def symbolic(n_vertices: int, pairs, fixed=None) -> dict:
    """(diagnostic, no GPU) the sparse solver's symbolic phase (dvo_amd_debug_graph_symbolic) for n_vertices vertices, the edges'
    (from, to) pairs in edge order and the fixed flags: dict(n_free, perm, parent, level, pivots, updates (lists of slot
    arrays per front, in elimination order), n_levels, widest, factor_doubles, flops)"""
    L = _lib()
    ce = (CGraphEdge * max(len(pairs), 1))()
    for i, (f, t) in enumerate(pairs):
        ce[i].from_, ce[i].to = int(f), int(t)
    fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed, dtype=np.int32))
    ip = C.POINTER(C.c_int)
    counts = [C.c_int() for _ in range(5)]
    fd, fl = C.c_double(), C.c_double()
    cap = max(n_vertices + 1, 16)
    while True:
        arrs = [np.zeros(cap, np.int32) for _ in range(7)]
        rc = L.dvo_amd_debug_graph_symbolic(n_vertices, None if fx is None else fx.ctypes.data_as(ip), len(pairs), ce, cap,
                                            *[C.byref(c) for c in counts], *[a.ctypes.data_as(ip) for a in arrs],
                                            C.byref(fd), C.byref(fl))
        if rc == 7 and counts[0].value <= MAX_FREE_VERTICES_SPARSE:
            cap = max(counts[0].value, counts[1].value + 1, counts[2].value)
            continue
        capi._check(rc, "dvo_amd_debug_graph_symbolic")
        break
    m, nf = counts[0].value, counts[1].value
    perm, parent, level, pptr, piv, uptr, upd = arrs
    return {"n_free": m, "perm": perm[:m].copy(), "parent": parent[:nf].copy(), "level": level[:nf].copy(),
            "pivots": [piv[pptr[k]:pptr[k + 1]].copy() for k in range(nf)],
            "updates": [upd[uptr[k]:uptr[k + 1]].copy() for k in range(nf)],
            "n_levels": counts[3].value, "widest": counts[4].value, "factor_doubles": fd.value, "flops": fl.value}


def debug_sparse_timing(tracker: "capi.DenseTracker") -> dict:
    """(diagnostic) the last sparse optimize() on the tracker (dvo_amd_debug_graph_sparse_timing)"""
    d = [C.c_double() for _ in range(4)]
    i = [C.c_int() for _ in range(3)]
    fd, fl = C.c_double(), C.c_double()
    capi._check(_lib().dvo_amd_debug_graph_sparse_timing(tracker._h, *[C.byref(x) for x in d], *[C.byref(x) for x in i],
                                                         C.byref(fd), C.byref(fl)), "dvo_amd_debug_graph_sparse_timing")
    return {"symbolic_ms": d[0].value, "linearise_ms": d[1].value, "factorize_ms": d[2].value, "solve_ms": d[3].value,
            "fronts": i[0].value, "levels": i[1].value, "widest": i[2].value, "factor_doubles": fd.value, "flops": fl.value}
