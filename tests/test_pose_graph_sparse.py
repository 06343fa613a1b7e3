"""The pose-graph optimizer's sparse solver (options.solver = DVO_AMD_GRAPH_SOLVER_SPARSE): its symbolic phase on the CPU, the
argument checks, and on the GPU the library against the float64 restatement and against the dense path."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_restatement as R  # noqa: E402
import slam_graph  # noqa: E402
from test_pose_graph import MARGIN, _c_edges, _compare, _exp, _non_pd_graph, to_pose_graph  # noqa: E402


# ---- CPU: the symbolic phase ---------------------------------------------------------------------------------------------------
def _chain(m):
    return m + 1, [(i, i + 1) for i in range(m)], [True] + [False] * m


def _ring(m):
    return m, [(i, (i + 1) % m) for i in range(m)], None


def _star(m):
    return m + 1, [(0, i) for i in range(1, m + 1)] + [(i, i + 1) for i in range(1, m, 7)], [True] + [False] * m


def _two_components(m):
    h = m // 2
    return m, [(i, i + 1) for i in range(h - 1)] + [(i, i + 1) for i in range(h, m - 1)] + [(0, h - 1), (h, m - 1)], None


def _slam(frames):
    g, _, _ = slam_graph.slam_graph(frames, seed=frames)
    return len(g.poses), [(f, t) for f, t, _, _ in g.edges], g.fixed


CASES = [("chain", _chain, m) for m in (1, 2, 17, 300, 3000)] + [("ring", _ring, m) for m in (3, 40, 300, 3000)] + \
        [("star", _star, m) for m in (5, 300)] + [("two", _two_components, m) for m in (40, 300)] + \
        [("slam", _slam, m) for m in (60, 300, 3000)]


def _free_slots(nv, pairs, fixed):
    active = sorted({v for p in pairs for v in p})
    free = [v for v in active if not (fixed is not None and fixed[v])]
    return {v: s for s, v in enumerate(free)}


def _check_structure(S, nv, pairs, fixed):
    from dvo_slam_amd import graph

    slot = _free_slots(nv, pairs, fixed)
    m = len(slot)
    assert S["n_free"] == m
    perm = S["perm"]
    assert sorted(perm.tolist()) == list(range(m)), "a permutation of the free active slots"
    pos = np.empty(m, np.int64)
    pos[perm] = np.arange(m)
    nf = len(S["parent"])
    # pivots in postorder concatenate to the permutation
    assert np.array_equal(np.concatenate(S["pivots"]) if nf else np.zeros(0, np.int32), perm)
    anc_piv = []
    for k in range(nf):
        p = S["parent"][k]
        assert p == -1 or (p > k and S["level"][p] > S["level"][k])
        chain, q = set(), p
        while q != -1:
            chain.update(S["pivots"][q].tolist())
            q = S["parent"][q]
        anc_piv.append(chain)
        assert set(S["updates"][k].tolist()) <= chain, "update set inside the ancestors' pivots"
        assert np.all(np.diff(pos[S["updates"][k]]) > 0) and np.all(np.diff(pos[S["pivots"][k]]) > 0)
    return slot, pos


def _fill_covered(S, slot, pos, pairs):
    """block-level symbolic elimination of the permuted pattern: every later neighbour of an eliminated vertex lies in its
    front (later pivots of the front, or its update set)"""
    m = len(slot)
    adj = [set() for _ in range(m)]
    for f, t in pairs:
        if f in slot and t in slot:
            adj[slot[f]].add(slot[t])
            adj[slot[t]].add(slot[f])
    front_of = {}
    for k, pv in enumerate(S["pivots"]):
        for v in pv:
            front_of[int(v)] = k
    for v in S["perm"].tolist():
        later = {w for w in adj[v] if pos[w] > pos[v]}
        k = front_of[v]
        allowed = {int(w) for w in S["pivots"][k] if pos[w] > pos[v]} | set(S["updates"][k].tolist())
        assert later <= allowed, (v, later - allowed)
        for a in later:  # eliminate v: its later neighbours become a clique
            adj[a] |= later - {a}


@pytest.mark.parametrize("name,make,m", CASES, ids=[f"{c[0]}{c[2]}" for c in CASES])
def test_symbolic_structure(name, make, m):
    from dvo_slam_amd import graph

    nv, pairs, fixed = make(m)
    S = graph.symbolic(nv, pairs, fixed)
    slot, pos = _check_structure(S, nv, pairs, fixed)
    if len(slot) <= 300:
        _fill_covered(S, slot, pos, pairs)
    mm = len(slot)
    if name in ("chain", "ring") and mm > 0:
        # nested dissection keeps the tree shallow: a 3000-vertex chain is not a 3000-deep tree
        assert S["n_levels"] <= 2 * np.log2(mm) + 2, (S["n_levels"], mm)
    assert S["factor_doubles"] > 0 and S["flops"] > 0
    again = graph.symbolic(nv, pairs, fixed)
    for key in S:
        a, b = S[key], again[key]
        if isinstance(a, list):
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)
        else:
            assert np.array_equal(a, b), key
    print(f"{name} m={mm}: {len(S['parent'])} fronts, {S['n_levels']} levels, widest {S['widest']}, "
          f"{S['factor_doubles'] / 1e6:.2f} M factor doubles, {S['flops'] / 1e9:.3f} GFLOP")


def _opt_call(L, poses, edges, opt):
    from dvo_slam_amd import graph

    P = np.ascontiguousarray(np.stack([T.T for T in poses]))
    st = graph.CGraphStats()
    return L.dvo_amd_optimize_graph(None, len(poses), P.ctypes.data_as(C.POINTER(C.c_double)), None, len(edges),
                                    _c_edges(edges), C.byref(opt), None, None, 0, None, C.byref(st))


def test_solver_option_checks_and_no_device():
    from dvo_slam_amd import graph

    L = graph._lib()
    assert graph.default_options("dogleg").solver == graph.DENSE == 0 and graph.SPARSE == 1
    poses = [np.eye(4), _exp([0.1, 0, 0, 0, 0, 0.1])]
    good = (0, 1, poses[1], np.eye(6))
    for bad in (2, -1):
        opt = graph.default_options("levenberg")
        opt.solver = bad
        assert _opt_call(L, poses, [good], opt) == 1  # DVO_AMD_ERR_INVALID_ARGUMENT before any device check
    if L.dvo_amd_device_count() > 0:
        return
    opt = graph.default_options("dogleg")
    opt.solver = graph.SPARSE
    assert _opt_call(L, poses, [good], opt) == 2      # DVO_AMD_ERR_NO_DEVICE: there is no CPU path
    P = np.ascontiguousarray(np.stack([T.T for T in poses]))
    assert L.dvo_amd_debug_graph_system_sparse(None, 2, P.ctypes.data_as(C.POINTER(C.c_double)), None, 1, _c_edges([good]),
                                               5.0, 0, None, None, None, None, None, None, None, None) == 2
    assert L.dvo_amd_debug_graph_sparse_timing(None, None, None, None, None, None, None, None, None, None) == 2


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trk():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi.DenseTracker()


def _H_from_blocks(rc, blocks, m):
    H = np.zeros((6 * m, 6 * m))
    for (r, c), B in zip(rc, blocks):
        H[6 * r:6 * r + 6, 6 * c:6 * c + 6] = B
    return H


@pytest.mark.gpu
def test_gpu_sparse_system_matches_dense_bits(trk):
    g, _ = R.ring_graph(574, n_chords=20, star=8, seed=11, noise=1e-3, drift=0.01)  # 573 free vertices
    pg = to_pose_graph(g)
    H, b, x, F, fp = pg.debug_system(trk, 5.0)
    rc, blocks, bs, xs, Fs, fps = pg.debug_system_sparse(trk, 5.0)
    assert fp < 0 and fps < 0 and F == Fs
    assert len(rc) == len({(int(r), int(c)) for r, c in rc})
    for (r, c), B in zip(rc, blocks):
        assert B.tobytes() == H[6 * r:6 * r + 6, 6 * c:6 * c + 6].tobytes(), (r, c)
    Hs = _H_from_blocks(rc, blocks, 573)
    assert Hs.tobytes() == H.tobytes(), "blocks not stored are zero in the dense H"
    assert bs.tobytes() == b.tobytes()
    assert np.linalg.norm(xs - x) <= 1e-9 * np.linalg.norm(x)
    xr = np.linalg.solve(H, b)
    assert np.linalg.norm(xs - xr) <= 1e-9 * np.linalg.norm(xr), np.linalg.norm(xs - xr) / np.linalg.norm(xr)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [30, 200, 573])
@pytest.mark.parametrize("algorithm", ["levenberg", "dogleg"])
def test_gpu_sparse_full_optimization_matches_restatement(trk, m, algorithm):
    g, truth = R.ring_graph(m + 1, n_chords=max(4, m // 30), star=8, seed=100 + m, drift=0.02)
    iters = 50 if algorithm == "levenberg" else 200
    res = to_pose_graph(g).optimize(trk, algorithm, iterations=iters, solver="sparse")
    o = R.optimize(g, algorithm, iterations=iters, follow=res.iterations, margin=MARGIN)
    _compare(res, o, g, o["F0"])
    assert res.final_objective < 1e-10 * res.initial_objective


def _past_cap_graph(kind):
    if kind == "ring":
        g, _ = R.ring_graph(1201, n_chords=40, star=8, seed=1200, drift=0.02)
        return g
    g, _, _ = slam_graph.slam_graph(1201, seed=7, drift=0.01)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ring", "slam"])
@pytest.mark.parametrize("algorithm", ["levenberg", "dogleg"])
def test_gpu_sparse_past_the_dense_cap(trk, kind, algorithm):
    from dvo_slam_amd import graph

    g = _past_cap_graph(kind)
    assert len(g.free) == 1200 > graph.MAX_FREE_VERTICES
    iters = 4
    res = to_pose_graph(g).optimize(trk, algorithm, iterations=iters, solver="sparse")
    o = R.optimize(g, algorithm, iterations=iters, follow=res.iterations, margin=MARGIN)
    _compare(res, o, g, o["F0"])
    assert res.final_objective < res.initial_objective
    print(f"{kind} m=1200 {algorithm}: F {res.initial_objective:.3e} -> {res.final_objective:.3e}, "
          f"{graph.debug_sparse_timing(trk)}")


def _tum_graph():
    return slam_graph.slam_graph(3000, seed=3000, noise=1e-3, drift=0.01)


def _run_tum(t, g):
    pg = to_pose_graph(g)
    a = pg.optimize(t, "dogleg", iterations=100, solver="sparse")
    b = pg.optimize(t, "levenberg", iterations=50, solver="sparse")
    return pg, a, b


def _fingerprint(res):
    return (np.stack(res.poses).tobytes(), res.weight.tobytes(), res.chi2.tobytes(),
            b"".join(v.tobytes() for v in res.iterations.values()), res.final_objective)


@pytest.mark.gpu
def test_gpu_sparse_tum_scale(trk):
    from dvo_slam_amd import graph

    g, truth, keys = _tum_graph()
    pg = to_pose_graph(g)
    lone = pg.add_vertex(_exp([1.0, 2.0, 3.0, 0.1, 0.2, 0.3]))  # touched by no edge
    before = [P.copy() for P in pg.poses]
    rc, blocks, b, x, F0, fp = pg.debug_system_sparse(trk, 5.0)
    assert fp < 0
    m = len(g.free)
    # ||H x - b|| with H from the stored blocks, multiplied on the host (blockwise)
    Hx = np.zeros(6 * m)
    for (r, c), B in zip(rc, blocks):
        Hx[6 * r:6 * r + 6] += B @ x[6 * c:6 * c + 6]
    assert np.linalg.norm(Hx - b) <= 1e-10 * np.linalg.norm(b), np.linalg.norm(Hx - b) / np.linalg.norm(b)
    a = pg.optimize(trk, "dogleg", iterations=100, solver="sparse")
    t = graph.debug_sparse_timing(trk)
    lev = pg.optimize(trk, "levenberg", iterations=50, solver="sparse")
    for res in (a, lev):
        F = np.r_[res.initial_objective, res.iterations["objective"]]
        assert np.all(np.diff(F) <= 0), "F non-increasing"
    again = pg.optimize(trk, "levenberg", iterations=10, solver="sparse")
    moved = abs(again.final_objective - again.initial_objective) / again.initial_objective
    assert not again.iterations["accepted"].any() or moved < 1e-9, moved
    err0 = R.rms_position(before[:len(truth)], truth)
    err1 = R.rms_position(pg.poses[:len(truth)], truth)
    print(f"F=3000 frames, m={m}: RMS {err0:.4f} -> {err1:.5f} m; dogleg {a.n_iterations} it ({a.termination}), "
          f"LM {lev.n_iterations} it; {t}")
    assert err1 * 10 <= err0
    for v in (0, lone):
        assert pg.poses[v].tobytes() == before[v].tobytes(), v


@pytest.mark.gpu
def test_gpu_sparse_deterministic_across_runs_and_contexts(trk):
    from dvo_slam_amd import capi

    g, _, _ = _tum_graph()
    other = capi.DenseTracker()
    outs = []
    for t in (trk, trk, other):
        _, a, b = _run_tum(t, g)
        outs.append((_fingerprint(a), _fingerprint(b)))
    assert outs[0] == outs[1] == outs[2]


@pytest.mark.gpu
def test_gpu_sparse_non_positive_definite_system(trk):
    g = _non_pd_graph()
    pg = to_pose_graph(g)
    _, _, _, x, _, fp = pg.debug_system_sparse(trk, 5.0)
    assert x is None and fp >= 0
    res = to_pose_graph(g).optimize(trk, "dogleg", iterations=100, solver="sparse")
    o = R.optimize(g, "dogleg", iterations=100, follow=res.iterations, margin=MARGIN)
    assert res.cholesky_failures >= 1 and o["cholesky_failures"] >= 1
    assert np.array_equal(res.iterations["lambda"], o["records"]["lambda"]), "lambda sequence"
    lev = to_pose_graph(g).optimize(trk, "levenberg", iterations=50, solver="sparse")
    assert lev.final_objective < 1e-10 * lev.initial_objective and lev.termination != "fail"


@pytest.mark.gpu
def test_gpu_sparse_disconnected_components(trk):
    g1, _ = R.ring_graph(80, n_chords=4, seed=61, drift=0.02)
    g2, _ = R.ring_graph(50, n_chords=3, seed=62, drift=0.02)
    off = len(g1.poses)
    joint = R.Graph(g1.poses + g2.poses, g1.fixed + g2.fixed,
                    g1.edges + [(f + off, t + off, Z, O) for f, t, Z, O in g2.edges])
    assert len(graph_roots(joint)) >= 2
    res = to_pose_graph(joint).optimize(trk, "levenberg", iterations=50, solver="sparse")
    r1 = to_pose_graph(g1).optimize(trk, "levenberg", iterations=50, solver="sparse")
    r2 = to_pose_graph(g2).optimize(trk, "levenberg", iterations=50, solver="sparse")
    for r in (res, r1, r2):
        assert r.final_objective < 1e-10 * r.initial_objective
    sep = r1.poses + r2.poses
    for v in range(len(sep)):
        assert np.max(np.abs(res.poses[v] - sep[v])) <= 1e-7, v


def graph_roots(g):
    from dvo_slam_amd import graph

    S = graph.symbolic(len(g.poses), [(f, t) for f, t, _, _ in g.edges], g.fixed)
    return [k for k, p in enumerate(S["parent"]) if p == -1]


@pytest.mark.gpu
def test_gpu_sparse_capacity(trk):
    from dvo_slam_amd import capi, graph

    m = graph.MAX_FREE_VERTICES_SPARSE + 1
    pg = graph.PoseGraph()
    pg.add_vertex(fixed=True)
    Z = _exp([0.1, 0, 0, 0, 0, 0])
    for i in range(m):
        pg.add_vertex(np.eye(4))
        pg.add_edge(i, i + 1, Z, np.eye(6))
    before = [P.copy() for P in pg.poses]
    with pytest.raises(capi.DvoAmdError) as ei:
        pg.optimize(trk, "dogleg", solver="sparse")
    assert ei.value.status == 7
    assert all(np.array_equal(a, b) for a, b in zip(pg.poses, before))


@pytest.mark.gpu
def test_gpu_sparse_no_free_vertex_on_a_fresh_context():
    from dvo_slam_amd import capi, graph

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    for case in ("edgeless", "all fixed"):
        t = capi.DenseTracker()  # a fresh context: no workspace from an earlier, larger call
        pg = graph.PoseGraph()
        for i in range(4):
            pg.add_vertex(_exp([0.1 * i, 0.2, 0.0, 0.0, 0.05 * i, 0.0]), fixed=case == "all fixed")
        if case == "all fixed":
            for i in range(3):
                pg.add_edge(i, i + 1, _exp([0.1, 0, 0, 0, 0.05, 0]), np.eye(6))
        before = [P.copy() for P in pg.poses]
        for algorithm in ("levenberg", "dogleg"):
            res = pg.optimize(t, algorithm, solver="sparse")
            assert res.n_free == 0 and res.n_iterations == 0, case
            assert all(a.tobytes() == b.tobytes() for a, b in zip(res.poses, before)), case


def lattice_graph(dims, copies, seed):
    """copies disjoint 3-D lattices of dims vertices (6-neighbour edges); per lattice its first vertex fixed; measurements the
    true relative poses, the initial estimate the truth times a seeded perturbation.  Nested dissection gives these lattices
    separators of dozens of vertices: fronts of the tiled tier."""
    rng = np.random.default_rng(seed)
    A, B, Cz = dims
    n = A * B * Cz
    truth, fixed, edges = [], [], []
    for c in range(copies):
        for z in range(Cz):
            for y in range(B):
                for x in range(A):
                    truth.append(_exp(np.r_[0.5 * x, 0.5 * y + 10.0 * c, 0.5 * z, rng.normal(scale=0.1, size=3)]))
                    fixed.append(len(truth) - 1 == c * n)
        idx = lambda x, y, z: c * n + (z * B + y) * A + x  # noqa: E731
        for z in range(Cz):
            for y in range(B):
                for x in range(A):
                    for dx, dy, dz in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
                        if x + dx < A and y + dy < B and z + dz < Cz:
                            f, t = idx(x, y, z), idx(x + dx, y + dy, z + dz)
                            edges.append((f, t, R.inverse(truth[f]) @ truth[t], R.information(rng)))
    poses = [T if f else T @ _exp(rng.normal(scale=0.02, size=6)) for T, f in zip(truth, fixed)]
    return R.Graph(poses, fixed, edges)


def _wide_fronts(g):
    from dvo_slam_amd import graph

    S = graph.symbolic(len(g.poses), [(f, t) for f, t, _, _ in g.edges], g.fixed)
    wide = [k for k in range(len(S["parent"]))
            if 6 * len(S["pivots"][k]) > 192 or 6 * (len(S["pivots"][k]) + len(S["updates"][k])) > 1024]
    return S, wide


@pytest.mark.gpu
@pytest.mark.parametrize("dims,copies", [((9, 8, 7), 2), ((10, 10, 10), 1)], ids=["two-wide-on-one-level", "wide-over-wide"])
def test_gpu_sparse_wide_fronts(trk, dims, copies):
    g = lattice_graph(dims, copies, seed=sum(dims) + copies)
    S, wide = _wide_fronts(g)
    levels = [int(S["level"][k]) for k in wide]
    if copies == 2:
        assert len(wide) >= 2 and len(set(levels)) < len(levels), "two wide fronts on one level"
    else:
        assert any(S["parent"][k] in wide for k in wide), "a wide front whose parent is wide"
    pg = to_pose_graph(g)
    H, b, x, F, fp = pg.debug_system(trk, 5.0)
    rc, blocks, bs, xs, Fs, fps = pg.debug_system_sparse(trk, 5.0)
    m = len(g.free)
    assert fp < 0 and fps < 0
    assert _H_from_blocks(rc, blocks, m).tobytes() == H.tobytes() and bs.tobytes() == b.tobytes()
    xr = np.linalg.solve(H, b)
    assert np.linalg.norm(xs - x) <= 1e-9 * np.linalg.norm(x)
    assert np.linalg.norm(xs - xr) <= 1e-9 * np.linalg.norm(xr), np.linalg.norm(xs - xr) / np.linalg.norm(xr)
    iters = 4
    res = to_pose_graph(g).optimize(trk, "levenberg", iterations=iters, solver="sparse")
    o = R.optimize(g, "levenberg", iterations=iters, follow=res.iterations, margin=MARGIN)
    _compare(res, o, g, o["F0"])
    assert res.final_objective < res.initial_objective
    print(f"lattice {dims} x {copies}: m={m}, {len(wide)} wide fronts on levels {levels} of {S['n_levels']}")
