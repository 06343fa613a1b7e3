"""Marginal covariances of pose-graph vertices (dvo_amd_graph_marginals, graph.PoseGraph.marginals): blocks of H^-1 from the GPU
solvers against np.linalg.inv of the restatement's own H.  The bar is 1e-9 block-relative (the bar one undamped solve has in
test_pose_graph.py), on graphs whose reference agrees with itself to 1e-11."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_marginals_cases as M  # noqa: E402
import pose_graph_restatement as R  # noqa: E402
from test_pose_graph import _c_edges, _exp, _planted_outlier_graph, to_pose_graph  # noqa: E402
from test_pose_graph_sparse import _wide_fronts, graph_roots, lattice_graph  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR, CONDITION = M.BAR, M.CONDITION
RINGS = ["ring30", "ring200", "ring573"]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def _call(poses, edges, opt, pairs, fixed=None, ctx=None, blocks=True, a_null=False):
    from dvo_slam_amd import graph

    L = graph._lib()
    P = np.ascontiguousarray(np.stack([T.T for T in poses]))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    k = len(pairs) if not isinstance(pairs, int) else pairs
    pr = np.asarray(pairs if not isinstance(pairs, int) else [], dtype=np.int32).reshape(-1, 2)
    a, b = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    out = np.zeros(36 * max(len(pr), 1))
    st = graph.CGraphMarginalStats()
    fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed, dtype=np.int32))
    return L.dvo_amd_graph_marginals(ctx, len(poses), P.ctypes.data_as(dp), None if fx is None else fx.ctypes.data_as(ip),
                                     len(edges), _c_edges(edges), None if opt is None else C.byref(opt), k,
                                     None if a_null or not len(pr) else a.ctypes.data_as(ip),
                                     b.ctypes.data_as(ip) if len(pr) else None, out.ctypes.data_as(dp) if blocks else None,
                                     C.byref(st))


def test_marginals_argument_checks_and_no_device():
    from dvo_slam_amd import graph

    L = graph._lib()
    opt = graph.default_options("dogleg")
    poses = [np.eye(4), _exp([0.1, 0, 0, 0, 0, 0.1])]
    good = (0, 1, poses[1], np.eye(6))
    INV, CAP = 1, 7
    # the checks of dvo_amd_optimize_graph
    assert _call(poses, [good], None, [(0, 0)]) == INV
    assert _call(poses, [(0, 2, np.eye(4), np.eye(6))], opt, [(0, 0)]) == INV
    assert _call(poses, [(-1, 1, np.eye(4), np.eye(6))], opt, [(0, 0)]) == INV
    assert _call(poses, [(1, 1, np.eye(4), np.eye(6))], opt, [(0, 0)]) == INV
    Zn = np.eye(4)
    Zn[0, 3] = np.nan
    assert _call(poses, [(0, 1, Zn, np.eye(6))], opt, [(0, 0)]) == INV
    On = np.eye(6)
    On[2, 2] = np.inf
    assert _call(poses, [(0, 1, np.eye(4), On)], opt, [(0, 0)]) == INV
    assert _call([np.eye(4), np.full((4, 4), np.nan)], [good], opt, [(0, 0)]) == INV
    Oa = np.eye(6)
    Oa[0, 1] = 1e-3
    assert _call(poses, [(0, 1, np.eye(4), Oa)], opt, [(0, 0)]) == INV
    for field, value in (("algorithm", 7), ("solver", 2), ("max_iterations", -1), ("max_trials", 0),
                         ("robust_delta", float("nan")), ("initial_lambda", float("inf"))):
        bad = graph.default_options("dogleg")
        setattr(bad, field, value)  # options the entry does not read are still validated
        assert _call(poses, [good], bad, [(0, 0)]) == INV, field
    # the entry's own: n_blocks < 0, index out of range, NULL arrays with n_blocks > 0
    assert _call(poses, [good], opt, -1) == INV
    assert _call(poses, [good], opt, [(0, 2)]) == INV
    assert _call(poses, [good], opt, [(-1, 0)]) == INV
    assert _call(poses, [good], opt, [(0, 1)], blocks=False) == INV
    assert _call(poses, [good], opt, [(0, 1)], a_null=True) == INV
    # capacity of the chosen solver, before any device is looked for
    Zs = _exp([0.1, 0, 0, 0, 0, 0])
    for solver, cap in ((graph.DENSE, graph.MAX_FREE_VERTICES), (graph.SPARSE, graph.MAX_FREE_VERTICES_SPARSE)):
        o = graph.default_options("dogleg")
        o.solver = solver
        chain = [np.eye(4)] * (cap + 2)
        edges = [(i, i + 1, Zs, np.eye(6)) for i in range(cap + 1)]
        assert _call(chain, edges, o, [(1, 1)], fixed=[1] + [0] * (cap + 1)) == CAP, solver
    if L.dvo_amd_device_count() > 0:
        return
    # valid arguments without a GPU: no device (and no CPU path), also for a stats-only call
    assert _call(poses, [good], opt, [(0, 0), (1, 0)]) == 2
    assert _call(poses, [good], opt, 0, blocks=False) == 2


@pytest.mark.parametrize("name", RINGS + ["slam1200"])
def test_reference_agrees_with_itself_and_is_a_covariance(name):
    g, H, Z = M.dense_reference(name)
    d = M.self_distance(H, Z)
    print(f"{name}: n={H.shape[0]}, inv vs Cholesky inverse {d:.2e}")
    assert d <= CONDITION
    assert M.block_rel(Z.T, Z) <= CONDITION
    np.linalg.cholesky(0.5 * (Z + Z.T))  # positive definite
    if name == "slam1200":  # the block-sparse assembly of the restated H is the restatement's H
        assert M.block_rel(M.sparse_H(g).toarray(), H) <= 1e-12


def test_reference_columns_agree_at_3000_frames():
    g = M.slam3000()
    Hs = M.sparse_H(g)
    slots = _sampled_slots(g)
    A = M.block_columns(Hs, slots, "COLAMD")
    B = M.block_columns(Hs, slots, "MMD_AT_PLUS_A")
    d = M.block_rel(A, B)
    print(f"slam3000: n={Hs.shape[0]}, 20 block columns, splu(COLAMD) vs splu(MMD_AT_PLUS_A) {d:.2e}")
    assert d <= CONDITION


def _sampled_slots(g, count=20, seed=3000):
    return sorted(int(s) for s in np.random.default_rng(seed).choice(len(g.free), size=count, replace=False))


def test_open_chain_uncertainty_grows_along_the_chain():
    rng = np.random.default_rng(4)
    truth = [np.eye(4)]
    for _ in range(40):
        truth.append(truth[-1] @ _exp(np.r_[0.3, rng.normal(scale=0.05, size=5)]))
    edges = [(i, i + 1, R.inverse(truth[i]) @ truth[i + 1], R.information(rng)) for i in range(40)]
    g = R.Graph(truth, [True] + [False] * 40, edges)
    Z = np.linalg.inv(R.linearise(g, 5.0)[0])
    # positional covariance in the world frame: the increment's translation is in the vertex's own frame
    tr = [np.trace(Z[6 * s:6 * s + 3, 6 * s:6 * s + 3]) for s in range(40)]
    assert np.all(np.diff(tr) >= 0), tr


def test_relative_covariance_matches_central_differences_and_rotation_units():
    from dvo_slam_amd import graph

    rng = np.random.default_rng(12)
    h = 1e-6
    for _ in range(8):
        Xa, Xb = _exp(rng.normal(size=6)), _exp(rng.normal(size=6))
        A = rng.normal(size=(12, 12))
        S = A @ A.T * 1e-4  # a joint covariance of (d_a, d_b)
        J = np.zeros((6, 12))
        for i in range(12):
            d = np.zeros(12)
            d[i] = h
            ep = R.edge_error(Xa @ R.inc(d[:6]), Xb @ R.inc(d[6:]), np.eye(4))
            em = R.edge_error(Xa @ R.inc(-d[:6]), Xb @ R.inc(-d[6:]), np.eye(4))
            J[:, i] = (ep - em) / (2 * h)
        want = J @ S @ J.T
        got = graph.relative_covariance(Xa, Xb, S[:6, :6], S[:6, 6:], S[6:, 6:])
        assert np.max(np.abs(got - want)) <= 1e-6 * np.max(np.abs(want))
        assert np.array_equal(got, got.T) or np.max(np.abs(got - got.T)) <= 1e-15 * np.max(np.abs(got))
    s = graph.ROTATION_VECTOR_SCALE
    assert np.array_equal(s, [1, 1, 1, 2, 2, 2])


def test_graph_marginals_example_compiles_as_c99(tmp_path):
    res = subprocess.run(["cc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "examples", "graph_marginals_example.c"), "-c", "-o",
                          str(tmp_path / "graph_marginals_example.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trk():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi.DenseTracker()


def _check_against_dense_reference(trk, name, solver):
    g, _, Z = M.dense_reference(name)
    pairs = M.requests(g, seed=len(g.poses))
    blocks, st = to_pose_graph(g).marginals(trk, pairs, solver=solver)
    want = M.expected(g, Z, pairs)
    d = M.block_rel(blocks, want)
    print(f"{solver} {name}: {len(pairs)} blocks, worst distance {d:.2e}, solved_columns {st.solved_columns}")
    assert st.factorized == 1 and st.n_free == len(g.free)
    assert st.fixed_blocks == sum(1 for a, b in pairs if g.fixed[a] or g.fixed[b]) and st.inactive_blocks == 0
    assert d <= BAR
    return g, Z, blocks, pairs, st


@pytest.mark.gpu
@pytest.mark.parametrize("name", RINGS)
def test_gpu_dense_marginals_match_reference(trk, name):
    _, _, _, _, st = _check_against_dense_reference(trk, name, "dense")
    assert st.solved_columns == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", RINGS + ["slam1200"])
def test_gpu_sparse_marginals_match_reference(trk, name):
    g, Z, _, pairs, st = _check_against_dense_reference(trk, name, "sparse")
    # diagonals and edge pairs alone come from the fronts; far-apart pairs take the solves and are still within the bar
    near = pairs[:len(pairs) - 50]
    blocks, st2 = to_pose_graph(g).marginals(trk, near, solver="sparse")
    assert st2.solved_columns == 0
    assert M.block_rel(blocks, M.expected(g, Z, near)) <= BAR
    free = g.free
    far = [(free[i], free[(i + len(free) // 2) % len(free)]) for i in range(0, len(free), max(1, len(free) // 12))]
    joined = {(f, t) for f, t, _, _ in g.edges} | {(t, f) for f, t, _, _ in g.edges}
    far = [p for p in far if p not in joined]
    blocks, st3 = to_pose_graph(g).marginals(trk, far, solver="sparse")
    d = M.block_rel(blocks, M.expected(g, Z, far))
    print(f"sparse {name}: {len(far)} far pairs, solved_columns {st3.solved_columns}, worst distance {d:.2e}")
    assert st3.solved_columns > 0 and d <= BAR


@pytest.mark.gpu
def test_gpu_sparse_marginals_at_3000_frames(trk):
    g = M.slam3000()
    slots = _sampled_slots(g)
    cols = M.block_columns(M.sparse_H(g), slots)
    free = g.free
    neighbours = {v: set() for v in range(len(g.poses))}
    for f, t, _, _ in g.edges:
        neighbours[f].add(t), neighbours[t].add(f)
    rng = np.random.default_rng(1)
    near, far, want_near, want_far = [], [], [], []
    for i, s in enumerate(slots):
        c = free[s]
        rows = [c] + sorted(v for v in neighbours[c] if not g.fixed[v])
        for a in rows:
            blk = cols[6 * g.slot[a]:6 * g.slot[a] + 6, 6 * i:6 * i + 6]
            near += [(a, c), (c, a)]
            want_near += [blk, blk.T]
        for a in (free[int(x)] for x in rng.integers(0, len(free), size=3)):
            if a != c and a not in neighbours[c]:
                blk = cols[6 * g.slot[a]:6 * g.slot[a] + 6, 6 * i:6 * i + 6]
                far += [(a, c), (c, a)]
                want_far += [blk, blk.T]
    pg = to_pose_graph(g)
    b1, s1 = pg.marginals(trk, near, solver="sparse")
    b2, s2 = pg.marginals(trk, far, solver="sparse")
    d1, d2 = M.block_rel(b1, np.stack(want_near)), M.block_rel(b2, np.stack(want_far))
    print(f"sparse slam3000: {len(near)} near blocks {d1:.2e} (solved_columns {s1.solved_columns}), {len(far)} far blocks "
          f"{d2:.2e} (solved_columns {s2.solved_columns})")
    assert s1.factorized == 1 and s1.n_free == len(free) and s1.solved_columns == 0 and s2.solved_columns > 0
    assert d1 <= BAR and d2 <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("name", RINGS)
def test_gpu_dense_and_sparse_marginals_agree(trk, name):
    g = M.GRAPHS[name]()
    pairs = M.requests(g, seed=7)
    pg = to_pose_graph(g)
    a, _ = pg.marginals(trk, pairs, solver="dense")
    b, _ = pg.marginals(trk, pairs, solver="sparse")
    d = max(M.block_rel(a, b), M.block_rel(b, a))
    print(f"{name}: dense vs sparse {d:.2e}")
    assert d <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["dense", "sparse"])
def test_gpu_marginals_after_optimize_hold_the_robust_weights(trk, solver):
    g, _ = _planted_outlier_graph()
    pg = to_pose_graph(g)
    res = pg.optimize(trk, "dogleg", iterations=200, solver=solver)
    assert res.weight[-1] < 0.05
    H = R.linearise(g, 5.0, poses=pg.poses)[0]
    H1 = R.linearise(g, 0.0, poses=pg.poses)[0]
    Z = np.linalg.inv(H)
    assert M.self_distance(H, Z) <= CONDITION
    pairs = M.requests(g, seed=3)
    blocks, st = pg.marginals(trk, pairs, solver=solver)
    d = M.block_rel(blocks, M.expected(g, Z, pairs))
    off = M.block_rel(blocks, M.expected(g, np.linalg.inv(H1), pairs))
    print(f"{solver}: after optimize {d:.2e} (against the unweighted H: {off:.2e})")
    assert st.factorized == 1 and d <= BAR
    assert off > 1e-3  # the Cauchy weight is in H: without it the answer is another


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["dense", "sparse"])
def test_gpu_marginals_fixed_inactive_floating_and_empty(solver):
    from dvo_slam_amd import capi, graph

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    t = capi.DenseTracker()  # a fresh context, first used for marginals
    g = M.ring(30)
    poses = g.poses + [np.eye(4), _exp([1.0, 0, 0, 0, 0, 0])]  # two vertices no edge touches; the last one fixed
    g2 = R.Graph(poses, g.fixed + [False, True], g.edges)
    lone, lone_fixed = len(poses) - 2, len(poses) - 1
    pairs = [(0, 0), (0, 5), (5, 0), (lone, lone), (lone, 3), (3, lone), (lone_fixed, lone), (lone_fixed, 4), (5, 5), (5, 9)]
    blocks, st = to_pose_graph(g2).marginals(t, pairs, solver=solver)
    Z = np.linalg.inv(R.linearise(g2, 5.0)[0])
    assert (st.factorized, st.n_free, st.fixed_blocks, st.inactive_blocks) == (1, 30, 5, 3)
    for k in (0, 1, 2, 6, 7):
        assert np.array_equal(blocks[k], np.zeros((6, 6)))
    for k in (3, 4, 5):
        assert np.all(np.isnan(blocks[k]))
    assert M.block_rel(blocks[8:], M.expected(g2, Z, pairs[8:])) <= BAR
    # the default request: every vertex's diagonal block in vertex order
    diag, st = to_pose_graph(g2).marginals(t, solver=solver)
    assert diag.shape == (len(poses), 6, 6) and st.fixed_blocks == 2 and st.inactive_blocks == 1
    assert M.block_rel(diag[1:31], M.expected(g2, Z, [(v, v) for v in range(1, 31)])) <= BAR
    vec, _ = to_pose_graph(g2).marginals(t, [(5, 9)], solver=solver, rotation="vector")
    s = graph.ROTATION_VECTOR_SCALE
    assert np.array_equal(vec[0], blocks[9] * np.outer(s, s))
    # a component with no fixed vertex: not an error, factorized == 0, NaN blocks (a fixed vertex's zeros stay)
    f = R.ring_graph(24, n_chords=4, seed=5, fixed_first=False)[0]
    f2 = R.Graph(f.poses + [np.eye(4)], f.fixed + [True], f.edges)
    blocks, st = to_pose_graph(f2).marginals(t, [(1, 1), (2, 3), (24, 1), (24, 24)], solver=solver)
    assert st.factorized == 0 and st.n_free == 24 and st.fixed_blocks == 2
    assert np.all(np.isnan(blocks[:2])) and np.array_equal(blocks[2:], np.zeros((2, 6, 6)))
    # no free active vertex
    pg = graph.PoseGraph()
    for i in range(3):
        pg.add_vertex(_exp([0.1 * i, 0, 0, 0, 0, 0]), fixed=True)
    pg.add_edge(0, 1, np.eye(4), np.eye(6))
    blocks, st = pg.marginals(t, solver=solver)
    assert (st.factorized, st.n_free, st.fixed_blocks) == (1, 0, 3) and np.array_equal(blocks, np.zeros((3, 6, 6)))
    blocks, st = pg.marginals(t, [], solver=solver)
    assert blocks.shape == (0, 6, 6) and st.factorized == 1


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["dense", "sparse"])
def test_gpu_marginals_bits(trk, solver):
    from dvo_slam_amd import capi

    g = M.ring(200)
    free = g.free
    pairs = M.requests(g, seed=11) + [(free[3], free[120]), (free[120], free[3]), (free[150], free[40])]
    pg = to_pose_graph(g)
    a, _ = pg.marginals(trk, pairs, solver=solver)
    b, _ = pg.marginals(trk, pairs, solver=solver)
    c, _ = pg.marginals(capi.DenseTracker(), pairs, solver=solver)
    assert a.tobytes() == b.tobytes() == c.tobytes()
    index = {}
    for k, p in enumerate(pairs):
        index.setdefault(p, k)
    for (x, y), k in index.items():
        if x == y:
            assert np.array_equal(a[k], a[k].T), (x, y)
        if (y, x) in index:
            assert a[k].tobytes() == np.ascontiguousarray(a[index[(y, x)]].T).tobytes(), (x, y)
    for p in [pairs[5], pairs[250], (free[3], free[120]), (free[120], free[3]), (free[150], free[40]), (free[7], free[7])]:
        alone, _ = pg.marginals(trk, [p], solver=solver)
        assert alone[0].tobytes() == a[index[p]].tobytes(), p
    rev, _ = pg.marginals(trk, pairs[::-1], solver=solver)
    assert rev[::-1].tobytes() == a.tobytes()


@pytest.mark.gpu
def test_gpu_marginals_capacity(trk):
    from dvo_slam_amd import capi, graph

    for solver, cap in (("dense", graph.MAX_FREE_VERTICES), ("sparse", graph.MAX_FREE_VERTICES_SPARSE)):
        pg = graph.PoseGraph()
        pg.add_vertex(fixed=True)
        Z = _exp([0.1, 0, 0, 0, 0, 0])
        for i in range(cap + 1):
            pg.add_vertex(np.eye(4))
            pg.add_edge(i, i + 1, Z, np.eye(6))
        with pytest.raises(capi.DvoAmdError) as ei:
            pg.marginals(trk, [(1, 1)], solver=solver)
        assert ei.value.status == 7


@pytest.mark.gpu
def test_gpu_marginals_disconnected_components(trk):
    g1, _ = R.ring_graph(80, n_chords=4, seed=61, drift=0.02)
    g2, _ = R.ring_graph(50, n_chords=3, seed=62, drift=0.02)
    off = len(g1.poses)
    joint = R.Graph(g1.poses + g2.poses, g1.fixed + g2.fixed, g1.edges + [(f + off, t + off, Z, O) for f, t, Z, O in g2.edges])
    assert len(graph_roots(joint)) >= 2
    H = R.linearise(joint, 5.0)[0]
    Z = np.linalg.inv(H)
    assert M.self_distance(H, Z) <= CONDITION
    pairs = M.requests(joint, seed=2) + [(5, off + 7), (off + 7, 5)]  # across components: zero covariance
    for solver in ("dense", "sparse"):
        blocks, st = to_pose_graph(joint).marginals(trk, pairs, solver=solver)
        d = M.block_rel(blocks[:-2], M.expected(joint, Z, pairs[:-2]))
        print(f"{solver} two components: {d:.2e}")
        assert st.factorized == 1 and d <= BAR
        assert np.max(np.abs(blocks[-2:])) <= 1e-20


@pytest.mark.gpu
@pytest.mark.parametrize("dims,copies", [((9, 8, 7), 2), ((10, 10, 10), 1)], ids=["two-wide-on-one-level", "wide-over-wide"])
def test_gpu_sparse_marginals_wide_fronts(trk, dims, copies):
    g = lattice_graph(dims, copies, seed=sum(dims) + copies)
    S, wide = _wide_fronts(g)
    assert len(wide) >= 2
    H = R.linearise(g, 5.0)[0]
    Z = np.linalg.inv(H)
    sd = M.self_distance(H, Z)
    assert sd <= CONDITION
    pairs = M.requests(g, n_random=0)
    blocks, st = to_pose_graph(g).marginals(trk, pairs, solver="sparse")
    d = M.block_rel(blocks, M.expected(g, Z, pairs))
    # every pair of pivots of a wide front meets in that front: the tiled path's blocks, and no pad pivot among them
    free = g.free
    inside = [(free[a], free[b]) for k in wide for a in S["pivots"][k][::5] for b in S["pivots"][k][::7]]
    blocks2, st2 = to_pose_graph(g).marginals(trk, inside, solver="sparse")
    d2 = M.block_rel(blocks2, M.expected(g, Z, inside))
    print(f"lattice {dims} x {copies}: m={len(free)}, {len(wide)} wide fronts, reference self-distance {sd:.1e}, "
          f"{len(pairs)} blocks {d:.2e}, {len(inside)} blocks inside wide fronts {d2:.2e}")
    assert st.factorized == 1 and st.solved_columns == 0 and st2.solved_columns == 0
    assert d <= BAR and d2 <= BAR
    if len(free) <= 1024:
        dense, _ = to_pose_graph(g).marginals(trk, pairs, solver="dense")
        assert M.block_rel(dense, blocks) <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["dense", "sparse"])
def test_gpu_optimize_is_untouched_by_a_marginals_call(trk, solver):
    g = M.ring(200)

    def run():
        res = to_pose_graph(g).optimize(trk, "levenberg", iterations=6, solver=solver)
        return (np.stack(res.poses).tobytes(), res.weight.tobytes(), res.chi2.tobytes(), res.iterations["objective"].tobytes())

    before = run()
    to_pose_graph(g).marginals(trk, M.requests(g, seed=1), solver=solver)
    to_pose_graph(M.ring(30)).marginals(trk, solver=solver)
    assert run() == before
