"""Pose-graph optimization (dvo_amd_optimize_graph, dvo_slam_amd.graph): the float64 restatement of the semantics on the CPU,
the argument checks, and on the GPU the library against the restatement."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-6


def _exp(xi):
    from dvo_slam_amd import synth

    return synth.se3_exp(xi)


def to_pose_graph(g: R.Graph):
    from dvo_slam_amd import graph

    pg = graph.PoseGraph()
    for P, f in zip(g.poses, g.fixed):
        pg.add_vertex(P, fixed=f)
    for f, t, Z, O in g.edges:
        pg.add_edge(f, t, Z, O)
    return pg


def rotation_angle(A, B):
    c = (np.trace(A[:3, :3].T @ B[:3, :3]) - 1.0) / 2.0
    return float(np.arccos(np.clip(c, -1.0, 1.0))) if c < 1 - 1e-12 else float(np.linalg.norm(
        0.5 * np.array([(A[:3, :3].T @ B[:3, :3])[2, 1] - (A[:3, :3].T @ B[:3, :3])[1, 2],
                        (A[:3, :3].T @ B[:3, :3])[0, 2] - (A[:3, :3].T @ B[:3, :3])[2, 0],
                        (A[:3, :3].T @ B[:3, :3])[1, 0] - (A[:3, :3].T @ B[:3, :3])[0, 1]])))


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------
def _random_triplets():
    rng = np.random.default_rng(7)
    out = []
    for k in range(24):
        Xf, Xt = _exp(rng.normal(size=6)), _exp(rng.normal(size=6))
        kind = k % 4
        if kind == 0:
            Z = _exp(rng.normal(size=6))
        elif kind == 1:  # small rotation error
            Z = R.inverse(Xf) @ Xt @ _exp(rng.normal(scale=1e-3, size=6))
        elif kind == 2:  # near pi
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            Z = R.inverse(Xf) @ Xt @ _exp(np.r_[rng.normal(size=3) * 0.1, ax * (np.pi - 1e-3)])
        else:  # exactly consistent
            Z = R.inverse(Xf) @ Xt
        out.append((Xf, Xt, Z))
    return out


def test_restatement_jacobians_match_central_differences():
    for Xf, Xt, Z in _random_triplets():
        Jf, Jt = R.jacobians(Xf, Xt, Z)
        Nf, Nt = R.numeric_jacobians(Xf, Xt, Z, 1e-6)
        assert np.all(np.abs(Jf - Nf) <= 1e-6 * (np.abs(Nf) + 1)), np.max(np.abs(Jf - Nf))
        assert np.all(np.abs(Jt - Nt) <= 1e-6 * (np.abs(Nt) + 1)), np.max(np.abs(Jt - Nt))


def test_inc_and_to_vector_mqt_round_trip():
    rng = np.random.default_rng(3)
    for _ in range(50):
        d = np.r_[rng.normal(size=3), rng.uniform(-0.5, 0.5, size=3)]
        assert np.allclose(R.to_vector_mqt(R.inc(d)), d, atol=1e-13)
        T = _exp(rng.normal(size=6))
        assert np.allclose(R.inc(R.to_vector_mqt(T)), T, atol=1e-13)
    # 1 - |q|^2 < 0: identity rotation
    T = R.inc([1.0, 2.0, 3.0, 0.8, 0.8, 0.0])
    assert np.array_equal(T[:3, :3], np.eye(3)) and np.array_equal(T[:3, 3], [1.0, 2.0, 3.0])


@pytest.mark.parametrize("algorithm", ["levenberg", "dogleg"])
def test_restatement_lowers_F_to_a_stationary_point(algorithm):
    g, truth = R.ring_graph(24, n_chords=6, seed=5, noise=1e-3)
    o = R.optimize(g, algorithm, iterations=50 if algorithm == "levenberg" else 200)
    F = o["records"]["objective"]
    acc = o["records"]["accepted"].astype(bool)
    assert F[0] < o["F0"]
    prev = np.r_[o["F0"], F[:-1]]
    assert np.all(F[acc] < prev[acc]), "every kept step lowers F strictly"
    assert np.all(F[~acc] == prev[~acc])
    # |grad F| relative to the start: the absolute floor is the rounding of F (an information of 2500 puts it near 1e-7)
    assert R.gradient_norm(g, o["poses"], 5.0) < 1e-8 * R.gradient_norm(g, g.poses, 5.0)
    assert R.rms_position(o["poses"], truth) < 0.1 * R.rms_position(g.poses, truth)


def _planted_outlier_graph():
    g, truth = R.ring_graph(20, n_chords=6, seed=9, noise=1e-3)
    Z = R.inverse(truth[2]) @ truth[12]
    Z[:3, 3] += [5.0, 0.0, 0.0]  # a wrong loop edge, 5 m off
    g.edges.append((2, 12, Z, R.information(np.random.default_rng(1))))
    return R.Graph(g.poses, g.fixed, g.edges), truth


def test_restatement_planted_outlier_is_down_weighted():
    g, _ = _planted_outlier_graph()
    o = R.optimize(g, "dogleg", iterations=200)
    assert o["rho1"][-1] < 0.05
    assert np.all(o["rho1"][:-1] > 0.9)


def test_remove_outlier_edges_orders_by_weight():
    from dvo_slam_amd import graph

    pg = graph.PoseGraph()
    for _ in range(4):
        pg.add_vertex()
    for k in range(6):
        pg.add_edge(k % 4, (k + 1) % 4, np.eye(4), np.eye(6))

    class Last:
        weight = np.array([0.9, 0.01, 0.5, 0.2, 0.01, 0.95])
        robust_delta = 5.0

    pg.last = Last()
    assert pg.remove_outlier_edges(0.6, n_max=3) == [1, 4, 3]
    assert pg.live_edges() == [0, 2, 5]
    assert pg.remove_outlier_edges(0.6) == [2]
    Last.robust_delta = 0.0  # no kernel: the reference skips edges without one
    assert pg.remove_outlier_edges(1.0) == []


def test_pose_graph_example_compiles_as_c99(tmp_path):
    exe = str(tmp_path / "pose_graph_example")
    res = subprocess.run(["cc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "examples", "pose_graph_example.c"), "-c", "-o", exe + ".o"],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def _c_edges(edges):
    from dvo_slam_amd import graph

    ce = (graph.CGraphEdge * max(len(edges), 1))()
    for i, (f, t, Z, O) in enumerate(edges):
        ce[i].from_, ce[i].to = f, t
        ce[i].measurement[:] = list(np.asarray(Z, dtype=np.float64).T.reshape(-1))
        ce[i].information[:] = list(np.asarray(O, dtype=np.float64).T.reshape(-1))
    return ce


def _call(L, poses, edges, opt, ctx=None):
    from dvo_slam_amd import graph

    P = np.ascontiguousarray(np.stack([T.T for T in poses]))
    st = graph.CGraphStats()
    dp = C.POINTER(C.c_double)
    return L.dvo_amd_optimize_graph(ctx, len(poses), P.ctypes.data_as(dp), None, len(edges), _c_edges(edges), C.byref(opt),
                                    None, None, 0, None, C.byref(st))


def test_argument_checks_and_no_device():
    from dvo_slam_amd import graph

    L = graph._lib()
    opt = graph.default_options("dogleg")
    assert (opt.max_iterations, opt.max_trials, opt.initial_lambda, opt.initial_delta, opt.robust_delta) == (100, 100, 1e-7,
                                                                                                             1e4, 5.0)
    lev = graph.default_options("levenberg")
    assert (lev.max_iterations, lev.max_trials, lev.initial_lambda) == (50, 10, 0.0)
    poses = [np.eye(4), _exp([0.1, 0, 0, 0, 0, 0.1])]
    good = (0, 1, poses[1], np.eye(6))
    INV = 1
    assert _call(L, poses, [(0, 2, np.eye(4), np.eye(6))], opt) == INV
    assert _call(L, poses, [(-1, 1, np.eye(4), np.eye(6))], opt) == INV
    assert _call(L, poses, [(1, 1, np.eye(4), np.eye(6))], opt) == INV
    Zn = np.eye(4)
    Zn[0, 3] = np.nan
    assert _call(L, poses, [(0, 1, Zn, np.eye(6))], opt) == INV
    On = np.eye(6)
    On[2, 2] = np.inf
    assert _call(L, poses, [(0, 1, np.eye(4), On)], opt) == INV
    Pn = [np.eye(4), np.full((4, 4), np.nan)]
    assert _call(L, Pn, [good], opt) == INV
    Oa = np.eye(6)
    Oa[0, 1] = 1e-3
    assert _call(L, poses, [(0, 1, np.eye(4), Oa)], opt) == INV
    Os = np.eye(6) * 100.0
    Os[0, 1], Os[1, 0] = 1.0, 1.0 + 1e-12  # symmetric to 1e-9 relative: accepted
    bad_opt = graph.default_options("dogleg")
    bad_opt.algorithm = 7
    assert _call(L, poses, [good], bad_opt) == INV
    if L.dvo_amd_device_count() > 0:
        return
    # valid arguments without a GPU: no device (and no CPU path)
    assert _call(L, poses, [good], opt) == 2
    assert _call(L, poses, [(0, 1, np.eye(4), Os)], opt) == 2
    d = C.c_double()
    assert L.dvo_amd_debug_graph_timing(None, C.byref(d), None, None, None) == 2
    P = np.ascontiguousarray(np.stack([T.T for T in poses]))
    assert L.dvo_amd_debug_graph_system(None, 2, P.ctypes.data_as(C.POINTER(C.c_double)), None, 1, _c_edges([good]), 5.0,
                                        None, None, None, None, None, None) == 2


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trk():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi.DenseTracker()


def _block_rel(A, B, bs=6):
    """max over 6x6 blocks of max|A - B| / max|B| (0 / 0 = 0; a nonzero difference on a zero block = inf)"""
    worst = 0.0
    for i in range(0, A.shape[0], bs):
        for j in range(0, A.shape[1] if A.ndim == 2 else 1, bs):
            a = A[i:i + bs, j:j + bs] if A.ndim == 2 else A[i:i + bs]
            b = B[i:i + bs, j:j + bs] if B.ndim == 2 else B[i:i + bs]
            d, s = np.max(np.abs(a - b)), np.max(np.abs(b))
            worst = max(worst, 0.0 if d == 0 else (d / s if s > 0 else np.inf))
    return worst


@pytest.mark.gpu
def test_gpu_first_system_and_one_step_match_restatement(trk):
    g, _ = R.ring_graph(574, n_chords=20, star=8, seed=11, noise=1e-3, drift=0.01)  # 573 free vertices
    H, b, x, F, fp = to_pose_graph(g).debug_system(trk, 5.0)
    Hr, br, Fr, _, _ = R.linearise(g, 5.0)
    assert H.shape == Hr.shape == (3438, 3438)
    assert _block_rel(H, Hr) <= 1e-12
    assert _block_rel(b, br) <= 1e-12
    assert abs(F - Fr) <= 1e-12 * abs(Fr)
    assert fp < 0
    xr = np.linalg.solve(Hr, br)
    assert np.linalg.norm(x - xr) <= 1e-9 * np.linalg.norm(xr), np.linalg.norm(x - xr) / np.linalg.norm(xr)


def _compare(res, o, g, F0):
    """library result vs restatement run that followed it; returns the adjudicated trials"""
    rec, rr = res.iterations, o["records"]
    floor = 1e-20 * max(F0, 1.0)  # the rounding floor of F on these consistent graphs
    for t in o["adjudicated"]:
        # a gain ratio within the margin of a threshold: the restatement decided the same way on its own, or F and F' both
        # sit at the rounding floor, where the two fp64 implementations cannot tell a step from no step
        own = bool(t["rho"] > 0)
        assert own == t["decided"] or max(t["F"], t["Fp"]) <= floor, ("a contested decision above the rounding floor", t)
    assert res.n_iterations == o["iterations"]
    assert res.termination == o["termination"]
    assert np.array_equal(rec["trials"], rr["trials"]) and np.array_equal(rec["accepted"], rr["accepted"])
    # F of two fp64 implementations whose solves round differently: 1e-10 relative, and absolutely 1e-12 of the starting F
    # (these graphs are consistent, F falls towards 0, and the pose rounding alone moves F by ~1e-15 near the optimum)
    f_abs = 1e-12 * max(F0, 1.0)
    assert np.all(np.abs(rec["objective"] - rr["objective"]) <= 1e-10 * np.abs(rr["objective"]) + f_abs)
    before = np.r_[F0, rr["objective"][:-1]]
    live = before > f_abs
    assert np.allclose(rec["lambda"][live], rr["lambda"][live], rtol=1e-8, atol=0)
    assert np.allclose(rec["delta"][live], rr["delta"][live], rtol=1e-8, atol=0)
    assert np.allclose(rec["step_norm"][live], rr["step_norm"][live], rtol=1e-6, atol=1e-12)
    assert abs(res.final_objective - o["F_final"]) <= 1e-10 * abs(o["F_final"]) + f_abs
    for v in range(len(g.poses)):
        A, B = res.poses[v], o["poses"][v]
        assert np.max(np.abs(A[:3, 3] - B[:3, 3])) <= 1e-9, v
        assert rotation_angle(A, B) <= 1e-9, v
    return o["adjudicated"]


@pytest.mark.gpu
@pytest.mark.parametrize("m", [30, 200, 573])
@pytest.mark.parametrize("algorithm", ["levenberg", "dogleg"])
def test_gpu_full_optimization_matches_restatement(trk, m, algorithm):
    g, truth = R.ring_graph(m + 1, n_chords=max(4, m // 30), star=8, seed=100 + m, drift=0.02)  # m free vertices
    iters = 50 if algorithm == "levenberg" else 200
    res = to_pose_graph(g).optimize(trk, algorithm, iterations=iters)
    o = R.optimize(g, algorithm, iterations=iters, follow=res.iterations, margin=MARGIN)
    adj = _compare(res, o, g, o["F0"])
    assert res.final_objective < 1e-10 * res.initial_objective
    print(f"m={m} {algorithm}: {res.n_iterations} iterations, {res.termination}, F {res.initial_objective:.3e} -> "
          f"{res.final_objective:.3e}, {len(adj)} trials at the rounding floor adjudicated")


def accuracy_graph():
    """A ring of 200 true poses: odometry edges carry an injected drift (a constant bias per step plus noise) and the
    information of that uncertainty; the chords are the true relative poses with 1e-3 noise and the information of it.
    The initial estimate chains the odometry.  Returns (Graph, truth)."""
    g, truth = R.ring_graph(200, n_chords=30, seed=21, drift=0.0, noise=0.0)
    rng = np.random.default_rng(4)
    bias = np.array([0.004, 0.0, 0.0, 0.0, 0.0, 0.002])
    odo_info = np.diag([1.0 / 0.01 ** 2] * 3 + [1.0 / 0.005 ** 2] * 3)
    edges = []
    for f, t, Z, _ in g.edges:
        if t == f + 1:
            edges.append((f, t, Z @ _exp(bias + rng.normal(scale=1e-3, size=6)), odo_info))
        else:
            edges.append((f, t, Z @ _exp(rng.normal(scale=1e-3, size=6)), np.eye(6) / 1e-3 ** 2))
    poses = [truth[0]]
    for f, t, Z, _ in edges:
        if t == f + 1:
            poses.append(poses[-1] @ Z)
    return R.Graph(poses, g.fixed, edges), truth


@pytest.mark.gpu
def test_gpu_accuracy_against_truth(trk):
    g, truth = accuracy_graph()
    res = to_pose_graph(g).optimize(trk, "dogleg", iterations=100)
    before, after = R.rms_position(g.poses, truth), R.rms_position(res.poses, truth)
    print(f"RMS position error: drifted {before:.4f} m -> optimized {after:.5f} m")
    assert after * 10 <= before


def _non_pd_graph():
    g, truth = R.ring_graph(30, n_chords=4, seed=31, drift=0.02)
    extra = truth[5] @ _exp([0.3, 0.1, 0.0, 0.0, 0.0, 0.2])
    O = np.diag([400.0, 400.0, 400.0, 0.0, 0.0, 0.0])  # no information on rotation: zero rows / columns of H
    edges = g.edges + [(5, 30, R.inverse(truth[5]) @ extra, O)]
    return R.Graph(g.poses + [extra @ _exp([0.05, 0.0, 0.0, 0.0, 0.0, 0.0])], g.fixed + [False], edges)


@pytest.mark.gpu
def test_gpu_non_positive_definite_system(trk):
    g = _non_pd_graph()
    H, b, x, F, fp = to_pose_graph(g).debug_system(trk, 5.0)
    s = g.slot[30]
    assert np.all(np.diag(H)[6 * s + 3:6 * s + 6] == 0.0) and x is None and fp >= 0
    res = to_pose_graph(g).optimize(trk, "dogleg", iterations=100)
    o = R.optimize(g, "dogleg", iterations=100, follow=res.iterations, margin=MARGIN)
    assert res.cholesky_failures >= 1 and o["cholesky_failures"] >= 1
    assert res.final_objective < res.initial_objective
    _compare(res, o, g, o["F0"])
    assert np.array_equal(res.iterations["lambda"], o["records"]["lambda"]), "lambda sequence"
    assert res.lambda_ == o["lambda"]
    lev = to_pose_graph(g).optimize(trk, "levenberg", iterations=50)
    assert lev.final_objective < 1e-10 * lev.initial_objective and lev.termination != "fail"


@pytest.mark.gpu
def test_gpu_fixed_and_inactive_vertices_unchanged(trk):
    g, _ = R.ring_graph(40, n_chords=5, seed=41, drift=0.02)
    pg = to_pose_graph(g)
    pg.set_fixed(7)
    lone = pg.add_vertex(_exp([1.0, 2.0, 3.0, 0.1, 0.2, 0.3]) + 1e-17)  # touched by no edge
    before = [P.copy() for P in pg.poses]
    res = pg.optimize(trk, "levenberg")
    for v in (0, 7, lone):
        assert res.poses[v].tobytes() == before[v].tobytes(), v
    assert res.n_free == 38
    assert not np.array_equal(res.poses[3], before[3])


@pytest.mark.gpu
def test_gpu_deterministic_across_runs_and_contexts(trk):
    from dvo_slam_amd import capi

    g, _ = R.ring_graph(200, n_chords=10, seed=51, noise=1e-3, drift=0.02)
    other = capi.DenseTracker()
    outs = []
    for t in (trk, trk, other):
        res = to_pose_graph(g).optimize(t, "dogleg", iterations=50)
        outs.append((np.stack(res.poses).tobytes(), res.weight.tobytes(), res.chi2.tobytes(),
                     b"".join(v.tobytes() for v in res.iterations.values())))
    assert outs[0] == outs[1] == outs[2]


@pytest.mark.gpu
def test_gpu_capacity(trk):
    from dvo_slam_amd import capi, graph

    m = 1025
    pg = graph.PoseGraph()
    pg.add_vertex(fixed=True)
    for i in range(m):
        pg.add_vertex(_exp([0.1 * (i + 1), 0, 0, 0, 0, 0]))
        pg.add_edge(i, i + 1, _exp([0.1, 0, 0, 0, 0, 0]), np.eye(6))
    before = [P.copy() for P in pg.poses]
    with pytest.raises(capi.DvoAmdError) as ei:
        pg.optimize(trk, "dogleg")
    assert ei.value.status == 7
    assert all(np.array_equal(a, b) for a, b in zip(pg.poses, before))


@pytest.mark.gpu
def test_gpu_loop_closure_end_to_end(trk, synth):
    from dvo_slam_amd import capi, constraints as Cn, graph
    import validator_scenario as S

    key, cands = S.gpu_keyframes(capi, Cn, synth, 640, 480, 6)
    # the true candidates (the decoys' rejection is tests/test_validator.py's subject), permissive thresholds as there
    cands = [c for c in cands if c.id < 60]
    val = Cn.createConstraintProposalValidator(min_constraint_ratio=0.0, ratio_coarse=-1e300, ratio_fine=-1e300)
    survivors = val.validate(Cn.proposalsForCandidates(key, cands))
    assert survivors
    pg = graph.PoseGraph()
    vid = {key.id: pg.add_vertex(key.pose, fixed=True)}
    for c in cands:
        vid[c.id] = pg.add_vertex(c.pose)
    pg.add_constraints(survivors, vid)
    by_vertex = {vid[c.id]: c for c in cands}
    moved = sorted({v for f, t, _, _ in pg.edges for v in (f, t) if v in by_vertex})
    assert moved
    res = pg.optimize(trk, "dogleg")
    truth = [by_vertex[v].pose_true for v in moved]
    before = R.rms_position([by_vertex[v].pose for v in moved], truth)
    after = R.rms_position([res.poses[v] for v in moved], truth)
    print(f"loop closure: {len(survivors)} constraints over {len(moved)} keyframes, RMS {before:.4f} -> {after:.5f} m")
    assert after < before


def _result_arrays(res):
    stats = [res.n_iterations, res.n_free, res.cholesky_failures, res.initial_objective, res.final_objective, res.lambda_,
             res.delta]
    return ([np.stack(res.poses), res.chi2, res.weight, np.array(stats, dtype=np.float64)] +
            [np.asarray(v) for v in res.iterations.values()] + [np.frombuffer(res.termination.encode(), dtype=np.uint8)])


def _marginal_arrays(out):
    blocks, st = out
    return [blocks, np.array([st.n_free, st.factorized, st.fixed_blocks, st.inactive_blocks, st.solved_columns])]


def workspace_reuse_calls():
    """The calls of test_gpu_workspace_reuse_across_entries_bit_for_bit, in order: (name, f(tracker) -> list of arrays).  Between
    them they reach every buffer group of a context's graph workspaces: the dense H / L, the sparse fronts, Zinv / cols, the
    batch workspace; call 6 is smaller than call 1, so a stale tail of a buffer would show."""
    from dvo_slam_amd import graph

    ring40 = R.ring_graph(41, n_chords=4, seed=61, drift=0.02)[0]  # 40 free vertices
    ring12 = R.ring_graph(13, n_chords=2, seed=62, drift=0.02)[0]
    trio = [R.ring_graph(16, n_chords=2, seed=63 + i, drift=0.02)[0] for i in range(3)]  # 15 free vertices each
    # an adjacent pair, a diagonal, and two vertices far apart on the ring that share no edge (the sparse column path)
    pairs = [(3, 4), (9, 9), (5, 25)]

    def batch(t):
        pgs = [to_pose_graph(g) for g in trio]
        out = []
        for i, res in enumerate(graph.optimize_batch(t, pgs, "levenberg", iterations=20)):
            out += _result_arrays(res) + [np.asarray(v) for v in graph.debug_batch_records(t, i).values()]
        return out

    def all_fixed(t):
        pg = to_pose_graph(ring12)
        for v in range(len(pg.poses)):
            pg.set_fixed(v)
        return _result_arrays(pg.optimize(t, "levenberg", iterations=5, solver="sparse"))

    return [
        ("dense levenberg, 40 free", lambda t: _result_arrays(to_pose_graph(ring40).optimize(t, "levenberg", iterations=20))),
        ("sparse dogleg, 40 free",
         lambda t: _result_arrays(to_pose_graph(ring40).optimize(t, "dogleg", iterations=40, solver="sparse"))),
        ("sparse marginals", lambda t: _marginal_arrays(to_pose_graph(ring40).marginals(t, pairs, solver="sparse"))),
        ("dense marginals, 12 free", lambda t: _marginal_arrays(to_pose_graph(ring12).marginals(t, solver="dense"))),
        ("batch of three", batch),
        ("dense levenberg, 12 free", lambda t: _result_arrays(to_pose_graph(ring12).optimize(t, "levenberg", iterations=20))),
        ("sparse levenberg, no free vertex", all_fixed),
    ]


@pytest.mark.gpu
def test_gpu_workspace_reuse_across_entries_bit_for_bit(trk):
    """Every graph entry in turn on one context gives the bits each gives on a fresh context of its own: nothing a call leaves
    in the shared workspace (grown buffers, stale tails, the sparse maps, the inverse's arena) reaches the next call."""
    from dvo_slam_amd import capi

    shared = capi.DenseTracker()
    for name, call in workspace_reuse_calls():
        got, want = call(shared), call(capi.DenseTracker())
        assert len(got) == len(want)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.dtype == b.dtype and a.shape == b.shape, (name, k)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, k)  # the raw bits: NaN blocks compare too
        if name == "sparse marginals":
            assert got[1][4] > 0, "the far-apart pair takes the column path"
