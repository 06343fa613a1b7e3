"""The edge geometry of the pose-graph kernels where outlier edges take it (dvo_slam_amd/csrc/dvo_graph_device.h): the three
trace <= 0 branches of quaternion() and its sign flip, the identity branch of increment(), the Cauchy kernel far below weight 1
and without a kernel, and the Jacobians away from the identity -- through k_linearise and both assemblies (dense, sparse),
k_optimize_batch and k_update, against the 60-digit mpmath reference of tests/pose_graph_geometry_cases.py.

The bars are the suite's own: 1e-12 block-relative on H and b and 1e-12 relative on F
(test_pose_graph.py::test_gpu_first_system_and_one_step_match_restatement), 1e-9 m and 1e-9 rad on poses (_compare), the
chi2 / weight bound of test_pose_graph_batch.py::_bars.  Every GPU test prints the worst deviation it met next to its bar.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_geometry_cases as G  # noqa: E402
import pose_graph_restatement as R  # noqa: E402
from test_pose_graph import MARGIN, _block_rel, rotation_angle, to_pose_graph  # noqa: E402
from test_pose_graph_batch import _check_one  # noqa: E402
from test_pose_graph_sparse import _H_from_blocks  # noqa: E402

POSE_BAR = 1e-9
MARGIN_STEP = 1e-9   # |1 - |x_rot|^2| of the reference at least this far from 0: the branch of inc() cannot turn by rounding


# ---- CPU: the reference, the family -------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_float64_restatement():
    """The mpmath reference and pose_graph_restatement state the same formulas independently: on every case of the family the
    float64 restatement is within rounding of the reference -- the error a few hundred ulp, the five products and rho0 within
    the bar the kernels are held to -- takes the same quaternion branch, and inc() takes the same branch on the same step."""
    fam = G.family()
    worst_e, worst_blk, worst_F = 0.0, 0.0, 0.0
    for c in fam["cases"]:
        ref = c["ref"]
        e = R.edge_error(c["Xf"], c["Xt"], c["Z"])
        # Delta chains three isometries with translations under 10 m: some tens of roundings of eps * 10 m on t, of eps on
        # the entries of R; Shepperd's square root is taken of a number >= 1, so q inherits the error of R: 1e-13 covers both
        worst_e = max(worst_e, float(np.max(np.abs(e - G._np(ref["e"])))))
        if c["strict"]:
            m = R.edge_delta(c["Xf"], c["Xt"], c["Z"])[:3, :3]
            tr = m[0, 0] + m[1, 1] + m[2, 2]
            i = int(np.argmax(np.diag(m)))
            w_raw = m[(i + 2) % 3, (i + 1) % 3] - m[(i + 1) % 3, (i + 2) % 3]
            cls = "tr>0" if tr > 0 else "i%d%s" % (i, "+" if w_raw >= 0 else "-")
            assert cls == c["cls"], (cls, c["cls"])
        for delta in G.DELTAS:
            a, b = G.restatement_blocks(c, delta), G.blocks(c, delta)
            worst_blk = max([worst_blk] + [G.rel(x, y) for x, y in zip(a[:5], b[:5])])
            assert abs(a[6] - b[6]) <= G.BAR * b[6]
            if b[5] != 0:
                worst_F = max(worst_F, abs(a[5] - b[5]) / abs(b[5]))
    print(f"restatement vs reference over {len(fam['cases'])} cases: |e - e_ref| {worst_e:.2e} (1e-13), products "
          f"{worst_blk:.2e} block-relative ({G.BAR:.0e}), rho0 {worst_F:.2e} relative ({G.BAR:.0e})")
    assert worst_e <= 1e-13 and worst_blk <= G.BAR and worst_F <= G.BAR
    for delta, moved in ((5.0, "to"), (0.0, "from")):
        for c, s in zip(fam["cases"], G.steps(delta, moved)):
            if abs(s["w2"]) < MARGIN_STEP:
                continue
            T = R.inc(s["x"])
            assert (1.0 - float(s["x"][3:] @ s["x"][3:]) < 0.0) == (s["w2"] < 0)
            assert np.array_equal(T[:3, :3], np.eye(3)) or s["w2"] > 0
            X = c["Xt"] if moved == "to" else c["Xf"]
            assert np.max(np.abs(X @ T - s["pose"])) <= 1e-13 * max(1.0, float(np.max(np.abs(s["pose"]))))


def test_family_census_and_margins():
    fam = G.family()
    cases, dropped = fam["cases"], fam["dropped"]
    cen = G.census(cases)
    ties = [c for c in cases if not c["strict"]]
    print(f"{fam['generated']} cases generated, {len(dropped)} dropped, {len(ties)} near a tie; strict cases per class: {cen}")
    for c, why in dropped:
        print("  dropped:", c["origin"], "angle %.9f" % c["angle"], why)
    assert set(cen) == set(G.CLASSES) and all(n >= 8 for n in cen.values()), cen
    assert len(dropped) <= 0.05 * fam["generated"]
    assert len(cases) + len(dropped) == fam["generated"] and 2 * len(cases) <= 1024
    for c in cases:
        ref = c["ref"]
        assert c["strict"] == (float(ref["margin"]) >= G.MARGIN_CLASS)
        assert c["cls"] == "tr>0" or float(ref["w_raw"]) >= G.MARGIN_CLASS
    # the grid: exactly consistent edges have e = 0 and chi2 = 0 exactly; the near-tie group is the body diagonals past 120
    # degrees, where the three diagonal entries of Delta are equal up to rounding
    exact = [c for c in cases if c["angle"] == 0.0]
    assert len(exact) >= 8 and all(c["ref"]["chi2"] == 0 and all(x == 0 for x in c["ref"]["e"]) for c in exact)
    assert ties and all(c["origin"] == "grid" and c["cls"] != "tr>0" for c in ties)
    grid = {c["angle"] for c in cases if c["origin"] == "grid"}
    assert grid == set(float(a) for a in G.GRID_ANGLES)
    # condition numbers of the information matrices
    assert max(np.linalg.cond(c["O"]) for c in cases) <= 1e4
    # both branches of inc() among the accepted steps of every batch run
    for delta in G.DELTAS:
        for moved in ("to", "from"):
            ident, rot = _inc_census(cases, G.steps(delta, moved))
            print(f"  delta {delta} moved {moved}: accepted steps with the identity rotation {ident}, with a rotation {rot}")
            assert ident >= 8 and rot >= 8


def _inc_census(cases, steps):
    ok = [s for c, s in zip(cases, steps) if c["strict"] and s["accepted"] and abs(s["rho"]) >= MARGIN]
    return sum(1 for s in ok if s["w2"] < -MARGIN_STEP), sum(1 for s in ok if s["w2"] > MARGIN_STEP)


def test_block_rel_vectorised_is_the_suites_block_rel():
    rng = np.random.default_rng(2)
    B = rng.normal(size=(24, 24))
    B[6:12, 12:18] = 0.0
    A = B + 1e-13 * rng.normal(size=B.shape)
    A[6:12, 12:18] = 0.0
    assert G.block_rel(A, B) == _block_rel(A, B) and G.block_rel(A[0], B[0]) == _block_rel(A[0], B[0])
    A[7, 13] = 1e-300
    assert G.block_rel(A, B) == _block_rel(A, B) == np.inf


def _check_flipped_loops(weight, poses, g, truth, clean_poses):
    assert np.all(weight[-3:] < 0.05), weight[-3:]
    assert np.all(weight[:-3] > 0.9), float(np.min(weight[:-3]))
    assert R.rms_position(poses, truth) <= 2.0 * R.rms_position(clean_poses, truth)


@pytest.mark.parametrize("m", [40, 30])
def test_restatement_flipped_loop_closures_are_down_weighted(m):
    g, truth = G.flipped_loop_graph(m)
    clean, _ = G.flipped_loop_graph(m, planted=False)
    assert len(g.edges) == len(clean.edges) + 3
    for k in range(3):  # the planted edges sit in the trace <= 0 branches at the start, one per largest diagonal
        f, t, Z, O = g.edges[-3 + k]
        ref = G.edge(g.poses[f], g.poses[t], Z, O)
        assert ref["cls"][:2] == "i%d" % k, ref["cls"]
    o = R.optimize(g, "dogleg", iterations=200)
    _check_flipped_loops(o["rho1"], o["poses"], g, truth, R.optimize(clean, "dogleg", iterations=200)["poses"])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trk():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi.DenseTracker()


def disjoint_graph(cases, fixed):
    """2K vertices, edge k from 2k to 2k + 1; fixed: "none", "from" or "to" """
    poses, fx, edges = [], [], []
    for k, c in enumerate(cases):
        poses += [c["Xf"], c["Xt"]]
        fx += [fixed == "from", fixed == "to"]
        edges.append((2 * k, 2 * k + 1, c["Z"], c["O"]))
    return R.Graph(poses, fx, edges)


def reference_system(cases, delta, fixed):
    """(H, b, F) of disjoint_graph in float64, every entry the reference's value rounded once"""
    per = 2 if fixed == "none" else 1
    n = 6 * per * len(cases)
    H, b, rho0 = np.zeros((n, n)), np.zeros(n), []
    for k, c in enumerate(cases):
        Aff, Att, Aft, gf, gt, r0, _ = G.blocks(c, delta)
        o = 6 * per * k
        if fixed == "none":
            H[o:o + 6, o:o + 6], H[o + 6:o + 12, o + 6:o + 12] = Aff, Att
            H[o:o + 6, o + 6:o + 12], H[o + 6:o + 12, o:o + 6] = Aft, Aft.T
            b[o:o + 6], b[o + 6:o + 12] = gf, gt
        elif fixed == "from":
            H[o:o + 6, o:o + 6], b[o:o + 6] = Att, gt
        else:
            H[o:o + 6, o:o + 6], b[o:o + 6] = Aff, gf
        rho0.append(r0)
    return H, b, math.fsum(rho0)


def _system_against_reference(name, cases, delta, fixed, H, b, F, fp):
    Hr, br, Fr = reference_system(cases, delta, fixed)
    assert H.shape == Hr.shape
    dH, db, dF = G.block_rel(H, Hr), G.block_rel(b, br), abs(F - Fr) / abs(Fr)
    print(f"{name} delta {delta} fixed {fixed}: H {dH:.2e}, b {db:.2e} block-relative ({G.BAR:.0e}), F {dF:.2e} relative "
          f"({G.BAR:.0e}); classes through k_linearise: {_all_census(cases)}")
    assert dH <= G.BAR and db <= G.BAR and dF <= G.BAR
    # all free: every edge's 12 x 12 block has rank 6 (the gauge), H is singular and x is not valid
    assert fp >= 0 if fixed == "none" else fp < 0


def _all_census(cases):
    return {k: sum(1 for c in cases if c["cls"] == k) for k in G.CLASSES}


@pytest.mark.gpu
@pytest.mark.parametrize("delta", G.DELTAS)
def test_gpu_first_system_dense_matches_reference(trk, delta):
    cases = G.family()["cases"]
    for fixed in ("none", "from", "to"):
        H, b, _, F, fp = to_pose_graph(disjoint_graph(cases, fixed)).debug_system(trk, delta)
        _system_against_reference("dense", cases, delta, fixed, H, b, F, fp)


@pytest.mark.gpu
@pytest.mark.parametrize("delta", G.DELTAS)
def test_gpu_first_system_sparse_matches_reference_and_dense_bits(trk, delta):
    cases = G.family()["cases"]
    for fixed in ("none", "from", "to"):
        pg = to_pose_graph(disjoint_graph(cases, fixed))
        H, b, _, F, fp = pg.debug_system(trk, delta)
        rc, blocks, bs, _, Fs, fps = pg.debug_system_sparse(trk, delta)
        assert len(rc) == len({(int(r), int(c)) for r, c in rc})
        Hs = _H_from_blocks(rc, blocks, H.shape[0] // 6)
        _system_against_reference("sparse", cases, delta, fixed, Hs, bs, Fs, fps)
        assert Hs.tobytes() == H.tobytes() and bs.tobytes() == b.tobytes() and Fs == F


def _two_vertex_graphs(cases, moved):
    return [R.Graph([c["Xf"], c["Xt"]], [moved == "to", moved == "from"], [(0, 1, c["Z"], c["O"])]) for c in cases]


def _run_batch(trk, cases, delta, moved):
    from dvo_slam_amd import graph

    res = graph.optimize_batch(trk, [to_pose_graph(g) for g in _two_vertex_graphs(cases, moved)], algorithm="levenberg",
                               iterations=1, max_trials=1, initial_lambda=G.LAMBDA, robust_delta=delta)
    for i, r in enumerate(res):
        r.iterations = graph.debug_batch_records(trk, i)
    return res


def _pose_dev(A, B):
    return float(np.max(np.abs(A[:3, 3] - B[:3, 3]))), rotation_angle(A, B)


@pytest.mark.gpu
@pytest.mark.parametrize("moved", ["to", "from"])
@pytest.mark.parametrize("delta", G.DELTAS)
def test_gpu_batch_one_trial_matches_reference(trk, delta, moved):
    cases = G.family()["cases"]
    steps = G.steps(delta, moved)
    ident, rot = _inc_census(cases, steps)
    assert ident >= 8 and rot >= 8
    res = _run_batch(trk, cases, delta, moved)
    worst = dict(F=0.0, t=0.0, angle=0.0, chi2=0.0, weight=0.0)
    seen = {k: 0 for k in G.CLASSES}
    n_id = n_rot = 0
    for c, s, r in zip(cases, steps, res):
        f_abs = 1e-12 * max(s["F0"], 1.0)
        assert abs(r.initial_objective - s["F0"]) <= 1e-12 * abs(s["F0"]) + f_abs
        if s["F0"] > 0:
            worst["F"] = max(worst["F"], abs(r.initial_objective - s["F0"]) / s["F0"])
        assert (r.n_iterations, r.n_free, r.termination) == (1, 1, "terminate")
        fixed_v, moved_v = (0, 1) if moved == "to" else (1, 0)
        before = (c["Xf"], c["Xt"])
        assert r.poses[fixed_v].tobytes() == before[fixed_v].tobytes()
        if not c["strict"] or abs(s["rho"]) < MARGIN:
            continue  # near a tie of quaternion()'s branches: F alone; a gain ratio at 0: either decision is right
        assert int(r.iterations["accepted"][0]) == int(s["accepted"]), (c["cls"], s["rho"])
        if s["accepted"]:
            assert r.final_objective < r.initial_objective
        if abs(s["w2"]) < MARGIN_STEP:
            continue
        seen[c["cls"]] += 1
        n_id += bool(s["accepted"] and s["w2"] < 0)
        n_rot += bool(s["accepted"] and s["w2"] > 0)
        want = s["pose"] if s["accepted"] else before[moved_v]
        dt, da = _pose_dev(r.poses[moved_v], want)
        worst["t"], worst["angle"] = max(worst["t"], dt), max(worst["angle"], da)
        assert dt <= POSE_BAR and da <= POSE_BAR, (c["cls"], s["w2"], dt, da)
        # test_pose_graph_batch.py::_bars: |de| <= 2e-8 between two estimates within the pose bars (edges under 7 m);
        # rho1 = 1 / (1 + chi2 / delta^2) moves by at most |d chi2| / delta^2, and is 1 without a kernel
        chi2, rho1 = (s["chi2"], s["rho1"]) if s["accepted"] else (float(c["ref"]["chi2"]), G.blocks(c, delta)[6])
        lmax, de = float(np.linalg.eigvalsh(c["O"])[-1]), 2e-8
        bound = 2.0 * np.sqrt(abs(chi2) * lmax) * de + lmax * de * de + f_abs
        worst["chi2"] = max(worst["chi2"], abs(r.chi2[0] - chi2) / bound)
        assert abs(r.chi2[0] - chi2) <= bound
        if delta > 0:
            worst["weight"] = max(worst["weight"], abs(r.weight[0] - rho1) / (bound / delta ** 2))
            assert abs(r.weight[0] - rho1) <= bound / delta ** 2
        else:
            assert r.weight[0] == 1.0
    print(f"batch delta {delta} moved {moved}: F0 {worst['F']:.2e} relative (1e-12), pose {worst['t']:.2e} m / "
          f"{worst['angle']:.2e} rad ({POSE_BAR:.0e}), chi2 {worst['chi2']:.2e} and weight {worst['weight']:.2e} of their "
          f"bounds; classes through k_optimize_batch: {seen}; accepted with the identity rotation {n_id}, with a rotation "
          f"{n_rot}")
    assert all(n >= 8 for n in seen.values()) and n_id >= 8 and n_rot >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("delta", G.DELTAS)
def test_gpu_single_entry_update_matches_reference_and_batch(trk, delta):
    """One Levenberg trial of the disjoint graph with every from-vertex fixed (H = the Att blocks, positive definite).  The
    single entry decides for the whole graph: rho = (sum F - sum F') / (1e-3 + sum of the edges' gains)."""
    cases = G.family()["cases"]
    steps = G.steps(delta, "to")
    rho = math.fsum(s["F0"] - s["Fp"] for s in steps) / (1e-3 + math.fsum(s["gain"] for s in steps))
    assert rho >= MARGIN, "the reference keeps this step, clear of the threshold"
    g = disjoint_graph(cases, "from")
    res = to_pose_graph(g).optimize(trk, "levenberg", iterations=1, max_trials=1, initial_lambda=G.LAMBDA, robust_delta=delta)
    assert int(res.iterations["accepted"][0]) == 1 and res.n_free == len(cases)
    F0 = math.fsum(s["F0"] for s in steps)
    assert abs(res.initial_objective - F0) <= 1e-12 * F0
    batch = _run_batch(trk, cases, delta, "to")
    worst = dict(t=0.0, angle=0.0, batch=0.0)
    seen = {k: 0 for k in G.CLASSES}
    n_id = n_rot = 0
    for k, (c, s, rb) in enumerate(zip(cases, steps, batch)):
        assert res.poses[2 * k].tobytes() == c["Xf"].tobytes()
        if not c["strict"] or abs(s["w2"]) < MARGIN_STEP:
            continue
        seen[c["cls"]] += 1
        n_id += s["w2"] < 0
        n_rot += s["w2"] > 0
        dt, da = _pose_dev(res.poses[2 * k + 1], s["pose"])
        worst["t"], worst["angle"] = max(worst["t"], dt), max(worst["angle"], da)
        assert dt <= POSE_BAR and da <= POSE_BAR, (c["cls"], s["w2"], dt, da)
        if int(rb.iterations["accepted"][0]):
            d = float(np.max(np.abs(res.poses[2 * k + 1] - rb.poses[1])))
            worst["batch"] = max(worst["batch"], d)
            assert d <= 1e-12, (c["cls"], d)
    print(f"single entry delta {delta}: pose {worst['t']:.2e} m / {worst['angle']:.2e} rad ({POSE_BAR:.0e}), against the batch "
          f"kernel {worst['batch']:.2e} (1e-12); classes through k_update: {seen}; identity rotation {n_id}, rotation {n_rot}")
    assert all(n >= 8 for n in seen.values()) and n_id >= 8 and n_rot >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dense", "sparse", "batch"])
def test_gpu_flipped_loop_closures_full_optimization(trk, variant):
    from dvo_slam_amd import graph

    m = 30 if variant == "batch" else 40
    g, truth = G.flipped_loop_graph(m)
    clean, _ = G.flipped_loop_graph(m, planted=False)
    if variant == "batch":
        res, res0 = graph.optimize_batch(trk, [to_pose_graph(g), to_pose_graph(clean)], algorithm="dogleg", iterations=200)
        res.iterations = graph.debug_batch_records(trk, 0)
    else:
        res = to_pose_graph(g).optimize(trk, "dogleg", iterations=200, solver=variant)
        res0 = to_pose_graph(clean).optimize(trk, "dogleg", iterations=200, solver=variant)
    # the measurements carry noise, F converges to a positive value: the restatement follows as in test_pose_graph_batch.py
    _check_one(res, g, "dogleg", 200, consistent=False)
    _check_flipped_loops(res.weight, res.poses, g, truth, res0.poses)
