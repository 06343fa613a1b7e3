"""Many small pose graphs in one call (dvo_amd_optimize_graphs_batch, dvo_slam_amd.graph.optimize_batch): the header, the
argument checks and the example on the CPU; on the GPU every graph of a batch against the float64 restatement
(tests/pose_graph_restatement.py) and against the single-graph entry, and the batch-invariance rule bit for bit.

The bars are the ones tests/test_pose_graph.py::_compare applies between the dense GPU path and the restatement: objective
1e-10 relative + 1e-12 F0, final poses 1e-9 in translation and rotation angle, lambda / Delta 1e-8 relative, step norm 1e-6
relative + 1e-12, iterations / termination / trials / accepted equal.  The batch entry returns only stats; the per-iteration
records the bars need (and the restatement's `follow`) come from dvo_amd_debug_graph_batch_records.

Graphs whose measurements are consistent (noise = 0) go through _compare itself.  The local maps have measurement noise, as
real local maps do, so their F converges to a positive value and every Levenberg / dogleg trial after convergence has a gain
ratio of rounding noise (|rho| ~ 1e-13): the restatement follows the library's decision there, exactly as _compare's callers
do, but _compare's extra assertion that such a trial sits below 1e-20 F0 is a statement about consistent graphs (F -> 0) and
does not apply; _bars() below is _compare without that one assertion and with every numeric bar unchanged.  In its place
_against_restatement() requires of every followed decision that differs from the restatement's own that |F - F'| is inside
twice the objective bar.  _margin() derives the band of gain ratios that count as contested for the dogleg on noisy graphs.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_restatement as R  # noqa: E402
import slam_graph  # noqa: E402
from test_pose_graph import (MARGIN, _c_edges, _compare, _exp, _non_pd_graph, _planted_outlier_graph,  # noqa: E402
                             rotation_angle, to_pose_graph)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "dvo_amd_optimize_graphs_batch"
CAP = 32
OK, INVALID, NO_DEVICE, CAPACITY = 0, 1, 2, 7


# ---- graphs -------------------------------------------------------------------------------------------------------------------
def local_maps(n_frames=600, k=15, both_fixed=False, seed=3):
    """slam_graph cut into its local maps: the keyframe (fixed), the k frames after it (the last one is the next keyframe), the
    odometry edges between them and the keyframe's edge to every frame.  both_fixed: the next keyframe is fixed too -- the
    shape KeyframeGraph::optimizeInterKeyframePoses optimizes."""
    g, _, keys = slam_graph.slam_graph(n_frames, k=k, seed=seed, noise=1e-3, drift=0.01)
    maps = []
    for kf in keys:
        last = min(kf + k, n_frames - 1)
        if last - kf < 2:
            continue
        edges = [(f - kf, t - kf, Z, O) for f, t, Z, O in g.edges
                 if kf <= f < t <= last and (t == f + 1 or f == kf)]
        fixed = [v == 0 or (both_fixed and v == last - kf) for v in range(last - kf + 1)]
        maps.append(R.Graph(g.poses[kf:last + 1], fixed, edges))
    return maps


def chain_graph(m, seed):
    """m free vertices on a ring behind a fixed one, consistent measurements"""
    g, _ = R.ring_graph(m + 1, n_chords=0 if m < 6 else 3, seed=seed, drift=0.02)
    return g


# ---- calls --------------------------------------------------------------------------------------------------------------------
def _items(graphs, with_outputs=True):
    """(items array, the numpy arrays behind it: poses n x 16 column-major, chi2, weight per graph)"""
    from dvo_slam_amd import graph

    items = (graph.CGraphBatchItem * max(len(graphs), 1))()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    keep = []
    for i, g in enumerate(graphs):
        nv, ne = len(g.poses), len(g.edges)
        P = np.ascontiguousarray(np.stack([T.T for T in g.poses])) if nv else np.zeros((1, 4, 4))
        fixed = np.ascontiguousarray(np.asarray(g.fixed, dtype=np.int32)) if nv else np.zeros(1, np.int32)
        ce = _c_edges(g.edges)
        chi2, weight = np.zeros(max(ne, 1)), np.zeros(max(ne, 1))
        items[i].n_vertices, items[i].n_edges = nv, ne
        items[i].poses, items[i].fixed, items[i].edges = P.ctypes.data_as(dp), fixed.ctypes.data_as(ip), ce
        if with_outputs:
            items[i].edge_chi2, items[i].edge_weight = chi2.ctypes.data_as(dp), weight.ctypes.data_as(dp)
        keep.append((P, fixed, ce, chi2, weight))
    return items, keep


def _raw(L, graphs, opt, ctx=None):
    """the raw call: (status, last error, poses arrays after the call, poses arrays before it)"""
    items, keep = _items(graphs)
    before = [k[0].copy() for k in keep]
    rc = L.dvo_amd_optimize_graphs_batch(ctx, len(graphs), items, C.byref(opt))
    return rc, L.dvo_amd_last_error().decode(), [k[0] for k in keep], before


def _untouched(after, before):
    return all(a.tobytes() == b.tobytes() for a, b in zip(after, before))


def _batch(trk, graphs, algorithm, iterations):
    """optimize_batch plus each graph's records (Result.iterations filled in from the debug entry)"""
    from dvo_slam_amd import graph

    res = graph.optimize_batch(trk, [to_pose_graph(g) for g in graphs], algorithm=algorithm, iterations=iterations)
    assert len(res) == len(graphs) and all(len(r.iterations["objective"]) == 0 for r in res)
    for i, r in enumerate(res):
        r.iterations = graph.debug_batch_records(trk, i)
        assert len(r.iterations["objective"]) == r.n_iterations
    return res


def _bars(res, o, g):
    """_compare of tests/test_pose_graph.py without its consistent-graph assertion on adjudicated trials; the bars unchanged"""
    rec, rr, F0 = res.iterations, o["records"], o["F0"]
    assert res.n_iterations == o["iterations"]
    assert res.termination == o["termination"]
    assert res.n_free == len(g.free)
    assert np.array_equal(rec["trials"], rr["trials"]) and np.array_equal(rec["accepted"], rr["accepted"])
    f_abs = 1e-12 * max(F0, 1.0)
    assert np.all(np.abs(rec["objective"] - rr["objective"]) <= 1e-10 * np.abs(rr["objective"]) + f_abs)
    before = np.r_[F0, rr["objective"][:-1]][:len(rr["objective"])]  # (no iteration: nothing to compare)
    live = before > f_abs
    assert np.allclose(rec["lambda"][live], rr["lambda"][live], rtol=1e-8, atol=0)
    assert np.allclose(rec["delta"][live], rr["delta"][live], rtol=1e-8, atol=0)
    assert np.allclose(rec["step_norm"][live], rr["step_norm"][live], rtol=1e-6, atol=1e-12)
    assert abs(res.final_objective - o["F_final"]) <= 1e-10 * abs(o["F_final"]) + f_abs
    assert abs(res.initial_objective - F0) <= 1e-10 * abs(F0) + f_abs
    if rec["lambda"].size and live[-1]:
        assert np.isclose(res.lambda_, o["lambda"], rtol=1e-8, atol=0)
        # stats.delta is 0 for Levenberg (dvo_amd.h); the restatement leaves its unused trust region at its initial value
        assert np.isclose(res.delta, o["delta"], rtol=1e-8, atol=0) if rr["delta"].any() else res.delta == 0.0
    for v in range(len(g.poses)):
        A, B = res.poses[v], o["poses"][v]
        assert np.max(np.abs(A[:3, 3] - B[:3, 3])) <= 1e-9, v
        assert rotation_angle(A, B) <= 1e-9, v
    # chi2 = e^T O e of two estimates within the pose bars: each end of an edge may differ by 1e-9 in translation and 1e-9 rad
    # (the translation part of e moves by the angle times the edge's length, under 7 m in these graphs; its quaternion part
    # by half the angle), so |de| <= 2 (1e-9 + 7e-9 + 0.5e-9) < 2e-8 and |d chi2| <= 2 sqrt(chi2 lmax(O)) |de| + lmax(O) |de|^2;
    # rho1 = 1 / (1 + chi2 / 25) moves by at most |d chi2| / 25
    de = 2e-8
    lmax = np.array([np.linalg.eigvalsh(O)[-1] for _, _, _, O in g.edges])
    bound = 2.0 * np.sqrt(np.abs(o["chi2"]) * lmax) * de + lmax * de * de + f_abs
    assert np.all(np.abs(res.chi2 - o["chi2"]) <= bound)
    assert np.all(np.abs(res.weight - o["rho1"]) <= bound / 25.0)


def _margin(g, algorithm):
    """The band of gain ratios in which the restatement takes the library's decision.  Levenberg's denominator is at least
    1e-3, so the rounding of F - F' stays far inside tests/test_pose_graph.py's MARGIN.  The dogleg clamps |gain| to 1e-12: on a
    graph with measurement noise F stays positive, and once the steps are down to the rounding of F the ratio is
    (rounding of F - F') / 1e-12.  F and F' are sums of len(edges) terms; 64 eps F0 bounds the rounding of their difference,
    so the band is 64 eps F0 / 1e-12 -- but never 0.25 or more, the distance from rho = 1 (the step the model predicts) to the
    nearest threshold: a healthy trial is always decided by the restatement itself."""
    if algorithm == "levenberg":
        return MARGIN
    F0 = R.objective(g.poses, g.edges, 5.0)
    return min(0.2, max(MARGIN, 64.0 * np.finfo(np.float64).eps * F0 / 1e-12))


def _check_one(r, g, algorithm, iterations, consistent, with_compare=True):
    """one graph's result against the restatement that follows its records; returns the restatement's output"""
    o = R.optimize(g, algorithm, iterations=iterations, follow=r.iterations,
                   margin=MARGIN if consistent else _margin(g, algorithm))
    if consistent and with_compare:
        _compare(r, o, g, o["F0"])
    for t in o["adjudicated"]:
        # a decision taken from the library against the restatement's own is one the objective bar cannot tell apart:
        # two implementations within 1e-10 F + 1e-12 F0 of each other on F and on F' may differ on the sign of F - F'
        own = bool(t["rho"] > 0)
        assert own == t["decided"] or abs(t["F"] - t["Fp"]) <= 2.0 * (1e-10 * abs(t["F"]) + 1e-12 * max(o["F0"], 1.0)), t
    _bars(r, o, g)
    return o


def _against_restatement(res, graphs, algorithm, iterations, consistent):
    return sum(len(_check_one(r, g, algorithm, iterations, consistent)["adjudicated"]) for r, g in zip(res, graphs))


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_batch_entry_is_declared_in_the_boundary_header_and_exported(tmp_path):
    from dvo_slam_amd import capi

    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)  # noqa: E731
    boundary = strip(open(os.path.join(ROOT, "include", "dvo_amd.h")).read())
    debug = strip(open(os.path.join(ROOT, "include", "dvo_amd_debug.h")).read())
    assert re.search(r"\b%s\s*\(" % SYMBOL, boundary) and not re.search(r"\b%s\b" % SYMBOL, debug)
    assert re.search(r"#define\s+DVO_AMD_GRAPH_BATCH_MAX_FREE_VERTICES\s+(\d+)", boundary).group(1) == str(CAP)
    assert 16 <= CAP
    assert hasattr(capi.lib(), SYMBOL) and SYMBOL in capi.EXPORTS
    assert capi.lib().dvo_amd_abi_version() == 3
    # the header with the new struct and entry is still plain C99
    src = tmp_path / "use.c"
    src.write_text('#include "dvo_amd.h"\n'
                   "int use(dvo_amd_context *c, dvo_amd_graph_batch_item *it, const dvo_amd_graph_options *o) {\n"
                   "  it[0].stats.iterations = DVO_AMD_GRAPH_BATCH_MAX_FREE_VERTICES;\n"
                   "  return dvo_amd_optimize_graphs_batch(c, 1, it, o);\n}\n")
    res = subprocess.run(["cc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                          str(src), "-c", "-o", str(tmp_path / "use.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def test_local_maps_example_compiles_as_c99(tmp_path):
    res = subprocess.run(["cc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                          os.path.join(ROOT, "examples", "local_maps_example.c"), "-c", "-o", str(tmp_path / "e.o")],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr


def _two_vertex(edge, poses=None):
    poses = [np.eye(4), _exp([0.1, 0, 0, 0, 0, 0.1])] if poses is None else poses
    return R.Graph(poses, [True, False], [edge])


def test_argument_checks_item_by_item_then_no_device():
    from dvo_slam_amd import graph

    L = graph._lib()
    opt = graph.default_options("levenberg")
    good = _two_vertex((0, 1, _exp([0.1, 0, 0, 0, 0, 0.1]), np.eye(6)))
    Zn = np.eye(4)
    Zn[0, 3] = np.nan
    Oa = np.eye(6)
    Oa[0, 1] = 1e-3
    bad = {"vertex index": _two_vertex((0, 2, np.eye(4), np.eye(6))),
           "from == to": _two_vertex((1, 1, np.eye(4), np.eye(6))),
           "non-finite measurement": _two_vertex((0, 1, Zn, np.eye(6))),
           "non-finite pose": _two_vertex((0, 1, np.eye(4), np.eye(6)), [np.eye(4), np.full((4, 4), np.nan)]),
           "not symmetric": _two_vertex((0, 1, np.eye(4), Oa))}
    for why, g in bad.items():
        for at in (0, 2):  # the bad item first and last: every item is checked before any work
            graphs = [good, good, good]
            graphs[at] = g
            rc, err, after, before = _raw(L, graphs, opt)
            assert rc == INVALID, why
            assert SYMBOL in err and "item %d" % at in err and why in err, err
            assert _untouched(after, before)
    # the options: sparse is refused, as is anything the single entry refuses
    sparse = graph.default_options("levenberg")
    sparse.solver = graph.SPARSE
    rc, err, after, before = _raw(L, [good, good], sparse)
    assert rc == INVALID and SYMBOL in err and _untouched(after, before)
    wrong = graph.default_options("dogleg")
    wrong.algorithm = 7
    assert _raw(L, [good], wrong)[0] == INVALID
    assert L.dvo_amd_optimize_graphs_batch(None, 1, None, C.byref(opt)) == INVALID
    assert L.dvo_amd_optimize_graphs_batch(None, -1, None, C.byref(opt)) == INVALID
    # capacity: one item over the cap fails the whole call before the device is looked for; a bad item goes first
    rc, err, after, before = _raw(L, [good, chain_graph(CAP + 1, 1), good], opt)
    assert rc == CAPACITY and "item 1" in err and _untouched(after, before)
    rc, err, after, before = _raw(L, [chain_graph(CAP + 1, 1), bad["from == to"]], opt)
    assert rc == INVALID and "item 1" in err and _untouched(after, before)
    if L.dvo_amd_device_count() > 0:
        return
    # valid arguments without a GPU: no device (and no CPU path)
    rc, err, after, before = _raw(L, [good, chain_graph(CAP, 2)], opt)
    assert rc == NO_DEVICE and _untouched(after, before)
    assert L.dvo_amd_optimize_graphs_batch(None, 0, None, C.byref(opt)) == NO_DEVICE
    assert L.dvo_amd_debug_graph_batch_records(None, 0, 0, None, None) == NO_DEVICE


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trk():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi.DenseTracker()


@pytest.mark.gpu
def test_gpu_local_maps_levenberg_match_restatement(trk):
    maps = local_maps()
    assert len(maps) >= 32 and all(len(g.free) == len(g.poses) - 1 for g in maps)
    res = _batch(trk, maps, "levenberg", 50)
    adj = _against_restatement(res, maps, "levenberg", 50, consistent=False)
    assert all(r.final_objective < r.initial_objective for r in res)
    its = [r.n_iterations for r in res]
    print(f"{len(maps)} local maps, Levenberg: iterations {min(its)}..{max(its)}, {adj} trials adjudicated")


@pytest.mark.gpu
def test_gpu_inter_keyframe_dogleg_match_restatement(trk):
    maps = local_maps(both_fixed=True)
    assert len(maps) >= 32 and all(len(g.free) == len(g.poses) - 2 for g in maps)
    res = _batch(trk, maps, "dogleg", 20)
    adj = _against_restatement(res, maps, "dogleg", 20, consistent=False)
    assert all(r.final_objective < r.initial_objective for r in res)
    its = [r.n_iterations for r in res]
    print(f"{len(maps)} inter-keyframe graphs, dogleg: iterations {min(its)}..{max(its)}, {adj} trials adjudicated")


def _mixed():
    """name -> graph: 1 free vertex ... the cap, and the special items"""
    out = {"m%d" % m: chain_graph(m, 200 + m) for m in (1, 2, 5, 12, 20, CAP)}
    g = chain_graph(4, 11)
    out["no edges"] = R.Graph(g.poses, g.fixed, [])
    out["no free vertex"] = R.Graph(g.poses, [True] * len(g.poses), g.edges)
    lone = _exp([1.0, 2.0, 3.0, 0.1, 0.2, 0.3]) + 1e-17
    g = chain_graph(7, 13)
    out["inactive vertex"] = R.Graph(g.poses + [lone], g.fixed + [False], g.edges)
    out["outlier"] = _planted_outlier_graph()[0]
    out["non pd"] = _non_pd_graph()
    return out


@pytest.mark.gpu
def test_gpu_mixed_sizes_and_special_items(trk):
    mixed = _mixed()
    names, graphs = list(mixed), list(mixed.values())
    assert [len(g.free) for g in graphs][:6] == [1, 2, 5, 12, 20, CAP] and len(mixed["non pd"].free) == 30
    before = [[P.copy() for P in g.poses] for g in graphs]
    res = _batch(trk, graphs, "dogleg", 100)
    by = dict(zip(names, res))
    for name, r, g, b in zip(names, res, graphs, before):
        # "outlier" is the one graph here with measurement noise (see the module's docstring); _compare indexes the first
        # record, which the two items without unknowns do not have
        o = _check_one(r, g, "dogleg", 100, consistent=name != "outlier",
                       with_compare=name not in ("no edges", "no free vertex"))
        assert r.cholesky_failures == o["cholesky_failures"], name
        for v in range(len(g.poses)):  # fixed and inactive vertices come back bit for bit
            if v not in g.slot:
                assert r.poses[v].tobytes() == b[v].tobytes(), (name, v)
    for name in ("no edges", "no free vertex"):
        r = by[name]
        assert (r.n_iterations, r.n_free, r.termination, r.cholesky_failures) == (0, 0, "iterations exhausted", 0)
    assert by["no edges"].initial_objective == 0.0 and by["no free vertex"].initial_objective > 0.0
    assert by["inactive vertex"].n_free == 7
    w = by["outlier"].weight  # tests/test_pose_graph.py::test_restatement_planted_outlier_is_down_weighted
    assert w[-1] < 0.05 and np.all(w[:-1] > 0.9)
    npd = by["non pd"]
    assert npd.cholesky_failures > 0 and npd.termination != "fail" and npd.final_objective < npd.initial_objective
    assert all(by[n].cholesky_failures == 0 for n in names if n != "non pd")
    # a failing dogleg (lambda cannot grow past 1e3 with initial_lambda = 1e3) ends that graph alone
    from dvo_slam_amd import graph

    fail = graph.optimize_batch(trk, [to_pose_graph(mixed["non pd"]), to_pose_graph(mixed["m12"])], algorithm="dogleg",
                                iterations=100, initial_lambda=1e3)
    assert fail[0].termination == "fail" and fail[0].n_iterations == 1
    ok12 = graph.optimize_batch(trk, [to_pose_graph(mixed["m12"])], algorithm="dogleg", iterations=100, initial_lambda=1e3)[0]
    assert fail[1].termination != "fail" and np.array_equal(np.stack(fail[1].poses), np.stack(ok12.poses))


@pytest.mark.gpu
def test_gpu_batch_agrees_with_the_single_entry(trk):
    """Two Levenberg iterations: these graphs converge quadratically (the restatement reaches the rounding floor of F in the
    third iteration of a local map), and the single entry cannot follow another run's decisions, so both runs are compared
    while every step still lowers F by far more than its rounding and the two summation orders decide alike.  The
    50-iteration runs are compared with the restatement above, which follows the decisions at the rounding floor."""
    maps = local_maps()[:16] + [chain_graph(CAP, 77), chain_graph(20, 78)]
    res = _batch(trk, maps, "levenberg", 2)
    for r, g in zip(res, maps):
        d = to_pose_graph(g).optimize(trk, "levenberg", iterations=2)
        f_abs = 1e-12 * max(d.initial_objective, 1.0)
        assert (r.n_iterations, r.termination, r.n_free) == (d.n_iterations, d.termination, d.n_free)
        assert np.array_equal(r.iterations["trials"], d.iterations["trials"])
        assert np.array_equal(r.iterations["accepted"], d.iterations["accepted"])
        assert np.all(np.abs(r.iterations["objective"] - d.iterations["objective"])
                      <= 1e-10 * np.abs(d.iterations["objective"]) + f_abs)
        assert np.allclose(r.iterations["lambda"], d.iterations["lambda"], rtol=1e-8, atol=0)
        assert abs(r.final_objective - d.final_objective) <= 1e-10 * abs(d.final_objective) + f_abs
        assert np.isclose(r.lambda_, d.lambda_, rtol=1e-8, atol=0)
        for A, B in zip(r.poses, d.poses):
            assert np.max(np.abs(A[:3, 3] - B[:3, 3])) <= 1e-9 and rotation_angle(A, B) <= 1e-9
        lmax = np.array([np.linalg.eigvalsh(O)[-1] for _, _, _, O in g.edges])
        bound = 2.0 * np.sqrt(np.abs(d.chi2) * lmax) * 2e-8 + lmax * 4e-16 + f_abs  # see _bars
        assert np.all(np.abs(r.chi2 - d.chi2) <= bound) and np.all(np.abs(r.weight - d.weight) <= bound / 25.0)


def _bits(r):
    return (np.stack(r.poses).tobytes(), r.chi2.tobytes(), r.weight.tobytes(),
            (r.n_iterations, r.termination, r.n_free, r.cholesky_failures),
            np.array([r.initial_objective, r.final_objective, r.lambda_, r.delta]).tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("algorithm", ["levenberg", "dogleg"])
def test_gpu_batch_invariance_bit_for_bit(trk, algorithm):
    from dvo_slam_amd import capi, graph

    maps = local_maps()
    probes = [maps[5], chain_graph(CAP, 91), _non_pd_graph()]
    filler = (maps * 3)[:99]
    other = capi.DenseTracker()
    for g in probes:
        run = lambda t, graphs: graph.optimize_batch(t, [to_pose_graph(x) for x in graphs], algorithm=algorithm,  # noqa: E731
                                                     iterations=30)
        alone = _bits(run(trk, [g])[0])
        assert _bits(run(trk, [g] + filler)[0]) == alone, "index 0 of 100"
        assert _bits(run(trk, filler + [g])[-1]) == alone, "index 99 of 100"
        assert _bits(run(other, [g])[0]) == alone, "a second context"
        assert _bits(run(trk, [g])[0]) == alone, "a second run"
        assert _bits(run(other, filler[:7] + [g] + filler[:3])[7]) == alone, "a second context, inside a batch"


@pytest.mark.gpu
def test_gpu_capacity_and_empty_batch(trk):
    from dvo_slam_amd import capi, graph

    L = graph._lib()
    opt = graph.default_options("levenberg")
    maps = local_maps()[:3]
    rc, err, after, before = _raw(L, maps[:2] + [chain_graph(CAP + 1, 5)] + maps[2:], opt, trk._h)
    assert rc == CAPACITY and "item 2" in err and _untouched(after, before)
    with pytest.raises(capi.DvoAmdError) as ei:
        graph.optimize_batch(trk, [to_pose_graph(chain_graph(CAP + 1, 5))])
    assert ei.value.status == CAPACITY
    assert L.dvo_amd_optimize_graphs_batch(trk._h, 0, None, C.byref(opt)) == OK
    assert graph.optimize_batch(trk, []) == []
    # the cap itself is taken, outputs may be NULL
    items, keep = _items([chain_graph(CAP, 6)], with_outputs=False)
    assert L.dvo_amd_optimize_graphs_batch(trk._h, 1, items, C.byref(opt)) == OK
    assert items[0].stats.n_free == CAP and items[0].stats.final_objective < 1e-10 * items[0].stats.initial_objective


@pytest.mark.gpu
def test_gpu_local_maps_example_runs(tmp_path):
    from dvo_slam_amd import _build

    _build.build()
    exe = os.path.join(ROOT, "examples", "_build", "local_maps_example")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.join(ROOT, "dvo_slam_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "local_maps_example.c"), "-o", exe, "-L" + libdir, "-ldvo_amd", "-lm",
           "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("local map")]
    assert len(lines) == 3, res.stdout
    for ln, frames in zip(lines, (6, 9, 12)):
        m = re.search(r"(\d+) free vertices, (\d+) iterations, termination (\d+), F (\S+) -> (\S+)", ln)
        n_free, its, _, f0, f1 = int(m.group(1)), int(m.group(2)), int(m.group(3)), float(m.group(4)), float(m.group(5))
        assert n_free == frames and its >= 1
        assert np.isfinite(f0) and np.isfinite(f1) and f1 < f0
