"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star):
  * pyramid planes, point selection, residuals and validity decisions: bit-exact against the oracle
    (rcp_mode = EXACT; the reference's _mm_rcp_ps is a host-specific approximation that no other machine reproduces);
  * estimated pose: || log(T_oracle^-1 T_gpu) || <= 1e-5 over (upsilon, omega).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-5  # BASELINE.json: ||log(T_ref^-1 T_gpu)|| <= 1e-5
# The reference algorithm is chaotic at the 1e-4 level: a +-1 change of the valid-constraint count V of one iteration
# (caused by a 1e-8 difference of the pose, i.e. by the order fp32 sums are taken in) re-pairs every later residual in
# computeScaleSse (quirk Q5) and moves the V % 50 tail the likelihood drops (Q6); the likelihood jumps by ~1e4 and the
# accept / reject decision of that iteration can flip, so one path takes a last step the other does not.
# tests/test_oracle.py::test_reference_algorithm_is_chaotic shows the oracle doing this to itself.  When GPU and oracle
# take the same path (same iteration count and termination per level) the 1e-5 bar applies.  When they fork, the flipped
# decision is adjudicated on its own evidence and the oracle is CONTINUED from the GPU's own state behind it
# (tests/fork_criterion.py, orc_match_from): the GPU's remaining iterations must be same-path with that continuation and its
# final pose within 1e-5 of the continuation's.  Deterministic: nothing is sampled, there is no tolerance for forked paths
# beyond the 1e-5 and no budget of allowed forks.
MODE_DISTANCE_TOL = 3e-4  # only for the oracle's OTHER modes (host-specific rcpps, quirk-free CLEAN): different algorithms
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    if c.lib().dvo_amd_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return c


def _pyramids(capi, orc, frame, K, levels):
    I, Z = frame
    return capi.RgbdImagePyramid(I, Z, K, levels), orc.Pyramid(I, Z, K, levels)


@pytest.fixture(scope="module")
def pair640(capi, orc, synth):
    (Ir, Zr), (Ic, Zc), Tgt = synth.make_pair(640, 480)
    K = synth.intrinsics_for(640, 480)
    gr, orr = _pyramids(capi, orc, (Ir, Zr), K, 4)
    gc, occ = _pyramids(capi, orc, (Ic, Zc), K, 4)
    return dict(gr=gr, gc=gc, orr=orr, occ=occ, Tgt=Tgt, K=K, frames=((Ir, Zr), (Ic, Zc)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _oracle_residual_image(orc, orr, occ, level, T, shape):
    pe, r, valid = orc.compute_residuals(orr, occ, level, T, orc.RCP_EXACT)
    rec, idx = orr.select(level)
    img = np.full((shape[0] * shape[1], 2), np.nan, np.float32)
    img[idx[: len(valid)][valid.astype(bool)]] = r
    return img.reshape(shape[0], shape[1], 2), len(r)


# ---------------------------------------------------------------------------------------------------------------------
# stage-wise, bit-exact
# ---------------------------------------------------------------------------------------------------------------------
def test_pyramid_planes_bit_exact(pair640):
    for which in ("r", "c"):
        g, o = pair640["g" + which], pair640["o" + which + ("r" if which == "r" else "c")]
        for level in range(4):
            w, h, k = g.level_info(level)
            assert (w, h) == o.size(level)
            assert np.array_equal(k, o.intrinsics(level))
            for plane in range(6):
                a, b = g.plane(level, plane), o.plane(level, plane)
                assert np.array_equal(np.isnan(a), np.isnan(b)), (level, plane)
                m = ~np.isnan(a)
                assert np.array_equal(_bits(a[m]), _bits(b[m])), (level, plane)


@pytest.mark.parametrize("thresholds", [(0.0, 0.0), (2.5, 0.01)])
def test_point_selection_identical(pair640, thresholds):
    ti, td = thresholds
    for level in range(4):
        count, mask = pair640["gr"].select(level, ti, td)
        rec, idx = pair640["orr"].select(level, ti, td)
        assert count == len(idx)
        om = np.zeros(mask.size, np.uint8)
        om[idx] = 1
        assert np.array_equal(mask.ravel(), om)


@pytest.mark.parametrize("level", [3, 2, 1, 0])
def test_residuals_and_validity_bit_exact(capi, orc, synth, pair640, level):
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    Tgt = pair640["Tgt"]
    odd = synth.se3_exp([0.05, -0.08, 0.1, 0.03, -0.02, 0.04])
    for T in (np.eye(4), Tgt, np.linalg.inv(Tgt), odd):
        g, n_gpu = trk.residuals(pair640["gr"], pair640["gc"], level, T)
        o, n_orc = _oracle_residual_image(orc, pair640["orr"], pair640["occ"], level, T, g.shape[:2])
        assert n_gpu == n_orc
        assert np.array_equal(np.isnan(g), np.isnan(o))
        m = ~np.isnan(g)
        assert np.array_equal(_bits(g[m]), _bits(o[m]))


def test_error_image_matches_the_oracle(capi, orc, pair640):
    """computeIntensityErrorImage (dense_tracking.cpp:378-444): |intensity residual| at every selected reference pixel whose
    warp is valid, 0 elsewhere -- against the oracle's residual stage, bit for bit"""
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    for level in (1, 3):
        img = trk.computeIntensityErrorImage(pair640["gr"], pair640["gc"], pair640["Tgt"], level=level)
        o, n = _oracle_residual_image(orc, pair640["orr"], pair640["occ"], level, pair640["Tgt"], img.shape)
        want = np.where(np.isnan(o[..., 0]), 0.0, np.abs(o[..., 0])).astype(np.float32)
        assert np.array_equal(_bits(img), _bits(want))
        assert (img > 0).sum() <= n


# ---------------------------------------------------------------------------------------------------------------------
# stage-wise, weighted iterations (a8-a12): weights, pair-quirk scale, likelihood cut, normal equations at a FIXED pose
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [3, 2, 1, 0])
def test_weighted_iteration_stages_match_the_oracle(capi, orc, synth, pair640, level):
    """One iteration body (dense_tracking.cpp:271-347 without accept test / solve) at fixed poses, first with unit weights
    (k = 0) and then with the t-distribution weights of the resulting precision (k >= 1: computeWeightsSse
    dense_tracking_impl.cpp:657-707, computeScaleSse incl. Q5 :590-638, computeCompleteDataLogLikelihood incl. Q6 :406-425,
    rankUpdate / b -= J^T W r math_sse.cpp:82-178) -- the stages a full match() only shows through the final pose.  The
    residual set is bit-identical on both sides; the sums are compared with a float64 restatement (fp32-epsilon level) and
    with the oracle within the reference's own sequential-fp32 error bars (tolerance block below).  The weights use the
    1-ulp v_rcp_f32 where the reference has rcpps + an exact tail (Q7): deliberate deviation, DESIGN.md section 6."""
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    gr, gc, orr, occ = pair640["gr"], pair640["gc"], pair640["orr"], pair640["occ"]
    for T in (np.eye(4), pair640["Tgt"], synth.se3_exp(synth.XI_GT_PAIR * 0.9)):
        prec = None
        for k in range(3):  # k = 0 unit weights, k = 1, 2 weighted with the previous precision
            o = orc.iteration(orr, occ, level, T, prec, orc.RCP_EXACT)
            g = trk.iteration_probe(gr, gc, level, T, prec, o["precision"])
            where = (level, k)
            assert g["n"] == o["n"], where
            n, cov, A64, b64, cs, ll64 = _f64_iteration(orc, orr, occ, level, T, prec, o["precision"])
            assert np.abs(g["scale"] - cov).max() <= F64_SCALE_RTOL * np.abs(cov).max(), where
            assert np.abs(g["scale"] - o["scale"]).max() <= REF_SCALE_RTOL * np.abs(cov).max(), where
            assert np.abs(g["precision"] - o["precision"]).max() <= 2 * REF_SCALE_RTOL * np.abs(o["precision"]).max(), where
            assert abs(g["ll"] - ll64) <= F64_LL_RTOL * abs(ll64) and abs(g["ll"] - o["ll"]) <= REF_LL_RTOL * abs(ll64), where
            assert np.abs(g["A"] - A64).max() <= F64_A_RTOL * np.abs(A64).max(), where
            assert np.abs(g["A"] - o["A"]).max() <= REF_A_RTOL * np.abs(A64).max(), where
            assert (np.abs(g["b"] - b64) / cs).max() <= F64_B_CS and (np.abs(g["b"] - o["b"]) / cs).max() <= REF_B_CS, where
            # the rcpps flavour of the reference (host specific) for the record: its 12-bit weights move the scale by < 2e-3
            s = orc.iteration(orr, occ, level, T, prec, orc.RCP_SSE)
            if s["n"] == o["n"] and k > 0:
                assert np.allclose(g["scale"], s["scale"], rtol=2e-3, atol=2e-3 * np.abs(s["scale"]).max()), where
            prec = o["precision"]


from stage_f64 import f64_iteration as _f64_iteration  # noqa: E402  (tests/stage_f64.py)
import fork_criterion  # noqa: E402  (tests/fork_criterion.py)


# Tolerances of the teacher-forced stage comparison.
#  * against the float64 restatement: what the GPU's own arithmetic may deviate by (fp32 products, 1-ulp v_rcp_f32 /
#    v_sqrt_f32 in the weights, fp32 accumulation inside a wave, fp64 across blocks);
#  * against the oracle = the reference's arithmetic: the reference accumulates every sum SEQUENTIALLY in fp32 over up to
#    211 000 terms (computeScaleSse dense_tracking_impl.cpp:590-638, rankUpdate math_sse.cpp:117), which by itself is off by
#    up to 3.4e-4 relative in the scale and 1e-4 of max|b| near convergence (measured against the float64 restatement on the
#    headline pair, scripts/diag_moments.py); the GPU cannot and should not reproduce that noise, so these bounds are the
#    reference's own error bars.
F64_SCALE_RTOL, F64_A_RTOL, F64_B_CS, F64_LL_RTOL = 1e-6, 1e-6, 5e-7, 1e-6  # measured on MI355X: 1.2e-7, 1.2e-7, 5.3e-8, 1.3e-7
REF_SCALE_RTOL, REF_A_RTOL, REF_B_CS, REF_LL_RTOL = 1e-3, 1e-3, 3e-5, 2e-6    # measured: 1.9e-4, 2.0e-4, 8.6e-6, 0
# the same bars on sparse and gappy passes (tests/test_sparse_passes.py: 0 .. 1 025 points, empty segments and blocks), measured on
# MI355X: F64 1.4e-7, 2.1e-7, 1.2e-7, 1.4e-7; REF 6.6e-7 (precision 5.3e-7), 1.0e-6, 5.5e-7, 0 -- few terms, little summation noise


@pytest.mark.parametrize("case", ["640x480 levels 3..0", "640x480 swapped", "336x250 levels 2..0", "1280x960 levels 4..0"])
def test_every_iteration_of_a_match_teacher_forced(capi, orc, synth, pair640, case, capsys):
    """Every Gauss-Newton iteration of a full oracle match() (BASELINE configs 2 and 3 and two more), replayed stage-wise on the GPU
    from the ORACLE's pose and previous precision of that iteration (dense_tracking.cpp:271-347 per iteration).  No pose drift
    between the two sides, so the weighted iterations (k >= 1) are held to the same tolerances as iteration 0:
    valid-constraint count exact; scale, normal equations and likelihood against a float64 restatement at fp32-epsilon level
    and against the oracle within the reference's own sequential-fp32 error bars (see the tolerance block above)."""
    if case.startswith("640x480"):
        gr, gc, orr, occ = pair640["gr"], pair640["gc"], pair640["orr"], pair640["occ"]
        if "swapped" in case:
            gr, gc, orr, occ = gc, gr, occ, orr
        first = 3
    elif case.startswith("1280x960"):
        (Ir, Zr), (Ic, Zc), _ = synth.make_pair(1280, 960)
        K = synth.intrinsics_for(1280, 960)
        gr, orr = _pyramids(capi, orc, (Ir, Zr), K, 5)
        gc, occ = _pyramids(capi, orc, (Ic, Zc), K, 5)
        first = 4
    else:
        (Ir, Zr), (Ic, Zc), _ = synth.make_pair(336, 250, xi_gt=synth.XI_GT_PAIR * 0.4)
        K = synth.intrinsics_for(336, 250)
        gr, gc = capi.RgbdImagePyramid(Ir, Zr, K, 3), capi.RgbdImagePyramid(Ic, Zc, K, 3)
        orr, occ = orc.Pyramid(Ir, Zr, K, 3), orc.Pyramid(Ic, Zc, K, 3)
        first = 2
    _teacher_forced(capi, orc, synth, gr, gc, orr, occ, first, case, capsys)


def _teacher_forced(capi, orc, synth, gr, gc, orr, occ, first, case, capsys):
    """every iteration of the oracle's match of (orr, occ), replayed on the GPU from the oracle's pose and previous precision"""
    # The reference's sequential fp32 sums drift with the number of terms (840 000 at level 0 of 1280x960): against the float64
    # restatement the oracle itself is off by 6.1e-4 (scale), 2.1e-3 (A), 1.2e-4 (b) there, the GPU by 1e-7 as everywhere.
    REF_SCALE_RTOL, REF_A_RTOL, REF_B_CS = ((2e-3, 6e-3, 4e-4) if case.startswith("1280x960") else
                                            (globals()["REF_SCALE_RTOL"], globals()["REF_A_RTOL"], globals()["REF_B_CS"]))
    trk = capi.DenseTracker(capi.Config(FirstLevel=first, LastLevel=0))
    ro = orc.match(orc.default_config(first_level=first, last_level=0, rcp_mode=orc.RCP_EXACT), orr, occ)
    n_checked = n_weighted = 0
    worst = dict(f64_scale=0.0, f64_A=0.0, f64_b=0.0, f64_ll=0.0, ref_scale=0.0, ref_A=0.0, ref_b=0.0, ref_ll=0.0)
    for L in ro["levels"]:
        prec = None
        for k, it in enumerate(L["iterations"]):
            P = it["precision"]  # float32 values: both sides evaluate A, b, ll under exactly this precision
            g = trk.iteration_probe(gr, gc, L["id"], it["estimate"], prec, P)
            where = (case, "level", L["id"], "iteration", k)
            assert g["n"] == it["valid_constraints"], where
            n, cov, A64, b64, cs, ll64 = _f64_iteration(orc, orr, occ, L["id"], it["estimate"], prec, P)
            assert n == g["n"]
            worst["f64_scale"] = max(worst["f64_scale"], np.abs(g["scale"] - cov).max() / np.abs(cov).max())
            worst["ref_scale"] = max(worst["ref_scale"], np.abs(g["scale"] - it["scale"]).max() / np.abs(cov).max())
            worst["f64_ll"] = max(worst["f64_ll"], abs(g["ll"] - ll64) / abs(ll64))
            worst["ref_ll"] = max(worst["ref_ll"], abs(-g["ll"] - it["tdist_loglik"]) / abs(ll64))
            worst["f64_A"] = max(worst["f64_A"], np.abs(g["A"] - A64).max() / np.abs(A64).max())
            worst["f64_b"] = max(worst["f64_b"], (np.abs(g["b"] - b64) / cs).max())
            if it["has_increment"]:  # Mu = 0: Statistics' EstimateInformation is A, the right-hand side is b
                worst["ref_A"] = max(worst["ref_A"], np.abs(g["A"] - it["information"]).max() / np.abs(A64).max())
                worst["ref_b"] = max(worst["ref_b"], (np.abs(g["b"] - it["rhs"]) / cs).max())
            assert worst["f64_scale"] <= F64_SCALE_RTOL and worst["ref_scale"] <= REF_SCALE_RTOL, where + (worst,)
            assert worst["f64_ll"] <= F64_LL_RTOL and worst["ref_ll"] <= REF_LL_RTOL, where + (worst,)
            assert worst["f64_A"] <= F64_A_RTOL and worst["ref_A"] <= REF_A_RTOL, where + (worst,)
            assert worst["f64_b"] <= F64_B_CS and worst["ref_b"] <= REF_B_CS, where + (worst,)
            n_checked += 1
            n_weighted += k > 0
            prec = P
    with capsys.disabled():
        print(f"\n[teacher-forced {case}] {n_checked} iterations ({n_weighted} weighted): worst deviations "
              + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert n_checked >= 10 and n_weighted >= 6
    return worst


@pytest.mark.parametrize("n_drop", [0, 1, 2, 3, 49])
def test_weighted_stage_tails(capi, orc, synth, n_drop):
    """V mod 2 / mod 4 / mod 50 tails of the order-dependent stages (Q5 odd tail :566-572, Q6 :413-424, Q7 :667-706): drop the
    depth of the last n_drop selected pixels of a small level so that V takes every residue class."""
    w, h = 160, 120
    (Ir, Zr), (Ic, Zc), Tgt = synth.make_pair(w, h, xi_gt=synth.XI_GT_PAIR * 0.5)
    Zr = Zr.copy()
    ok = np.flatnonzero(~np.isnan(Zr.ravel()))
    Zr.ravel()[ok[len(ok) - 2 * n_drop:]] = np.nan
    K = synth.intrinsics_for(w, h)
    gr, gc = capi.RgbdImagePyramid(Ir, Zr, K, 1), capi.RgbdImagePyramid(Ic, Zc, K, 1)
    orr, occ = orc.Pyramid(Ir, Zr, K, 1), orc.Pyramid(Ic, Zc, K, 1)
    trk = capi.DenseTracker(capi.Config(FirstLevel=0, LastLevel=0))
    o0 = orc.iteration(orr, occ, 0, Tgt, None, orc.RCP_EXACT)
    o1 = orc.iteration(orr, occ, 0, Tgt, o0["precision"], orc.RCP_EXACT)
    g1 = trk.iteration_probe(gr, gc, 0, Tgt, o0["precision"], o1["precision"])
    assert g1["n"] == o1["n"]
    n, cov, A64, b64, cs, ll64 = _f64_iteration(orc, orr, occ, 0, Tgt, o0["precision"], o1["precision"])
    assert np.abs(g1["scale"] - cov).max() <= F64_SCALE_RTOL * np.abs(cov).max()
    assert abs(g1["ll"] - ll64) <= F64_LL_RTOL * abs(ll64) and abs(g1["ll"] - o1["ll"]) <= REF_LL_RTOL * abs(ll64)
    assert np.abs(g1["A"] - A64).max() <= F64_A_RTOL * np.abs(A64).max()
    assert (np.abs(g1["b"] - b64) / cs).max() <= F64_B_CS


# ---------------------------------------------------------------------------------------------------------------------
# full match(): pose parity, statistics, quirks
# ---------------------------------------------------------------------------------------------------------------------
# which configurations took the same iteration path as the oracle and which forked (tests/fork_criterion.py); the last test
# of this file asserts that the number of forks does not grow
_PATHS = {"same": [], "forked": [], "fork_err": [], "reports": []}
# Per-iteration checks of a free-running match() against the oracle's: fork_criterion.compare_iterations (the tolerances and
# their reasons live there).  levels_orc here: [(V, -ll, P 2x2, has_increment, increment)] per level.
ITER_COUNT_SLACK = fork_criterion.ITER_COUNT_SLACK


def _compare_iterations(levels_gpu, levels_orc, label, first_is_identical=True, count_slack=None, increment_band=0.0):
    """Asserts the per-iteration quantities of two same-path runs; returns (iterations compared, iterations with identical V).
    increment_band: only the sensor-noise suite passes one (the analytic suite keeps 3e-6 / 2e-2)."""
    G = [dict(id=L["Id"], termination=L["TerminationCriterion"],
              iters=[dict(V=it["ValidConstraints"], nll=it["TDistributionLogLikelihood"], has_inc=it["has_increment"],
                          inc=it["EstimateIncrement"], P=it["TDistributionPrecision"]) for it in L["Iterations"]]) for L in levels_gpu]
    O = [dict(id=Lg["id"], termination=Lg["termination"],
              iters=[dict(V=V, nll=nll, P=P, has_inc=bool(has_inc), inc=inc) for V, nll, P, has_inc, inc in Lo])
         for Lg, Lo in zip(G, levels_orc)]
    return fork_criterion.compare_iterations(G, O, label, first_is_identical=first_is_identical, count_slack=count_slack,
                                             increment_band=increment_band)


def _oracle_levels(ro):
    return [[(it["valid_constraints"], it["tdist_loglik"], it["precision"], it["has_increment"], it["increment"])
             for it in L["iterations"]] for L in ro["levels"]]


def _check_match(capi, orc, synth, g_ref, g_cur, o_ref, o_cur, cfg_kw, T_init=None, tol=POSE_TOL, paths=None, label=None,
                 count_slack=None, increment_band=0.0, mask=None):
    # mask: a capi.SelectionMask of the GPU's match; o_ref then carries the same restriction as its keep plane (Pyramid.set_keep),
    # which every oracle entry used below follows by itself
    import inspect

    _PATHS = paths if paths is not None else globals()["_PATHS"]  # (the sensor-regime suite keeps its own book)
    label = label or (inspect.stack()[1].function + repr(sorted(cfg_kw.items())))
    gcfg = capi.Config(**cfg_kw)
    trk = capi.DenseTracker(gcfg)
    rg = trk.match(g_ref, g_cur, T_init, mask=mask)
    ocfg = fork_criterion.oracle_config_of(orc, gcfg)
    ro = orc.match(ocfg, o_ref, o_cur, T_init)
    err = synth.pose_error(ro["T"], rg.Transformation)
    same_path = fork_criterion.same_path(rg, ro)
    _PATHS["same" if same_path else "forked"].append(label)
    _PATHS.setdefault("errs", []).append(err)
    if not same_path:
        _PATHS.setdefault("fork_err", []).append(err)
    if same_path:
        if err > tol:
            # the oracle's own iteration path and still beyond the bar (an alignment cut short by MaxIterationsPerLevel, a short coarse
            # stage): nothing flipped, so nothing to re-synchronise -- every increment teacher-forced against the reference
            # arithmetic's own summation-noise band, the distance against the oracle's noise on its last level
            # (fork_criterion.same_path_beyond_the_bar: the rule the validator's stages are held to)
            lines = fork_criterion.same_path_beyond_the_bar(orc, synth, ocfg, o_ref, o_cur, rg, ro, err, tol)
            _PATHS.setdefault("same_beyond", []).append((label, lines))
            print(f"[same path beyond the bar] {label}: " + " | ".join(lines))
        # every Gauss-Newton iteration, not only the final pose; a constraint count that differs from the oracle's (pose drift) is
        # held to the reference's residual stage at the GPU's own pose, exactly (fork_criterion.count_probe)
        n_it, n_same_v = fork_criterion.compare_iterations(fork_criterion.gpu_levels(rg), fork_criterion.oracle_levels(ro), label,
                                                           count_slack=count_slack, increment_band=increment_band,
                                                           probe=fork_criterion.count_probe(orc, ocfg, o_ref, o_cur))
        print(f"[iterations] {label}: {n_it} compared, {n_same_v} with identical ValidConstraints, pose err {err:.2e}")
    else:
        # no blanket tolerance and nothing sampled: the flipped decision is adjudicated, the oracle is continued from the GPU's own
        # state behind it, and the GPU's remaining iterations and final pose are held to that continuation (tests/fork_criterion.py)
        report, _, _ = fork_criterion.adjudicate(orc, synth, ocfg, o_ref, o_cur, T_init, rg, ro, err, tol, count_slack, increment_band)
        _PATHS["reports"].append((label, report))
        # up to the fork both ran the same iterations: compare the common prefix of every level up to the first level whose
        # iteration count differs
        for Lg, Lo in zip(rg.Levels, ro["levels"]):
            if len(Lg["Iterations"]) != len(Lo["iterations"]) or Lg["TerminationCriterion"] != Lo["termination"]:
                break
            li = rg.Levels.index(Lg)
            fork_criterion.compare_iterations(fork_criterion.gpu_levels(rg), fork_criterion.oracle_levels(ro), label + " (prefix)",
                                              start=(li, 0), until=(li, len(Lg["Iterations"]) - 1), first_is_identical=li == 0,
                                              count_slack=count_slack, increment_band=increment_band,
                                              probe=fork_criterion.count_probe(orc, ocfg, o_ref, o_cur))
    assert rg.isNaN() == ro["is_nan"]
    assert [L["Id"] for L in rg.Levels] == [L["id"] for L in ro["levels"]]
    for Lg, Lo in zip(rg.Levels, ro["levels"]):
        assert Lg["ValidPixels"] == Lo["valid_pixels"] and Lg["MaxValidPixels"] == Lo["max_valid_pixels"]
        # the first iteration of the first level sees identical inputs: identical constraint count
    assert rg.Levels[0]["Iterations"][0]["ValidConstraints"] == ro["levels"][0]["iterations"][0]["valid_constraints"]
    return rg, ro, err


def test_match_640x480_4_levels(capi, orc, synth, pair640):
    """BASELINE config 2: synthetic 640x480 pair, FirstLevel 3 -> LastLevel 0."""
    rg, ro, err = _check_match(capi, orc, synth, pair640["gr"], pair640["gc"], pair640["orr"], pair640["occ"],
                               dict(FirstLevel=3, LastLevel=0))
    assert err <= POSE_TOL  # the headline pair meets the bar whichever path it takes
    assert synth.pose_error(pair640["Tgt"], rg.Transformation) < 2e-5  # and it is the right answer
    # first iteration of the coarsest level: same residuals, unit weights -> same scale / normal equations up to summation order
    ig, io = rg.Levels[0]["Iterations"][0], ro["levels"][0]["iterations"][0]
    assert np.allclose(ig["TDistributionPrecision"], io["precision"], rtol=2e-5)
    assert abs(ig["TDistributionLogLikelihood"] - io["tdist_loglik"]) <= 2e-5 * abs(io["tdist_loglik"])
    assert np.allclose(ig["EstimateInformation"], io["information"], rtol=1e-4, atol=1e-4 * np.abs(io["information"]).max())
    assert np.allclose(ig["EstimateIncrement"], io["increment"], rtol=1e-3, atol=1e-7)
    # Result::Information = A * 0.008^2 of the last iteration with an increment (dense_tracking.cpp:372)
    last = rg.Levels[-1]
    its = last["Iterations"]
    src = its[-2] if last["TerminationCriterion"] == 2 else its[-1]
    assert np.allclose(rg.Information, src["EstimateInformation"] * 0.008 * 0.008)
    assert rg.LogLikelihood == src["TDistributionLogLikelihood"] + src["PriorLogLikelihood"]
    # the final information matrix carries the scale P of the last accepted iteration; if GPU and oracle end on different
    # iterations of the last level (forked path, tests/fork_criterion.py) it is only comparable to the size of that step
    same_path = all(Lg["TerminationCriterion"] == Lo["termination"] and len(Lg["Iterations"]) == len(Lo["iterations"])
                    for Lg, Lo in zip(rg.Levels, ro["levels"]))
    tol = 5e-3 if same_path else 0.15
    assert np.allclose(rg.Information, ro["information"], rtol=tol, atol=tol * np.abs(ro["information"]).max())


@pytest.mark.parametrize("size", [(640, 480, 4), (1280, 960, 5)])
def test_headline_parity_against_all_oracle_modes(capi, orc, synth, size, capsys):
    """BASELINE configs 2 and 3: the gate (1e-5) is against the exact-reciprocal oracle; the rcpps oracle is host specific
    (its own distance to the exact mode is ~8e-5 on the EPYC host), the CLEAN oracle (no Q5 / Q6) shows how little the
    reference's quirks move the answer.  The figures are printed for the record (pytest -s)."""
    w, h, levels = size
    (Ir, Zr), (Ic, Zc), Tgt = synth.make_pair(w, h)
    K = synth.intrinsics_for(w, h)
    g = capi.DenseTracker(capi.Config(FirstLevel=levels - 1, LastLevel=0)).match(
        capi.RgbdImagePyramid(Ir, Zr, K, levels), capi.RgbdImagePyramid(Ic, Zc, K, levels))
    pr, pc = orc.Pyramid(Ir, Zr, K, levels), orc.Pyramid(Ic, Zc, K, levels)
    err = {}
    for name, mode in (("exact", orc.RCP_EXACT), ("rcpps", orc.RCP_SSE), ("clean", orc.RCP_CLEAN)):
        o = orc.match(orc.default_config(first_level=levels - 1, last_level=0, rcp_mode=mode), pr, pc)
        err[name] = synth.pose_error(o["T"], g.Transformation)
    with capsys.disabled():
        print(f"\n[parity {w}x{h}] vs exact-reciprocal oracle {err['exact']:.2e}, vs rcpps oracle (this host) {err['rcpps']:.2e}, "
              f"vs CLEAN oracle {err['clean']:.2e}, vs ground truth {synth.pose_error(Tgt, g.Transformation):.2e}")
    assert err["exact"] <= POSE_TOL
    assert err["rcpps"] <= MODE_DISTANCE_TOL and err["clean"] <= MODE_DISTANCE_TOL
    assert synth.pose_error(Tgt, g.Transformation) < 2e-5


@pytest.mark.parametrize("size", [(336, 250, 3), (64, 48, 2), (132, 97, 1), (1008, 500, 3)])
def test_odd_sizes_match_the_oracle(capi, orc, synth, size):
    """Widths that are not multiples of 64, odd heights, a level smaller than one wave segment, a single level: planes and
    residuals bit-exact, poses within the bar (no padding / tail assumptions leak into the result)."""
    w, h, levels = size
    (Ir, Zr), (Ic, Zc), Tgt = synth.make_pair(w, h, xi_gt=synth.XI_GT_PAIR * 0.4)
    K = synth.intrinsics_for(w, h)
    gr, gc = capi.RgbdImagePyramid(Ir, Zr, K, levels), capi.RgbdImagePyramid(Ic, Zc, K, levels)
    orr, occ = orc.Pyramid(Ir, Zr, K, levels), orc.Pyramid(Ic, Zc, K, levels)
    for level in range(levels):
        for plane in (0, 1, 2, 5):
            a, b = gc.plane(level, plane), occ.plane(level, plane)
            assert a.shape == b.shape and np.array_equal(_bits(a)[~np.isnan(b)], _bits(b)[~np.isnan(b)])
        T = synth.se3_exp(synth.XI_GT_PAIR * 0.3)
        trk = capi.DenseTracker(capi.Config(FirstLevel=levels - 1, LastLevel=0))
        got, nv = trk.residuals(gr, gc, level, T)
        want, n_want = _oracle_residual_image(orc, orr, occ, level, T, got.shape[:2])
        assert nv == n_want
        assert np.array_equal(np.isnan(got), np.isnan(want))
        m = ~np.isnan(got)
        assert np.array_equal(_bits(got[m]), _bits(want[m]))
    _check_match(capi, orc, synth, gr, gc, orr, occ, dict(FirstLevel=levels - 1, LastLevel=0))


def test_match_reference_default_levels(capi, orc, synth, pair640):
    """the reference's default FirstLevel 3 -> LastLevel 1 (dense_tracking_config.cpp:28-29)"""
    _check_match(capi, orc, synth, pair640["gr"], pair640["gc"], pair640["orr"], pair640["occ"], dict())


def test_match_with_initial_estimate_and_prior(capi, orc, synth, pair640):
    """dvo_benchmark's configuration: mu 0.05, use_initial_estimate, 50 iterations, precision 1e-4 (benchmark.yaml)"""
    T0 = synth.se3_exp(synth.XI_GT_PAIR * 0.7)
    rg, ro, _ = _check_match(capi, orc, synth, pair640["gr"], pair640["gc"], pair640["orr"], pair640["occ"],
                             dict(FirstLevel=3, LastLevel=1, MaxIterationsPerLevel=50, Precision=1e-4, Mu=0.05,
                                  UseInitialEstimate=True), T_init=T0)
    assert rg.Levels[0]["Iterations"][0]["PriorLogLikelihood"] > 0


def test_match_with_gradient_thresholds(capi, orc, synth, pair640):
    _check_match(capi, orc, synth, pair640["gr"], pair640["gc"], pair640["orr"], pair640["occ"],
                 dict(FirstLevel=3, LastLevel=0, IntensityDerivativeThreshold=2.5, DepthDerivativeThreshold=0.01))


def test_match_swapped_roles_and_larger_motion(capi, orc, synth, pair640):
    _check_match(capi, orc, synth, pair640["gc"], pair640["gr"], pair640["occ"], pair640["orr"],
                 dict(FirstLevel=3, LastLevel=0))
    (Ir, Zr), _ = pair640["frames"]
    T2 = synth.se3_exp([0.04, -0.02, 0.03, 0.015, -0.02, 0.01])
    cur = synth.render(640, 480, T2, frame_id=5)
    g2, o2 = _pyramids(capi, orc, cur, pair640["K"], 4)
    rg, ro, _ = _check_match(capi, orc, synth, pair640["gr"], g2, pair640["orr"], o2, dict(FirstLevel=3, LastLevel=0))
    assert synth.pose_error(T2, rg.Transformation) < 1e-4


def test_overflowing_likelihood_is_reproduced(capi, orc, synth, capsys):
    """computeCompleteDataLogLikelihood multiplies 50 terms 1 + 0.2 r^T P r in a double before it takes a log
    (dense_tracking_impl.cpp:413-419).  With the precisions noise-free synthetic depth produces (1e9 and more) and 50 consecutive
    large residuals the product overflows: likelihood -inf, iteration rejected (:312), the level ends early.  Found by the
    like-with-like validator test of round 3 (candidate 2 of BASELINE config 5's scenario, both initialisations); never on
    sensor data.  The GPU path screens every likelihood pass (largest Mahalanobis distance) and, only when a group of fifty could
    have overflowed, redoes the reference's own multiplications (k_ll_overflow).  Here: the pair that overflows, GPU against the
    oracle AS IT IS (same iteration path, infinite likelihood at the same iteration), against the oracle's ll_guard mode (the
    same sum without the overflow: far away, so the emulation matters), the stage probe, and the band pipeline."""
    key, cands = synth.loop_closure_scenario(640, 480, 32, decoys=False)
    K = synth.intrinsics_for(640, 480)
    c = cands[2]
    gr, orr = _pyramids(capi, orc, key["frame"], K, 4)
    gc, occ = _pyramids(capi, orc, c["frame"], K, 4)
    ocfg = orc.default_config(first_level=3, last_level=0, rcp_mode=orc.RCP_EXACT, use_initial_estimate=1)
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0, UseInitialEstimate=True))
    n_inf = 0
    for init in (np.eye(4), np.linalg.inv(c["pose"]) @ key["pose"]):
        ro = orc.match(ocfg, orr, occ, init)
        assert fork_criterion.has_overflowed_likelihood(ro), "the scenario no longer overflows: pick another pair"
        rg = trk.match(gr, gc, init)
        err = synth.pose_error(ro["T"], rg.Transformation)
        guarded = fork_criterion.without_overflow(orc, ocfg, orr, occ, init)
        far = synth.pose_error(guarded["T"], ro["T"])
        with capsys.disabled():
            print(f"\n[overflow] GPU vs oracle {err:.2e}; the oracle without the overflow lands {far:.2e} from itself; paths GPU "
                  f"{[(L['TerminationCriterion'], len(L['Iterations'])) for L in rg.Levels]} oracle "
                  f"{[(L['termination'], len(L['iterations'])) for L in ro['levels']]}")
        assert far > 1e-4  # the artefact moves the answer by far more than the bar ...
        same_path = [(L["TerminationCriterion"], len(L["Iterations"])) for L in rg.Levels] == \
                    [(L["termination"], len(L["iterations"])) for L in ro["levels"]]
        if same_path:
            assert err <= POSE_TOL  # ... and the GPU follows the reference through it
        else:
            _PATHS["forked"].append("overflow pair")
            _PATHS["fork_err"].append(err)
            _PATHS["reports"].append(("overflow pair", fork_criterion.adjudicate(orc, synth, ocfg, orr, occ, init, rg, ro, err, POSE_TOL)[0]))
        # the infinite likelihood sits at the same iteration on both sides
        g_inf = [(L["Id"], k) for L in rg.Levels for k, it in enumerate(L["Iterations"]) if not np.isfinite(it["TDistributionLogLikelihood"])]
        o_inf = [(L["id"], k) for L in ro["levels"] for k, it in enumerate(L["iterations"]) if not np.isfinite(it["tdist_loglik"])]
        assert o_inf and (g_inf == o_inf or not same_path), (g_inf, o_inf)
        n_inf += len(g_inf)
        # stage probe at the oracle's pose of that iteration: likelihood -inf on both sides
        lvl, k = o_inf[0]
        L = next(L for L in ro["levels"] if L["id"] == lvl)
        it, prev = L["iterations"][k], L["iterations"][k - 1]
        g = trk.iteration_probe(gr, gc, lvl, it["estimate"], prev["precision"], it["precision"])
        assert g["n"] == it["valid_constraints"] and g["ll"] == -np.inf
        # the band pipeline (all bands on this GPU) reproduces it too
        banded = trk.match_banded(gr, gc, 3, init)
        assert synth.pose_error(rg.Transformation, banded.Transformation) <= 1e-7
    assert n_inf >= 1


def test_match_1280x960_5_levels(capi, orc, synth):
    """BASELINE config 3"""
    (Ir, Zr), (Ic, Zc), Tgt = synth.make_pair(1280, 960)
    K = synth.intrinsics_for(1280, 960)
    gr, orr = _pyramids(capi, orc, (Ir, Zr), K, 5)
    gc, occ = _pyramids(capi, orc, (Ic, Zc), K, 5)
    rg, ro, _ = _check_match(capi, orc, synth, gr, gc, orr, occ, dict(FirstLevel=4, LastLevel=0))
    assert synth.pose_error(Tgt, rg.Transformation) < 2e-5


@pytest.mark.parametrize("name", ["pair_160x120_l3", "pair_320x240_l4_mu"])
def test_match_against_committed_golden_vectors(capi, synth, name):
    """small cases whose expected outputs are committed (generated by the oracle, tests/golden/make_golden.py)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    w, h, levels, first, last, s, mu, use_init = mg.CASES[name]
    want = np.load(os.path.join(GOLDEN, name + ".npz"))
    (Ir, Zr), (Ic, Zc), Tgt = synth.make_pair(w, h, xi_gt=synth.XI_GT_PAIR * s)
    K = synth.intrinsics_for(w, h)
    gr, gc = capi.RgbdImagePyramid(Ir, Zr, K, levels), capi.RgbdImagePyramid(Ic, Zc, K, levels)
    trk = capi.DenseTracker(capi.Config(FirstLevel=first, LastLevel=last, Mu=mu, UseInitialEstimate=use_init,
                                        MaxIterationsPerLevel=50))
    T0 = synth.se3_exp(synth.XI_GT_PAIR * s * 0.8) if use_init else None
    rg = trk.match(gr, gc, T0)
    assert synth.pose_error(want["T"], rg.Transformation) <= POSE_TOL
    assert [L["ValidPixels"] for L in rg.Levels] == list(want["levels"][:, 1])
    # the committed per-iteration vectors (V, -ll, P, increment) of every Gauss-Newton iteration (dense_tracking.cpp:273-352),
    # level by level until the two iteration paths part (a fork at a converged level's last accept / reject is legitimate:
    # chaos caveat at the top of this file; it is counted by the fork budget at the end)
    assert [L["Id"] for L in rg.Levels] == list(want["levels"][:, 0])
    rows = want["iterations"]
    forked = False
    for li, L in enumerate(rg.Levels):
        per_level = [(int(r[2]), r[3], r[5:9].reshape(2, 2).T, bool(r[4]), r[9:15]) for r in rows if int(r[0]) == L["Id"]]
        if L["TerminationCriterion"] != want["levels"][li, 2] or len(L["Iterations"]) != want["levels"][li, 3]:
            forked = True
            break
        _compare_iterations([L], [per_level], name, first_is_identical=li == 0)
    _PATHS["forked" if forked else "same"].append("golden " + name)
    if forked:
        # the committed vectors hold no poses per iteration: adjudicate the fork against the live oracle (whose final pose
        # must be the committed one)
        from oracle import oracle as orc

        ocfg = orc.default_config(first_level=first, last_level=last, mu=mu, use_initial_estimate=int(use_init),
                                  max_iterations_per_level=50, rcp_mode=orc.RCP_EXACT)
        o_ref, o_cur = orc.Pyramid(Ir, Zr, K, levels), orc.Pyramid(Ic, Zc, K, levels)
        ro = orc.match(ocfg, o_ref, o_cur, T0)
        assert synth.pose_error(want["T"], ro["T"]) <= 1e-12
        err = synth.pose_error(want["T"], rg.Transformation)
        _PATHS["fork_err"].append(err)
        _PATHS["reports"].append(("golden " + name, fork_criterion.adjudicate(orc, synth, ocfg, o_ref, o_cur, T0, rg, ro, err, POSE_TOL)[0]))
    else:
        assert np.allclose(rg.Information, want["information"], rtol=5e-3, atol=5e-3 * np.abs(want["information"]).max())
    assert [gr.select(l)[0] for l in range(levels)] == list(want["sel_counts"])
    res, n = trk.residuals(gr, gc, last, np.eye(4))
    assert n == int(want["res_count"])
    flat = res.reshape(-1, 2)
    flat = flat[~np.isnan(flat[:, 0])]
    assert np.array_equal(flat[:: max(1, len(flat) // 257)], want["res_sample"])


# ---------------------------------------------------------------------------------------------------------------------
# edge cases the reference's control flow has (NaN / too few constraints / iteration caps / bad arguments)
# ---------------------------------------------------------------------------------------------------------------------
def test_too_few_constraints_gives_nan_result(capi, orc, synth, pair640):
    (Ir, Zr), (Ic, Zc) = pair640["frames"]
    g_nan, o_nan = _pyramids(capi, orc, (Ic, np.full_like(Zc, np.nan)), pair640["K"], 4)
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    rg = trk.match(pair640["gr"], g_nan)
    ro = orc.match(orc.default_config(first_level=3, last_level=0, rcp_mode=orc.RCP_EXACT), pair640["orr"], o_nan)
    assert rg.isNaN() and ro["is_nan"]
    assert np.allclose(rg.Transformation, np.eye(4))
    for Lg, Lo in zip(rg.Levels, ro["levels"]):
        assert Lg["TerminationCriterion"] == Lo["termination"]
        assert [it["ValidConstraints"] for it in Lg["Iterations"]] == [it["valid_constraints"] for it in Lo["iterations"]]


@pytest.mark.parametrize("cfg_kw", [
    dict(FirstLevel=3, LastLevel=0, IntensityDerivativeThreshold=1e9, DepthDerivativeThreshold=1e9),  # nothing selected
    dict(FirstLevel=3, LastLevel=0, MaxIterationsPerLevel=1),                                        # one iteration per level
    dict(FirstLevel=3, LastLevel=1, Precision=1.0),                                                  # every increment "too small"
    dict(FirstLevel=2, LastLevel=2, Mu=10.0, UseInitialEstimate=True),                               # a prior that dominates
])
def test_control_flow_corner_cases_follow_the_oracle(capi, orc, synth, pair640, cfg_kw):
    """Termination criteria, statistics bookkeeping and the NaN result of the level loop (dense_tracking.cpp:247-373) where
    the loop does something other than converge: no selected pixel at all (TooFewConstraints on every level, NaN result),
    the iteration cap hit at once, a precision every increment meets, a prior that outweighs the data."""
    gcfg = capi.Config(**cfg_kw)
    T0 = synth.se3_exp(synth.XI_GT_PAIR * 0.5) if gcfg.UseInitialEstimate else None
    rg = capi.DenseTracker(gcfg).match(pair640["gr"], pair640["gc"], T0)
    ocfg = orc.default_config(first_level=gcfg.FirstLevel, last_level=gcfg.LastLevel,
                              max_iterations_per_level=gcfg.MaxIterationsPerLevel, precision=gcfg.Precision, mu=gcfg.Mu,
                              use_initial_estimate=int(gcfg.UseInitialEstimate),
                              intensity_derivative_threshold=gcfg.IntensityDerivativeThreshold,
                              depth_derivative_threshold=gcfg.DepthDerivativeThreshold, rcp_mode=orc.RCP_EXACT)
    ro = orc.match(ocfg, pair640["orr"], pair640["occ"], T0)
    assert rg.isNaN() == ro["is_nan"]
    assert [(L["Id"], L["ValidPixels"]) for L in rg.Levels] == [(L["id"], L["valid_pixels"]) for L in ro["levels"]]
    same_path = [(L["TerminationCriterion"], len(L["Iterations"])) for L in rg.Levels] == \
                [(L["termination"], len(L["iterations"])) for L in ro["levels"]]
    # the three degenerate loops leave no room for a fork; the prior-dominated one converges normally and may end on a
    # different coin flip (chaos caveat at the top of this file)
    assert same_path or cfg_kw.get("Mu", 0.0) > 0.0
    for Lg, Lo in zip(rg.Levels, ro["levels"]):
        for ig, io in list(zip(Lg["Iterations"], Lo["iterations"]))[:3]:
            assert abs(ig["ValidConstraints"] - io["valid_constraints"]) <= ITER_COUNT_SLACK
            assert abs(ig["PriorLogLikelihood"] - io["prior_loglik"]) <= 1e-5 * max(1.0, abs(io["prior_loglik"]))
    if not ro["is_nan"]:
        err = synth.pose_error(ro["T"], rg.Transformation)
        if same_path:
            assert err <= POSE_TOL
        else:
            _PATHS["forked"].append("control flow " + repr(sorted(cfg_kw.items())))
            _PATHS["fork_err"].append(err)
            _PATHS["reports"].append((_PATHS["forked"][-1], fork_criterion.adjudicate(
                orc, synth, ocfg, pair640["orr"], pair640["occ"], T0, rg, ro, err, POSE_TOL)[0]))
        if same_path:
            assert np.allclose(rg.Information, ro["information"], rtol=5e-3, atol=5e-3 * np.abs(ro["information"]).max())


def test_iteration_cap(capi, orc, synth, pair640):
    rg, ro, _ = _check_match(capi, orc, synth, pair640["gr"], pair640["gc"], pair640["orr"], pair640["occ"],
                             dict(FirstLevel=3, LastLevel=2, MaxIterationsPerLevel=2), tol=1e-4)
    for Lg, Lo in zip(rg.Levels, ro["levels"]):
        assert Lg["TerminationCriterion"] == Lo["termination"] and len(Lg["Iterations"]) == len(Lo["iterations"]) <= 2


def test_argument_errors(capi, synth, pair640):
    with pytest.raises(capi.DvoAmdError) as e:
        capi.DenseTracker(capi.Config(FirstLevel=1, LastLevel=2))
    assert e.value.status == 5  # not sane
    trk = capi.DenseTracker(capi.Config(FirstLevel=5, LastLevel=0))
    with pytest.raises(capi.DvoAmdError) as e:
        trk.match(pair640["gr"], pair640["gc"])
    assert e.value.status == 6  # pyramid has only 4 levels
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0, UseInitialEstimate=True))
    with pytest.raises(capi.DvoAmdError) as e:
        trk.match(pair640["gr"], pair640["gc"], np.full((4, 4), np.nan))
    assert e.value.status == 9
    I = np.zeros((30, 30), np.float32)
    with pytest.raises(capi.DvoAmdError):  # width % 4 != 0
        capi.RgbdImagePyramid(I, I, (10, 10, 15, 15), 1)
    (Ir, Zr), _ = pair640["frames"]
    small = capi.RgbdImagePyramid(Ir[:240, :320].copy(), Zr[:240, :320].copy(), synth.intrinsics_for(320, 240), 4)
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    with pytest.raises(capi.DvoAmdError) as e:
        trk.match(pair640["gr"], small)
    assert e.value.status == 1


def test_two_threshold_sets_share_a_pyramid_across_threads(capi, synth, pair640):
    """Finished pyramids are shared by any number of trackers and threads.  Two trackers with different gradient thresholds
    (different PointSelections on the same keyframe, point_selection.cpp:51-59) align against the same reference pyramid from
    two threads while further threshold pairs keep being added: every result equals its single-threaded one."""
    import threading

    cfgs = [capi.Config(FirstLevel=3, LastLevel=1), capi.Config(FirstLevel=3, LastLevel=1, IntensityDerivativeThreshold=2.5,
                                                                DepthDerivativeThreshold=0.01)]
    (Ir, Zr), _ = pair640["frames"]
    ref = capi.RgbdImagePyramid(Ir, Zr, pair640["K"], 4)  # a fresh pyramid: no selection cached yet
    # (a batch of 8 sums in a different order than a single match: the reference run is the same batch, single-threaded)
    want = [capi.DenseTracker(c).match_batch([pair640["gr"]] * 8, [pair640["gc"]] * 8, stats=False)[0].Transformation for c in cfgs]
    got, errs = [[], []], []

    def worker(t):
        try:
            trk = capi.DenseTracker(cfgs[t])
            for _ in range(6):
                got[t].extend(r.Transformation for r in trk.match_batch([ref] * 8, [pair640["gc"]] * 8, stats=False))
        except Exception as exc:  # pragma: no cover
            errs.append(exc)

    def selector():
        try:
            for k in range(12):
                ref.select(1, 0.5 + 0.25 * k, 0.001 * k)  # grows the selection list under the readers
        except Exception as exc:  # pragma: no cover
            errs.append(exc)

    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)] + [threading.Thread(target=selector)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    for t in range(2):
        assert len(got[t]) == 48 and all(np.array_equal(T, want[t]) for T in got[t])


def test_failed_scratch_allocation_leaves_a_working_tracker(capi, synth, pair640, monkeypatch):
    """An allocation failure while the scratch of the resident pairs is built returns DVO_AMD_ERR_OUT_OF_MEMORY and leaves
    nothing half-built behind: the retry rebuilds and gives the usual result."""
    monkeypatch.setenv("DVO_AMD_FAULT_SLOT_ALLOC", "2")
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    monkeypatch.delenv("DVO_AMD_FAULT_SLOT_ALLOC")
    with pytest.raises(capi.DvoAmdError) as e:
        trk.match_batch([pair640["gr"]] * 5, [pair640["gc"]] * 5, stats=False)
    assert e.value.status == 4
    again = trk.match_batch([pair640["gr"]] * 5, [pair640["gc"]] * 5, stats=False)
    want = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0)).match(pair640["gr"], pair640["gc"])
    assert all(synth.pose_error(want.Transformation, r.Transformation) <= POSE_TOL for r in again)


# ---------------------------------------------------------------------------------------------------------------------
# size-independent properties at full size
# ---------------------------------------------------------------------------------------------------------------------
def test_frame_against_itself_is_identity(capi, synth, pair640):
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    r = trk.match(pair640["gr"], pair640["gr"])
    assert synth.pose_error(np.eye(4), r.Transformation) < 1e-6


def test_forward_backward_consistency(capi, synth, pair640):
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    f = trk.match(pair640["gr"], pair640["gc"]).Transformation
    b = trk.match(pair640["gc"], pair640["gr"]).Transformation
    assert synth.pose_error(np.eye(4), f @ b) < 5e-5


def test_deterministic_and_batch_equals_single(capi, synth, pair640):
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    a = trk.match(pair640["gr"], pair640["gc"])
    b = trk.match(pair640["gr"], pair640["gc"])
    assert np.array_equal(a.Transformation, b.Transformation) and np.array_equal(a.Information, b.Information)
    # a batch advances the same state machines in lock step; a pair's geometry and summation tree are its level's own, so the
    # results are the single match()'s bit for bit (tests/test_determinism.py is the systematic version of this)
    refs = [pair640["gr"], pair640["gc"], pair640["gr"], pair640["gr"], pair640["gc"]]
    curs = [pair640["gc"], pair640["gr"], pair640["gr"], pair640["gc"], pair640["gc"]]
    out = trk.match_batch(refs, curs)
    singles = [trk.match(r, c) for r, c in zip(refs, curs)]
    for o, s in zip(out, singles):
        assert np.array_equal(s.Transformation, o.Transformation) and np.array_equal(s.Information, o.Information)
        assert [L["ValidPixels"] for L in o.Levels] == [L["ValidPixels"] for L in s.Levels]
    # continuous batching: at most 2 pairs resident, the others take over the slots as they free up
    rolling = trk.match_batch(refs, curs, in_flight=2)
    for o, s in zip(rolling, singles):
        assert np.array_equal(s.Transformation, o.Transformation) and np.array_equal(s.Information, o.Information)
        assert [len(L["Iterations"]) for L in o.Levels] == [len(L["Iterations"]) for L in s.Levels]
    big = trk.match_batch([pair640["gr"]] * 40, [pair640["gc"]] * 40, stats=False)  # > one launch worth of items: 2 groups
    assert all(np.array_equal(big[0].Transformation, o.Transformation) for o in big)
    assert np.array_equal(a.Transformation, big[0].Transformation)
    # 90 resident pairs = three groups ticking independently on their own streams, 130 pairs rolling through them; raw
    # result structs; mixed pairs so that the groups finish levels at different times
    n = 130
    refs = [pair640["gr"] if i % 3 else pair640["gc"] for i in range(n)]
    curs = [pair640["gc"] if i % 3 else pair640["gr"] for i in range(n)]
    raw = trk.match_batch(refs, curs, stats=False, in_flight=90, raw=True)
    fwd, bwd = singles[0], singles[1]
    for i in range(n):
        T = np.array(raw[i].transformation[:]).reshape(4, 4).T
        assert np.array_equal((fwd if i % 3 else bwd).Transformation, T)
        assert raw[i].is_nan == 0 and raw[i].n_levels == 4


def test_odometry_over_a_frame_stream_composes_to_ground_truth(capi, synth):
    """BASELINE config 4's workload (frame t-1 -> frame t along xi(t) = t * xi_step) as one batch: the chained estimates
    reproduce the trajectory, every pair agrees with ground truth, and chaining 2-frame hops agrees with 1-frame hops."""
    n, w, h = 10, 640, 480
    K = synth.intrinsics_for(w, h)
    poses = synth.stream_poses(n)
    pyr = [capi.RgbdImagePyramid(*synth.render(w, h, poses[t], frame_id=t), K, 4) for t in range(n)]
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    hops = trk.match_batch(pyr[:-1], pyr[1:], stats=False)
    acc = np.eye(4)
    for t, r in enumerate(hops):
        assert not r.isNaN()
        assert synth.pose_error(r.Transformation, poses[t + 1] @ np.linalg.inv(poses[t])) < 3e-5
        acc = r.Transformation @ acc
    assert synth.pose_error(acc, poses[-1]) < 1e-4  # nine hops, errors do not pile up
    double = trk.match_batch(pyr[:-2], pyr[2:], stats=False)
    for t, r in enumerate(double):
        assert synth.pose_error(r.Transformation, hops[t + 1].Transformation @ hops[t].Transformation) < 6e-5


def test_config4_full_size_120_frame_stream(capi, synth):
    """BASELINE config 4 at its stated size: the 120-frame trajectory xi(t) = t * xi_step, frame-to-frame odometry
    (ref = t - 1, cur = t) as one batch; every hop against ground truth, the chained pose against the end pose, and on a
    sample of frames the tile-shard band pipeline (2 / 8 bands) against the unsharded alignment."""
    n, w, h = 120, 640, 480
    K = synth.intrinsics_for(w, h)
    poses = synth.stream_poses(n)
    pyr = [capi.RgbdImagePyramid(*synth.render(w, h, poses[t], frame_id=t), K, 4) for t in range(n)]
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    hops = trk.match_batch(pyr[:-1], pyr[1:], stats=False, in_flight=72)
    acc = np.eye(4)
    errs = []
    for t, r in enumerate(hops):
        assert not r.isNaN()
        errs.append(synth.pose_error(r.Transformation, poses[t + 1] @ np.linalg.inv(poses[t])))
        acc = r.Transformation @ acc
    # against GROUND TRUTH (not the oracle): the estimator's own accuracy on this scene, 1e-5 .. 1e-4 depending on the view
    assert np.median(errs) < 5e-5 and max(errs) < 3e-4, (np.median(errs), max(errs))
    assert synth.pose_error(acc, poses[-1]) < 2e-3  # 119 hops chained
    for t in (0, 17, 59, 118):
        whole = trk.match(pyr[t], pyr[t + 1])
        for n_bands in (2, 8):
            banded = trk.match_banded(pyr[t], pyr[t + 1], n_bands)
            assert [[it["ValidConstraints"] for it in L["Iterations"]] for L in banded.Levels] == \
                   [[it["ValidConstraints"] for it in L["Iterations"]] for L in whole.Levels]
            assert np.array_equal(whole.Transformation, banded.Transformation)  # 2 and 8 divide 16: bit for bit


def test_speculative_level_start_gives_the_same_results(capi, synth, pair640, monkeypatch):
    """Speculative level starts (next level started in the tick of a level's last likelihood; always with
    DVO_AMD_SPEC_LEVELS=1, by default while at most 8 pairs are resident): fewer ticks, identical iteration paths and poses
    (the option is read when a tracker is created)."""
    cfg = capi.Config(FirstLevel=3, LastLevel=0)
    monkeypatch.setenv("DVO_AMD_SPEC_LEVELS", "0")  # (the default speculates while at most 8 pairs are resident)
    plain = capi.DenseTracker(cfg)
    monkeypatch.setenv("DVO_AMD_SPEC_LEVELS", "1")
    spec = capi.DenseTracker(cfg)
    monkeypatch.delenv("DVO_AMD_SPEC_LEVELS")
    auto = capi.DenseTracker(cfg)
    assert auto.match(pair640["gr"], pair640["gc"]).n_ticks == spec.match(pair640["gr"], pair640["gc"]).n_ticks
    fewer = 0
    for ref, cur in ((pair640["gr"], pair640["gc"]), (pair640["gc"], pair640["gr"]), (pair640["gr"], pair640["gr"])):
        a, b = plain.match(ref, cur), spec.match(ref, cur)
        assert np.array_equal(a.Transformation, b.Transformation) and np.array_equal(a.Information, b.Information)
        assert [(L["TerminationCriterion"], len(L["Iterations"])) for L in a.Levels] == \
               [(L["TerminationCriterion"], len(L["Iterations"])) for L in b.Levels]
        assert b.n_ticks <= a.n_ticks
        fewer += a.n_ticks - b.n_ticks
    assert fewer > 0
    batch = spec.match_batch([pair640["gr"]] * 50, [pair640["gc"]] * 50, stats=False, in_flight=40)
    ref = plain.match(pair640["gr"], pair640["gc"])
    assert all(np.array_equal(ref.Transformation, o.Transformation) for o in batch)


def test_queue_keeps_pairs_resident_across_submissions(capi, synth, pair640):
    """dvo_amd_match_submit / _wait / _poll: pairs queued while the tracker is still working enter the slots that open up, so
    the tracker never drains between submissions (the shape of tbb::parallel_reduce over a proposal list that keeps growing,
    keyframe_graph.cpp:587-590).  Every result is the one a single match() gives."""
    cfg = capi.Config(FirstLevel=3, LastLevel=0)
    trk, plain = capi.DenseTracker(cfg), capi.DenseTracker(cfg)
    fwd, bwd = plain.match(pair640["gr"], pair640["gc"]), plain.match(pair640["gc"], pair640["gr"])

    def pairs(n, phase):
        refs = [pair640["gr"] if (i + phase) % 2 else pair640["gc"] for i in range(n)]
        curs = [pair640["gc"] if (i + phase) % 2 else pair640["gr"] for i in range(n)]
        return refs, curs

    def check(results, n, phase):
        for i in range(n):
            want = fwd if (i + phase) % 2 else bwd
            assert np.array_equal(want.Transformation, results[i].Transformation)

    # three submissions back to back, 40 resident pairs (two groups): the second and third are queued while the first runs
    subs = [trk.submit(*pairs(n, ph), in_flight=40) for n, ph in ((50, 0), (7, 1), (90, 0))]
    ticks_before_wait = sum(r.n_ticks for r in subs[0].results(raw=True))
    assert ticks_before_wait > 0  # submit() started the work without waiting for it
    check(trk.wait(subs[1]), 7, 1)      # out of order: the small one in the middle first
    check(trk.wait(subs[0]), 50, 0)
    # poll never waits for the GPU; it completes the submission all the same
    spins = 0
    while not trk.poll(subs[2]):
        spins += 1
        assert spins < 10_000_000
    check(subs[2].results(), 90, 0)
    assert trk.poll() and trk.wait() is None  # nothing left: ticket 0 = "everything submitted so far"
    # an empty submission is complete at once; match_many (= submit + wait) still works on the same tracker afterwards
    assert trk.poll(trk.submit([], [], in_flight=40))
    check(trk.match_batch(*pairs(9, 1), in_flight=40), 9, 1)
    # a different residency lets what is queued finish in the old layout first, then re-lays the tracker out
    a = trk.submit(*pairs(30, 0), in_flight=40)
    b = trk.submit(*pairs(30, 1), in_flight=12)
    check(trk.wait(b), 30, 1)
    check(trk.wait(a), 30, 0)
    # the configuration is frozen while pairs are queued
    c = trk.submit(*pairs(20, 0), in_flight=12)
    with pytest.raises(capi.DvoAmdError):
        trk.configure(capi.Config(FirstLevel=3, LastLevel=1))
    check(trk.wait(c), 20, 0)
    trk.configure(capi.Config(FirstLevel=3, LastLevel=1))
    assert len(trk.match(pair640["gr"], pair640["gc"]).Levels) == 3


def test_entries_outside_the_queue_are_refused_while_pairs_are_queued(capi, synth, pair640):
    """the band pipeline, the residual / stage probes, the kernel bench and match_selection work in slot 0 of the
    context's scratch (or change what the queue reads): with a submission in flight they are refused like dvo_amd_configure,
    and the submission still completes with the single match()'s bits.  A Submission the caller dropped stays alive inside the
    tracker until the library is done with its result storage."""
    import gc

    cfg = capi.Config(FirstLevel=3, LastLevel=0)
    trk, plain = capi.DenseTracker(cfg), capi.DenseTracker(cfg)
    want = plain.match(pair640["gr"], pair640["gc"])
    sub = trk.submit([pair640["gr"]] * 60, [pair640["gc"]] * 60, in_flight=20)
    T = np.eye(4)
    for call in (lambda: trk.match_banded(pair640["gr"], pair640["gc"], 2),
                 lambda: trk.residuals(pair640["gr"], pair640["gc"], 0, T),
                 lambda: trk.computeIntensityErrorImage(pair640["gr"], pair640["gc"], T, 1),
                 lambda: trk.iteration_probe(pair640["gr"], pair640["gc"], 2, T),
                 lambda: trk.bench_residual_pass(pair640["gr"], pair640["gc"], 0, T, 4),
                 lambda: capi._check(capi.lib().dvo_amd_match_selection(trk._h, pair640["gr"]._h, 2.5, 0.01, pair640["gc"]._h, None,
                                                                        capi.C.byref(capi.CResult())), "dvo_amd_match_selection")):
        with pytest.raises(capi.DvoAmdError):
            call()
    for r in trk.wait(sub):
        assert np.array_equal(want.Transformation, r.Transformation)
    # idle again: the same entries work
    assert trk.residuals(pair640["gr"], pair640["gc"], 0, T)[1] > 0
    assert np.array_equal(trk.match_banded(pair640["gr"], pair640["gc"], 2).Transformation, want.Transformation)
    # fire and forget: the caller drops the Submission, the tracker keeps its result storage alive until wait() returns
    trk.submit([pair640["gr"]] * 40, [pair640["gc"]] * 40, in_flight=10)
    gc.collect()
    junk = [np.zeros(100_000) for _ in range(20)]  # churn the allocator: freed result structs would be overwritten
    assert trk.wait() is None and not trk._open
    del junk
    assert np.array_equal(trk.match(pair640["gr"], pair640["gc"]).Transformation, want.Transformation)


def test_queue_holds_its_own_pyramid_references(capi, synth):
    """The queue retains the pyramids of a submission: the caller may drop its handles right after submitting (the reference's
    callers hand boost::shared_ptr copies to their TBB tasks the same way, keyframe_graph.cpp:576-593)."""
    (Ir, Zr), (Ic, Zc), Tgt = synth.make_pair(320, 240, xi_gt=synth.XI_GT_PAIR * 0.5)
    K = synth.intrinsics_for(320, 240)
    cfg = capi.Config(FirstLevel=2, LastLevel=0)
    trk = capi.DenseTracker(cfg)
    ref, cur = capi.RgbdImagePyramid(Ir, Zr, K, 3), capi.RgbdImagePyramid(Ic, Zc, K, 3)
    want = capi.DenseTracker(cfg).match(ref, cur)
    sub = trk.submit([ref] * 12, [cur] * 12, in_flight=4)
    del ref, cur
    for r in trk.wait(sub):
        assert np.array_equal(want.Transformation, r.Transformation)
    # a tracker destroyed with pairs still queued stops its kernels and gives the pyramids back
    ref, cur = capi.RgbdImagePyramid(Ir, Zr, K, 3), capi.RgbdImagePyramid(Ic, Zc, K, 3)
    doomed = capi.DenseTracker(cfg)
    keep = doomed.submit([ref] * 30, [cur] * 30, in_flight=4)
    del doomed
    assert keep.n == 30
    assert np.array_equal(want.Transformation, capi.DenseTracker(cfg).match(ref, cur).Transformation)


def test_small_argument_blocks_change_nothing(capi, synth, pair640, monkeypatch):
    """Ticks of at most eight pairs are launched behind small kernel-argument blocks (k_tick_small / k_finalize_small, the same
    device code): every result, statistics included, is bit for bit the one of the full-size launch, and so is a nine-pair
    batch (full size, 256-thread reduce: the reducer follows one summation tree in both forms)."""
    monkeypatch.setenv("DVO_AMD_SMALL_ARGS", "0")
    full = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    monkeypatch.delenv("DVO_AMD_SMALL_ARGS")
    small = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    a, b = full.match(pair640["gr"], pair640["gc"]), small.match(pair640["gr"], pair640["gc"])
    assert np.array_equal(a.Transformation, b.Transformation) and np.array_equal(a.Information, b.Information)
    assert a.LogLikelihood == b.LogLikelihood and len(a.Levels) == len(b.Levels)
    for la, lb in zip(a.Levels, b.Levels):
        assert la["TerminationCriterion"] == lb["TerminationCriterion"] and len(la["Iterations"]) == len(lb["Iterations"])
        for ia, ib in zip(la["Iterations"], lb["Iterations"]):
            assert ia["ValidConstraints"] == ib["ValidConstraints"]
            assert ia["TDistributionLogLikelihood"] == ib["TDistributionLogLikelihood"]
            assert np.array_equal(ia["EstimateIncrement"], ib["EstimateIncrement"])
    refs, curs = [pair640["gr"], pair640["gc"]] * 4, [pair640["gc"], pair640["gr"]] * 4
    for x, y in zip(full.match_batch(refs, curs, stats=False), small.match_batch(refs, curs, stats=False)):  # eight pairs
        assert np.array_equal(x.Transformation, y.Transformation)
    nine = small.match_batch(refs + [pair640["gr"]], curs + [pair640["gc"]], stats=False)
    assert all(np.array_equal(a.Transformation, r.Transformation) for r in nine[0::2])


def test_pyramid_from_device_memory(capi, synth, pair640):
    torch = pytest.importorskip("torch")
    (Ir, Zr), (Ic, Zc) = pair640["frames"]
    dI, dZ = torch.from_numpy(Ic).cuda(), torch.from_numpy(Zc).cuda()
    torch.cuda.synchronize()
    p = capi.RgbdImagePyramid.from_device(dI.data_ptr(), dZ.data_ptr(), 640, 480, pair640["K"], 4)
    for plane in (0, 1, 5):
        assert np.array_equal(p.plane(2, plane), pair640["gc"].plane(2, plane), equal_nan=True)
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    a = trk.match(pair640["gr"], p).Transformation
    b = trk.match(pair640["gr"], pair640["gc"]).Transformation
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# frame ingest on the device: bit-exact against the oracle's restatement of the host-side conversion
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 1])
def test_ingest_raw_frame_bit_exact(capi, orc, synth, pair640, channels):
    (Ir, Zr), (Ic, Zc) = pair640["frames"]
    bgr, raw_z = synth.to_raw(Ic, Zc)
    raw_z[5, 8:24] = 0
    raw_z[6, 0], raw_z[6, 1] = 65535, 1
    img = bgr if channels == 3 else bgr[..., 1].copy()
    for scale in (1.0 / 5000.0, 0.001):
        I_o, Z_o = orc.ingest_gray(img), orc.ingest_depth(raw_z, scale)
        p = capi.RgbdImagePyramid.from_raw(img, raw_z, pair640["K"], 4, depth_scale=scale)
        assert np.array_equal(_bits(p.plane(0, 0)), _bits(I_o))
        zg = p.plane(0, 1)
        assert np.array_equal(np.isnan(zg), np.isnan(Z_o)) and np.array_equal(_bits(zg)[~np.isnan(Z_o)], _bits(Z_o)[~np.isnan(Z_o)])
        q = orc.Pyramid(I_o, Z_o, pair640["K"], 4)
        for level in range(4):
            for plane in range(6):
                a, b = p.plane(level, plane), q.plane(level, plane)
                assert np.array_equal(np.isnan(a), np.isnan(b)), (level, plane)
                assert np.array_equal(_bits(a)[~np.isnan(b)], _bits(b)[~np.isnan(b)]), (level, plane)


def test_ingest_from_device_memory_and_odd_strides(capi, orc, synth, pair640):
    torch = pytest.importorskip("torch")
    (Ir, Zr), (Ic, Zc) = pair640["frames"]
    bgr, raw_z = synth.to_raw(Ic, Zc)
    ref = capi.RgbdImagePyramid.from_raw(bgr, raw_z, pair640["K"], 4)
    # padded rows whose strides break the 4- and 8-byte alignment of the fast loads
    wide_img = torch.zeros((480, 640 * 3 + 7), dtype=torch.uint8, device="cuda")
    wide_img[:, : 640 * 3] = torch.from_numpy(bgr.reshape(480, -1)).cuda()
    wide_z = torch.zeros((480, 643), dtype=torch.int16, device="cuda")
    wide_z[:, :640] = torch.from_numpy(raw_z.view(np.int16)).cuda()
    torch.cuda.synchronize()
    p = capi.RgbdImagePyramid.from_raw_device(wide_img.data_ptr(), 3, wide_z.data_ptr(), 640, 480, pair640["K"], 4,
                                              image_stride_bytes=640 * 3 + 7, depth_stride=643)
    for level, plane in ((0, 0), (0, 1), (1, 4), (3, 2)):
        assert np.array_equal(p.plane(level, plane), ref.plane(level, plane), equal_nan=True)


def test_match_from_raw_frames_equals_oracle_on_ingested_planes(capi, orc, synth, pair640):
    (Ir, Zr), (Ic, Zc) = pair640["frames"]
    raw_r, raw_c = synth.to_raw(Ir, Zr), synth.to_raw(Ic, Zc)
    gr = capi.RgbdImagePyramid.from_raw(*raw_r, pair640["K"], 4)
    gc = capi.RgbdImagePyramid.from_raw(*raw_c, pair640["K"], 4)
    orr = orc.Pyramid(orc.ingest_gray(raw_r[0]), orc.ingest_depth(raw_r[1]), pair640["K"], 4)
    occ = orc.Pyramid(orc.ingest_gray(raw_c[0]), orc.ingest_depth(raw_c[1]), pair640["K"], 4)
    rg, ro, err = _check_match(capi, orc, synth, gr, gc, orr, occ, dict(FirstLevel=3, LastLevel=0))
    assert synth.pose_error(rg.Transformation, pair640["Tgt"]) < 2e-3  # 8-bit / 0.2 mm quantisation of the raw frame


def test_ingest_argument_errors(capi, synth, pair640):
    img = np.zeros((480, 640, 2), np.uint8)
    z = np.zeros((480, 640), np.uint16)
    with pytest.raises(Exception):
        capi.RgbdImagePyramid.from_raw(img, z, pair640["K"], 4)  # 2 channels
    with pytest.raises(Exception):
        capi.RgbdImagePyramid.from_raw(np.zeros((480, 640), np.uint8), z, pair640["K"], 4, depth_scale=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# dual-match front-end step
# ---------------------------------------------------------------------------------------------------------------------
def test_track_frame_equals_oracle_and_two_single_matches(capi, orc, synth):
    _track_frame_case(capi, orc, synth, synth.render, _PATHS)


def _track_frame_case(capi, orc, synth, render, _PATHS, gt_tol=1e-3, count_slack=None, increment_band=0.0):
    """render(width, height, T_cam, frame_id=...) -> (intensity, depth) float planes: the noise-free frames here, the sensor
    regime's in tests/test_sensor_regime.py"""
    from oracle import frontend

    K = synth.intrinsics_for(640, 480)
    poses = synth.stream_poses(7)
    frames = [render(640, 480, poses[t], frame_id=t) for t in (0, 5, 6)]  # keyframe, last frame, new frame
    g = [capi.RgbdImagePyramid(I, Z, K, 4) for I, Z in frames]
    o = [orc.Pyramid(I, Z, K, 4) for I, Z in frames]
    for cfg_kw in (dict(FirstLevel=3, LastLevel=1, UseInitialEstimate=True), dict(FirstLevel=3, LastLevel=0, UseInitialEstimate=False)):
        gcfg = capi.Config(**cfg_kw)
        trk = capi.DenseTracker(gcfg)
        ocfg = fork_criterion.oracle_config_of(orc, gcfg)
        last_kf_pose = poses[5] @ synth.se3_exp(np.array([0.002, -0.001, 0.001, 0.0005, 0.001, -0.0005]))  # a slightly-off estimate
        rk, ro, crit = trk.track_frame(g[0], g[1], g[2], last_kf_pose)
        ok, oo, ocrit = frontend.track_frame(ocfg, o[0], o[1], o[2], last_kf_pose)
        # both alignments against the oracle's of the same (reference, current, initial transformation): 1e-5 on the same path; a
        # fork is adjudicated and re-synchronised (tests/fork_criterion.py), and the criteria of that alignment are then held to
        # what the reference returns from the GPU's own state behind the fork (the continuation's result), at the same tolerances
        init_kf = np.linalg.inv(last_kf_pose)
        settled = {}
        for name, got, want, o_ref, T0 in (("keyframe", rk, ok, o[0], init_kf), ("odometry", ro, oo, o[1], np.eye(4))):
            err = synth.pose_error(got.Transformation, want["T"])
            settled[name] = want
            if fork_criterion.same_path(got, want):
                assert err <= POSE_TOL, err
            else:
                _PATHS["forked"].append(f"track_frame {sorted(cfg_kw.items())} {name}")
                _PATHS["fork_err"].append(err)
                report, _, final = fork_criterion.adjudicate(orc, synth, ocfg, o_ref, o[2], T0, got, want, err, POSE_TOL,
                                                             count_slack, increment_band)
                _PATHS["reports"].append((_PATHS["forked"][-1], report))
                settled[name] = final
        assert synth.pose_error(rk.Transformation, poses[6]) < gt_tol and synth.pose_error(ro.Transformation, poses[6] @ np.linalg.inv(poses[5])) < gt_tol
        # the likelihood is discontinuous in the valid-constraint count (Q5 re-pairing, Q6 tail): +-1 constraint moves it by
        # ~1e4 of ~4e6 even on the same iteration path, so it is only comparable to a few percent (chaos caveat above)
        for name, want in frontend.criteria(settled["keyframe"], settled["odometry"]).items():
            got = crit[name]
            if isinstance(want, bool):
                assert got == want, name
            else:
                rtol = 3e-2 if name.endswith("neg_loglik") else 2e-3
                assert abs(got - want) <= rtol * abs(want) + 1e-6, (name, got, want)
        # one two-pair batch == the two single alignments the reference runs side by side
        init = np.eye(4)
        init[:3, :3], init[:3, 3] = last_kf_pose[:3, :3].T, -last_kf_pose[:3, :3].T @ last_kf_pose[:3, 3]
        a = trk.match(g[0], g[2], init if gcfg.UseInitialEstimate else None)
        b = trk.match(g[1], g[2], np.eye(4) if gcfg.UseInitialEstimate else None)
        # identical inputs, the level's own geometry in both: the same bits
        assert np.array_equal(b.Transformation, ro.Transformation)
        assert synth.pose_error(a.Transformation, rk.Transformation) <= 1e-12  # the inverse of the pose is rounded differently
        kf_last = rk.Levels[-1]
        assert crit["keyframe_constraint_ratio"] == kf_last["Iterations"][-1]["ValidConstraints"] / kf_last["ValidPixels"]
        ev = np.linalg.eigvalsh(rk.Information)
        assert abs(crit["keyframe_condition_number"] - abs(ev[-1] / ev[0])) <= 1e-9 * abs(ev[-1] / ev[0])


# ---------------------------------------------------------------------------------------------------------------------
# tile-shard (multi-GPU) pipeline, verified with all bands on one GPU and with a 1-rank RCCL communicator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bands", [1, 2, 3, 8])
def test_banded_pipeline_equals_unsharded(capi, synth, pair640, n_bands, monkeypatch):
    # the band pipeline cuts a level into the same wave segments as the unsharded driver, whatever the band count, and folds
    # the band records along the level's summation tree: 1, 2 and 8 bands are the unsharded match bit for bit, 3 bands (off the
    # chunk boundaries of that tree) agree to the rounding of the fp64 sums
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    whole = trk.match(pair640["gr"], pair640["gc"])
    banded = trk.match_banded(pair640["gr"], pair640["gc"], n_bands)
    assert [L["ValidPixels"] for L in banded.Levels] == [L["ValidPixels"] for L in whole.Levels]
    # same constraints, same pairing, same likelihood cut: identical iteration structure; sums associate differently
    assert [[it["ValidConstraints"] for it in L["Iterations"]] for L in banded.Levels] == \
           [[it["ValidConstraints"] for it in L["Iterations"]] for L in whole.Levels]
    assert [L["TerminationCriterion"] for L in banded.Levels] == [L["TerminationCriterion"] for L in whole.Levels]
    if 16 % n_bands == 0:
        assert np.array_equal(whole.Transformation, banded.Transformation) and np.array_equal(whole.Information, banded.Information)
    else:
        assert synth.pose_error(whole.Transformation, banded.Transformation) <= 1e-12
        assert np.allclose(banded.Information, whole.Information, rtol=1e-12)


def test_sharded_match_with_single_rank_communicator(capi, synth, pair640, monkeypatch):
    """RCCL plumbing (unique id, communicator, per-tick all-gather) on the one GPU this box has"""
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    trk.comm_create(capi.comm_unique_id(), 1, 0)
    sharded = trk.match_sharded(pair640["gr"], pair640["gc"])
    whole = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0)).match(pair640["gr"], pair640["gc"])
    assert np.array_equal(whole.Transformation, sharded.Transformation)
    assert [len(L["Iterations"]) for L in sharded.Levels] == [len(L["Iterations"]) for L in whole.Levels]


@pytest.mark.parametrize("exchange", ["rccl", "peer"])
def test_sharded_overflow_verdict_with_a_single_rank(capi, synth, exchange):
    """the closed-band form of k_ll_overflow, the edge record and its extra exchange, with one rank (the two-rank case runs in
    tests/test_distributed.py): the pair whose likelihood overflows in the reference comes back as from match()"""
    key, cands = synth.loop_closure_scenario(640, 480, 32, decoys=False)
    K = synth.intrinsics_for(640, 480)
    c = cands[2]
    k_pyr, c_pyr = capi.RgbdImagePyramid(*key["frame"], K, 4), capi.RgbdImagePyramid(*c["frame"], K, 4)
    cfg = capi.Config(FirstLevel=3, LastLevel=0, UseInitialEstimate=True)
    trk = capi.DenseTracker(cfg)
    if exchange == "rccl":
        trk.comm_create(capi.comm_unique_id(), 1, 0)
    else:
        trk.exchange_attach([trk.exchange_create(1, 0)])
    plain = capi.DenseTracker(cfg)
    n_inf = 0
    for init in (np.eye(4), np.linalg.inv(c["pose"]) @ key["pose"]):
        a, b = plain.match(k_pyr, c_pyr, init), trk.match_sharded(k_pyr, c_pyr, init)
        n_inf += sum(not np.isfinite(it["TDistributionLogLikelihood"]) for L in a.Levels for it in L["Iterations"])
        assert [(L["TerminationCriterion"], len(L["Iterations"])) for L in a.Levels] == [(L["TerminationCriterion"], len(L["Iterations"])) for L in b.Levels]
        assert np.array_equal(a.Transformation, b.Transformation)
    assert n_inf >= 1


def test_closed_band_never_reads_behind_its_edge(capi):
    """ADVICE round 4.  k_ll_overflow on a CLOSED band (a rank of a tile-sharded pair: the residuals behind the band are another
    GPU's, this rank's copy of them is stale).  A chunk of the band that is not its last one can still hold the start of the group
    of fifty that straddles the band edge -- when fewer than fifty valid pixels lie behind it (a depth hole at the band edge).
    Until round 4 only the band's LAST chunk stopped at the last complete group: the other chunk walked on into the stale data
    and could raise an overflow no single-GPU match() sees.  The buffer here: a band of two chunks (16 wave segments); chunk 0
    holds 1001 valid residuals (group [1000, 1050) starts in it), chunk 1 five and then a hole, and behind the band stale
    residuals whose fifty-term product overflows."""
    trk = capi.DenseTracker(capi.Config(FirstLevel=0, LastLevel=0))
    steps, n_blocks, seg_px = 2, 8, 128
    n_px = n_blocks * 4 * seg_px
    P = np.array([[1e9, 0.0], [0.0, 1e9]], np.float32)
    res = np.full((n_px, 2), np.nan, np.float32)
    res[:1001] = 1e-6                      # chunk 0 (segments 0..7 = 1024 pixels): terms 1 + 0.2 * 2e-3
    res[1024:1029] = 1e-6                  # chunk 1: five valid pixels, then the hole up to the band edge (pixel 2048)
    res[2048:] = 0.5                       # behind the band: q = 5e8, a term of 1e8 per pixel: forty of them overflow a double
    band_valid = 1006
    kw = dict(n_blocks=n_blocks, steps=steps, seg_first=0, n_segs=16, rank_offset=0, cut_rank=5000, precision=P)
    assert trk.ll_overflow_probe(res, rank_end=band_valid, **kw) is False      # closed: group [1000, 1050) is the host's business
    assert trk.ll_overflow_probe(res, rank_end=-1, **kw) is True               # open band: the same walk may (and must) run on
    # a band that starts inside a group (rank_offset 30): its first complete group is [50, 100) = its pixels 20..69
    assert trk.ll_overflow_probe(res, rank_end=30 + band_valid, **dict(kw, rank_offset=30)) is False
    inside = res.copy()
    inside[520:570] = 0.5                  # ranks 520..569: groups [500, 550) and [550, 600) hold 30 and 20 huge terms: 1e240 at most ...
    assert trk.ll_overflow_probe(inside, rank_end=band_valid, **kw) is False
    inside[500:550] = 0.5                  # ... now group [500, 550) is all huge (1e400): overflows inside the band
    assert trk.ll_overflow_probe(inside, rank_end=band_valid, **kw) is True
    # the last chunk of a closed band: 60 valid pixels behind the last group boundary, none of them judged
    tail = np.full((n_px, 2), np.nan, np.float32)
    tail[:1000] = 1e-6
    tail[1024:1084] = 0.5                  # ranks 1000..1059: group [1000, 1050) is complete INSIDE the band: judged, overflows
    assert trk.ll_overflow_probe(tail, rank_end=1060, **kw) is True
    tail[1024:1084] = np.nan
    tail[1024:1064] = 0.5                  # ranks 1000..1039 only (they alone would overflow): completed -- and judged -- by the next rank
    assert trk.ll_overflow_probe(tail, rank_end=1040, **kw) is False


def test_sharded_match_with_single_rank_peer_exchange(capi, synth, pair640, monkeypatch):
    """the one-hop exchange (exchange buffer, k_exchange, pinned forward) with one rank: equals the band pipeline"""
    trk = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0))
    trk.exchange_attach([trk.exchange_create(1, 0)])
    sharded = trk.match_sharded(pair640["gr"], pair640["gc"])
    banded = capi.DenseTracker(capi.Config(FirstLevel=3, LastLevel=0)).match_banded(pair640["gr"], pair640["gc"], 1)
    assert np.array_equal(banded.Transformation, sharded.Transformation)
    assert [len(L["Iterations"]) for L in sharded.Levels] == [len(L["Iterations"]) for L in banded.Levels]


# ---------------------------------------------------------------------------------------------------------------------
# keep last: the fork budget
# ---------------------------------------------------------------------------------------------------------------------
def test_zz_every_fork_was_adjudicated(capsys):
    """Every _check_match() above recorded whether GPU and oracle took the same iteration path (same termination and
    iteration count on every level).  A fork is only legitimate on its own evidence (tests/fork_criterion.py): each one was
    adjudicated where it happened -- an illegitimate fork failed its test there -- and the verdicts are printed here.  There is
    no budget of allowed forks: how many configurations fork, and which, changes with any change of summation order."""
    with capsys.disabled():
        print(f"\n[paths] analytic (noise-free) regime: same path: {len(_PATHS['same'])}, forked: {len(_PATHS['forked'])} "
              f"(accumulator: {os.environ.get('DVO_AMD_ACCUM', 'mfma')}); configurations beyond 1e-5 of the oracle: "
              f"{sum(e > 1e-5 for e in _PATHS.get('errs', []))} of {len(_PATHS.get('errs', []))}, worst "
              f"{max(_PATHS.get('errs', [0.0])):.2e}; pose errors of the forked configurations: "
              f"{['%.1e' % e for e in _PATHS['fork_err']]}")
        print("[re-syncs per forked configuration] "
              + "; ".join(f"{label}: {sum(ln.startswith('re-sync') for ln in report)}" for label, report in _PATHS["reports"]))
        for label, report in _PATHS["reports"]:
            print(f"[fork] {label}")
            for line in report:
                print(f"        {line}")
    if not _PATHS["same"] and not _PATHS["forked"]:
        pytest.skip("no match configuration ran in this session")
    assert len(_PATHS["reports"]) == len(_PATHS["forked"])  # none slipped through without a verdict


def test_zz_parity_suite_under_the_register_accumulator():
    """The shipped alternative accumulator (DVO_AMD_ACCUM=valu: 87 fp32 registers per lane instead of the Gram matrix on the
    matrix pipe) sums in another order, so other configurations fork.  Under the old fork budget it would have turned the
    suite red; under the per-fork criterion every one of its forks must be legitimate too.  Runs the match-level tests of this
    file once more in a child process with the switch set (the kernel form is chosen once per process)."""
    import subprocess
    import sys

    if os.environ.get("DVO_AMD_ACCUM"):
        pytest.skip("already the child run")
    env = dict(os.environ, DVO_AMD_ACCUM="valu")
    sel = "test_match or test_odd_sizes or test_headline or test_control_flow or test_zz_every_fork"
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-s", "-x", "-k", sel,
                          "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=900)
    tail = "\n".join(res.stdout.splitlines()[-40:])
    print(tail)
    assert res.returncode == 0, tail + res.stderr[-2000:]
