"""The residual pass on sparse point sets and gappy valid streams, against the mask-aware oracle (tests/sparse_pass_cases.py).

The order-dependent parts of the pass -- a point's valid rank inside its wave segment and its carry into the next step, the two
parity hypotheses S0 / S1 and first_w that k_finalize stitches across segments (Q5), the likelihood cut at 50 floor(V / 50) and
k_ll_overflow's seg_prefix arithmetic (Q6), the last V mod 4 weights of the host-rcpps mode (Q7) -- each depend on how many valid
points the segments before them held.  Dense scenes give every segment hundreds; here segments hold none, one, an odd count, and
the cuts and tails land on segment boundaries.  The reference is the oracle with the case's keep plane (oracle.Pyramid.set_keep)
and the float64 restatement on the oracle's records (tests/stage_f64.py), never an earlier output of the library.

On the CPU: every gappy scene has the property it is named for, asserted on the oracle's own out_valid flags.  On the GPU, per
case: residuals and validity bit for bit, the teacher-forced stages inside the unchanged bars of tests/test_gpu_parity.py, the
Q7 tail's weights, a free-running match under _check_match's rule, and a batch against its single calls."""
import numpy as np
import pytest

import fork_criterion  # noqa: F401  (tests/fork_criterion.py: the rule _check_match applies)
import selection_mask_cases
import sparse_pass_cases as cases
import test_gpu_parity as P
import test_rcp_mode
from stage_f64 import f64_iteration_terms

ODD_POSE = [0.05, -0.08, 0.1, 0.03, -0.02, 0.04]  # the `odd` pose of tests/test_gpu_parity.py
# every free-running match of this file, in a book of its own (the last test reads it)
SPARSE_PATHS = {"same": [], "forked": [], "fork_err": [], "reports": [], "errs": []}
# worst deviation per bar of tests/test_gpu_parity.py over the cases of this file (the last test prints it)
WORST = dict(f64_scale=0.0, f64_A=0.0, f64_b=0.0, f64_ll=0.0, ref_scale=0.0, ref_precision=0.0, ref_A=0.0, ref_b=0.0, ref_ll=0.0)
MODES = {"exact": "RCP_EXACT", "host_sse": "RCP_SSE"}


def _mode_cases():
    """(mode, case): every case in exact mode; the cases whose quirk is mode-specific -- the counted ones and the Q7 tails -- in
    the host-rcpps mode too"""
    out = [("exact", c) for c in cases.case_names()]
    return out + [("host_sse", f"n{n}") for n in cases.COUNTS] + [("host_sse", c) for c in cases.TAIL_SCENES]


@pytest.fixture(scope="module")
def oracle_side(orc, synth):
    return cases.Oracle(orc, synth)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_the_case_list_is_the_counts_and_the_scenes():
    assert set(cases.COUNTS) == {0, 1, 63, 64, 65, 1023, 1024, 1025, 2, 5, 6, 7, 49, 50, 51, 99, 100, 101, 255, 256, 257}
    assert cases.SEG == 256 and cases.BLOCK == 1024 and len(cases.SCENES) == len(cases.PROPERTIES) == 14


@pytest.mark.parametrize("name", list(cases.SCENES))
def test_every_gappy_scene_has_the_property_it_is_named_for(orc, oracle_side, name):
    """A condition, not a measurement: the oracle's own out_valid flags of the walked stream, under the scene's keep plane at the
    scene pose (in the host-rcpps mode for the Q7 scenes, cases.scene_rcp), must give every segment its wanted count (and places, where the scene names them) and have the property."""
    ref, cur, keep = oracle_side.gappy[name]
    n_points, want_counts = cases.wanted(name)
    records, index = ref.select(cases.LEVEL)
    assert len(index) == n_points == int(keep.sum()) and n_points % 2 == 0
    _, residuals, valid = orc.compute_residuals(ref, cur, cases.LEVEL, np.eye(4), cases.scene_rcp(orc, name))
    counts = cases.segment_counts(valid)
    assert len(valid) == n_points and counts == want_counts, (name, counts)
    assert len(residuals) == sum(counts)
    at = 0
    for length, _, flags in cases.SCENES[name]:  # (where a scene wants its flags in exact places)
        assert flags is None or np.array_equal(valid[at:at + length].astype(bool), flags), name
        at += length
    assert cases.PROPERTIES[name](valid.astype(bool), counts), (name, counts)
    # and the selection stays a real motion's: the residuals are not all zero (a frame against itself makes the scale singular)
    assert np.abs(residuals).max() > 0


@pytest.mark.parametrize("n", cases.COUNTS)
def test_every_counted_case_keeps_exactly_n_points(orc, oracle_side, n):
    ref, cur, keep = oracle_side.counted[n]
    assert int(keep.sum()) == n and len(ref.select(cases.LEVEL)[1]) == n
    _, _, valid = orc.compute_residuals(ref, cur, cases.LEVEL, np.eye(4), orc.RCP_EXACT)
    assert len(valid) == n - n % 2  # Q3: an odd trailing point is counted but never walked


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    if c.lib().dvo_amd_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    return c


@pytest.fixture(scope="module")
def device_side(capi, synth, oracle_side):
    return cases.Device(capi, synth, oracle_side)


@pytest.fixture(scope="module")
def trackers(capi):
    out = {}
    for mode in MODES:
        out[mode] = capi.DenseTracker(capi.Config(FirstLevel=cases.LEVEL, LastLevel=cases.LEVEL))
        out[mode].set_reciprocal_mode(mode)
    return out


def _sides(oracle_side, device_side, case):
    o = dict((c[0], c[1:]) for c in oracle_side.cases())[case]
    return device_side.cases[case] + o[:2]  # (gr, gc, mask, orr, occ)


@pytest.mark.gpu
def test_the_level_is_walked_in_four_step_segments(trackers, device_side):
    """what puts point p in segment p // 256 and block p // 1 024; if the step table moves, the scenes have to move with it"""
    gr, _, mask = device_side.cases["empty_block"]
    steps, blocks, points = trackers["exact"].level_geometry(gr, cases.LEVEL)
    assert steps * 64 == cases.SEG and 4 * cases.SEG == cases.BLOCK
    assert points >= max(cases.COUNTS) and blocks == -(-points // cases.BLOCK)
    assert gr.select(cases.LEVEL, mask=mask)[0] == cases.wanted("empty_block")[0] > 2 * cases.BLOCK


@pytest.mark.gpu
@pytest.mark.parametrize("mode,case", _mode_cases())
def test_residuals_and_validity_bit_for_bit(orc, synth, oracle_side, device_side, trackers, mode, case):
    gr, gc, mask, orr, occ = _sides(oracle_side, device_side, case)
    rcp = getattr(orc, MODES[mode])
    _, index = orr.select(cases.LEVEL)
    for T in (np.eye(4), oracle_side.Tgt, synth.se3_exp(ODD_POSE)):
        g, n_gpu = trackers[mode].residuals(gr, gc, cases.LEVEL, T, mask=mask)
        _, r, valid = orc.compute_residuals(orr, occ, cases.LEVEL, T, rcp)
        want = np.full((g.shape[0] * g.shape[1], 2), np.nan, np.float32)
        if len(r):
            want[index[: len(valid)][valid.astype(bool)]] = r
        want = want.reshape(g.shape)
        assert n_gpu == len(r), (case, mode)
        assert np.array_equal(np.isnan(g), np.isnan(want)), (case, mode)
        m = ~np.isnan(g)
        assert np.array_equal(P._bits(g[m]), P._bits(want[m])), (case, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,case", _mode_cases())
def test_teacher_forced_stages_stay_inside_the_dense_bars(orc, oracle_side, device_side, trackers, mode, case, capsys):
    """One iteration body at the scene pose and at the ground-truth pose: k = 0 with unit weights, k = 1, 2 with the weights of the
    oracle's previous precision, A / b / ll evaluated under the oracle's precision.  The count is exact; scale, precision, A, b and
    ll are held to the float64 restatement and to the oracle inside F64_* / REF_* of tests/test_gpu_parity.py, unchanged.  One
    normaliser is restated: the likelihood's.  Below fifty constraints ll is the determinant term alone and above it that term and
    the Q6 sum can cancel, so where |ll64| is less than a tenth of the restatement's sum of absolute terms, that sum is the
    normaliser.  Below six valid constraints the probe's outputs stay zeroed, as orc_iteration leaves its own."""
    gr, gc, mask, orr, occ = _sides(oracle_side, device_side, case)
    rcp = getattr(orc, MODES[mode])
    worst = dict.fromkeys(WORST, 0.0)
    n_stages = 0
    for T in (np.eye(4), oracle_side.Tgt):
        prec = None
        for k in range(3):
            o = orc.iteration(orr, occ, cases.LEVEL, T, prec, rcp)
            where = (case, mode, "k", k, "V", o["n"])
            if o["n"] < 6:
                g = trackers[mode].iteration_probe(gr, gc, cases.LEVEL, T, prec, None, mask=mask)
                assert g["n"] == o["n"], where
                assert not g["scale"].any() and not g["precision"].any() and not g["A"].any() and not g["b"].any(), where
                assert g["ll"] == 0.0 and g["ll_sum"] == 0.0, where
                break
            g = trackers[mode].iteration_probe(gr, gc, cases.LEVEL, T, prec, o["precision"], mask=mask)
            assert g["n"] == o["n"], where
            n, cov, A64, b64, cs, ll64, ll_abs = f64_iteration_terms(orc, orr, occ, cases.LEVEL, T, prec, o["precision"], rcp_mode=rcp)
            assert n == o["n"]
            ll_norm = abs(ll64) if abs(ll64) >= 0.1 * ll_abs else ll_abs
            dev = dict(f64_scale=np.abs(g["scale"] - cov).max() / np.abs(cov).max(),
                       ref_scale=np.abs(g["scale"] - o["scale"]).max() / np.abs(cov).max(),
                       ref_precision=np.abs(g["precision"] - o["precision"]).max() / np.abs(o["precision"]).max(),
                       f64_ll=abs(g["ll"] - ll64) / ll_norm, ref_ll=abs(g["ll"] - o["ll"]) / ll_norm,
                       f64_A=np.abs(g["A"] - A64).max() / np.abs(A64).max(), ref_A=np.abs(g["A"] - o["A"]).max() / np.abs(A64).max(),
                       f64_b=(np.abs(g["b"] - b64) / cs).max(), ref_b=(np.abs(g["b"] - o["b"]) / cs).max())
            print(where, {key: f"{v:.1e}" for key, v in dev.items()})
            for key, v in dev.items():
                worst[key] = max(worst[key], float(v))
                WORST[key] = max(WORST[key], float(v))
            assert dev["f64_scale"] <= P.F64_SCALE_RTOL and dev["ref_scale"] <= P.REF_SCALE_RTOL, where + (dev,)
            assert dev["ref_precision"] <= 2 * P.REF_SCALE_RTOL, where + (dev,)
            assert dev["f64_ll"] <= P.F64_LL_RTOL and dev["ref_ll"] <= P.REF_LL_RTOL, where + (dev,)
            assert dev["f64_A"] <= P.F64_A_RTOL and dev["ref_A"] <= P.REF_A_RTOL, where + (dev,)
            assert dev["f64_b"] <= P.F64_B_CS and dev["ref_b"] <= P.REF_B_CS, where + (dev,)
            n_stages += 1
            prec = o["precision"]
    print(f"[sparse stages {case} {mode}] {n_stages} stages: worst " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.TAIL_SCENES)
def test_the_q7_tail_across_a_segment_boundary(orc, oracle_side, device_side, trackers, case):
    """host-rcpps mode: every weight of the pass, n_tail, the tail's pixels, w_table / w_exact, recomputed_equal and what the
    exact weights add, as test_every_weight_is_computeWeightsSse_as_this_host_runs_it compares them (its own body, shared)"""
    gr, gc, mask, orr, occ = _sides(oracle_side, device_side, case)
    t = test_rcp_mode.check_pass_weights(trackers["host_sse"], orc, gr, gc, orr, occ, cases.LEVEL, np.eye(4), mask=mask)
    assert t == sum(cases.wanted(case)[1]) % 4 == cases.TAIL_SCENES.index(case) + 1


@pytest.fixture(scope="module")
def singles(oracle_side, device_side, trackers):
    """{gappy case: Result of a single exact-mode match()}"""
    return {name: trackers["exact"].match(*device_side.cases[name][:2], mask=device_side.cases[name][2]) for name in cases.SCENES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.case_names())
def test_free_running_match_follows_the_oracle(capi, orc, synth, oracle_side, device_side, case):
    """trk.match(mask=) against orc.match on the keep-plane pyramid under _check_match's rule: same path -> 1e-5 and every
    iteration through compare_iterations, a fork -> adjudicated.  Fewer than six valid constraints: NaN on both sides, the same
    termination criterion and ValidPixels."""
    gr, gc, mask, orr, occ = _sides(oracle_side, device_side, case)
    rg, ro, err = P._check_match(capi, orc, synth, gr, gc, orr, occ, dict(FirstLevel=cases.LEVEL, LastLevel=cases.LEVEL), mask=mask,
                                 paths=SPARSE_PATHS, label=case)
    assert len(rg.Levels) == len(ro["levels"]) == 1
    v0 = ro["levels"][0]["iterations"][0]["valid_constraints"]
    print(f"[sparse match {case}] V of iteration 0: {v0}, pose error {err:.2e}, NaN {rg.isNaN()}")
    if v0 < 6:
        assert rg.isNaN() and ro["is_nan"], case
        assert rg.Levels[0]["TerminationCriterion"] == ro["levels"][0]["termination"], case
        assert rg.Levels[0]["ValidPixels"] == ro["levels"][0]["valid_pixels"], case
        assert [it["ValidConstraints"] for it in rg.Levels[0]["Iterations"]] == [it["valid_constraints"] for it in ro["levels"][0]["iterations"]]


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [0, 3])
def test_a_batch_of_the_gappy_cases_equals_its_single_calls(device_side, trackers, singles, in_flight):
    names = list(cases.SCENES)
    refs, curs, masks = ([device_side.cases[n][k] for n in names] for k in range(3))
    got = trackers["exact"].match_batch(refs, curs, masks=masks, in_flight=in_flight)
    for name, r in zip(names, got):
        assert selection_mask_cases.same_result(r, singles[name]), (in_flight, name)


@pytest.mark.gpu
def test_zz_every_sparse_fork_was_adjudicated_and_the_worst_deviations(capsys):
    """the book of this file's free-running matches: every fork adjudicated, none waved through; and the worst deviation per bar
    over every stage this session compared (against the float64 restatement and the oracle)"""
    S = SPARSE_PATHS
    with capsys.disabled():
        print(f"\n[sparse paths] same path: {len(S['same'])}, forked: {len(S['forked'])}; worst pose error "
              f"{max(S.get('errs') or [0.0]):.2e}; forked: {S['forked']}")
        for label, report in S["reports"]:
            print(f"[sparse fork] {label}: " + " | ".join(report))
        print("[sparse stages] worst deviations over all cases: " + ", ".join(f"{k} {v:.1e}" for k, v in WORST.items()))
    if not S["same"] and not S["forked"]:
        pytest.skip("no match of this file ran in this session")
    assert len(S["reports"]) == len(S["forked"])  # none slipped through without a verdict
