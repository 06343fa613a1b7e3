"""Pose scoring (include/dvo_amd.h, "Pose scoring"): dvo_amd_score_poses / _many, dvo_amd_pose_grid, dvo_amd_rank_poses and
constraints.seed_proposals.  The rule is pinned in the header; tests/pose_score_ref.py restates what is new in it on top of
tests/residual_mask_ref.py.  Every comparison of records is equality of integers; the only tolerance in this file is the 1e-12
of the hypothesis grid against its numpy loop (both are fp64 closed forms of about a hundred operations on entries of magnitude
<= a few: four orders above fp64 epsilon, far below anything a float cast sees).
CPU: the exports, the refusals that need no device, the ranking, the grid, the restatement fed with the oracle's residuals (the
planted pose wins at the coarsest level of every scene), the scenes' coverage.  GPU: the device's records against the restatement
fed with dvo_amd_mask_from_residuals at each hypothesis and, independently, with the oracle's residuals."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_score_ref as ps  # noqa: E402
import residual_mask_ref as rm  # noqa: E402
import selection_mask_cases as cases  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_pose_score_options", "dvo_amd_score_poses", "dvo_amd_score_poses_many", "dvo_amd_rank_poses",
               "dvo_amd_pose_grid"]
INVALID, NO_DEVICE = 1, 2
SIZES = {"80x48": (80, 48, 3), "72x50": (72, 50, 2), "64x32": (64, 32, 3)}  # (72x50: level 1 has the odd height 25)
CHUNK = 1024  # pixels of a level a block of k_score_poses owns (k_residual_mask's chunk, dvo_types.h)
# the 27 hypotheses of the tests: T_est in the middle, steps of 2 cm along x and of 2 degrees about y and z
GRID = dict(vx=(3, 0.02), wy=(3, np.deg2rad(2.0)), wz=(3, np.deg2rad(2.0)))
PLANTED = 13


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


# ---- the scenes: tests/test_residual_mask.py's recipe ---------------------------------------------------------------------------

def planted_rectangle(w, h):
    return h // 3, h // 3 + h // 4 + 1, w // 2, w // 2 + w // 4 + 1


def make_scene(synth, name, size=None):
    """A pair whose pose takes part of the reference out of the current image, NaN holes punched into both depth images, and an
    object planted into the current frame (30 % farther, intensity inverted).  T_est = reference -> current."""
    w, h, levels = size or SIZES[name]
    (Ir, Zr), (Ic, Zc), T_gt = synth.make_pair(w, h, xi_gt=3.0 * synth.XI_GT_PAIR)
    Ir, Zr, Ic, Zc = Ir.copy(), Zr.copy(), Ic.copy(), Zc.copy()
    Zr[h // 8:h // 8 + h // 6, w // 6:w // 6 + w // 8] = np.nan
    Zc[(2 * h) // 3:(2 * h) // 3 + h // 6, w // 8:w // 8 + w // 6] = np.nan
    y0, y1, x0, x1 = planted_rectangle(w, h)
    Zc[y0:y1, x0:x1] *= F(1.3)
    Ic[y0:y1, x0:x1] = F(255.0) - Ic[y0:y1, x0:x1]
    return dict(name=name, w=w, h=h, levels=levels, K=synth.intrinsics_for(w, h), ref=(Ir, Zr), cur=(Ic, Zc), T_gt=T_gt,
                T_est=np.linalg.inv(T_gt))


def oracle_level(orc, pr, pc, level, T):
    """(evaluated, residual image) of a level from the oracle: its planes and its residual stage under thresholds (-1, -1)"""
    w, h = pr.size(level)
    evaluated = rm.evaluated_ref(pr.plane(level, 1), pr.plane(level, 4), pr.plane(level, 5))
    _, res, valid = orc.compute_residuals(pr, pc, level, T, orc.RCP_EXACT, -1.0, -1.0)
    _, index = pr.select(level, -1.0, -1.0)
    return evaluated, rm.residual_image((h, w), index, valid, res)


def oracle_precision(orc, pr, pc, level, T):
    """a precision as a tracker would hold it at T: the scale estimate of unit weights, then one robust round"""
    first = orc.iteration(pr, pc, level, T, None, orc.RCP_EXACT, -1.0, -1.0)["precision"]
    return orc.iteration(pr, pc, level, T, first, orc.RCP_EXACT, -1.0, -1.0)["precision"].astype(F)


def scored_levels(levels):
    return sorted({levels - 1, 0})  # the finest and the coarsest


class OracleScene:
    """a scene in the oracle: the pyramids, the 27 hypotheses, the precision of each scored level at T_est, and per scored level
    the validity predicate and the residual image of every hypothesis (computed once, shared and left unchanged)"""

    def __init__(self, orc, capi, s):
        self.s = s
        self.pr, self.pc = orc.Pyramid(*s["ref"], s["K"], s["levels"]), orc.Pyramid(*s["cur"], s["K"], s["levels"])
        self.Ts = capi.pose_grid(s["T_est"], **GRID)
        self.P, self.evaluated, self.images = {}, {}, {}
        for l in scored_levels(s["levels"]):
            self.P[l] = oracle_precision(orc, self.pr, self.pc, l, s["T_est"])
            got = [oracle_level(orc, self.pr, self.pc, l, T) for T in self.Ts]
            self.evaluated[l], self.images[l] = got[0][0], [image for _, image in got]

    def restated(self, level, max_distance=ps.MAX_DISTANCE, invalid_distance=-1.0):
        return ps.scores_ref(self.evaluated[level], self.images[level], self.P[level], max_distance, invalid_distance)


@pytest.fixture(scope="module")
def scenes(synth):
    return {name: make_scene(synth, name) for name in SIZES}


@pytest.fixture(scope="module")
def oracle_scenes(orc, capi, scenes):
    return {name: OracleScene(orc, capi, s) for name, s in scenes.items()}


# ---- CPU: exports, defaults, refusals -------------------------------------------------------------------------------------------

def test_the_library_exports_the_entries_and_the_binding_covers_the_headers(capi):
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
    text = {h: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S) for h in ("dvo_amd.h", "dvo_amd_debug.h")}
    declared = {h: set(re.findall(r"\b(dvo_amd_[a-z0-9_]+)\s*\(", t)) for h, t in text.items()}
    assert sorted(capi.EXPORTS) == sorted(declared["dvo_amd.h"] | declared["dvo_amd_debug.h"])
    assert set(NEW_SYMBOLS) <= declared["dvo_amd.h"] and not set(NEW_SYMBOLS) & declared["dvo_amd_debug.h"]
    assert L.dvo_amd_abi_version() == 3
    assert capi.POSE_SCORE_FIELDS == ps.FIELDS and capi.POSE_SCORE_DTYPE.itemsize == 48
    assert "Pose scoring" in open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    types = open(os.path.join(ROOT, "dvo_slam_amd", "csrc", "dvo_types.h")).read()
    assert f"constexpr int kPoseScoreTile = {capi.POSE_SCORE_TILE};" in types


def test_the_default_options_are_the_documented_ones(capi):
    opt = capi.PoseScoreOptions()
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt))
    capi.lib().dvo_amd_default_pose_score_options(C.byref(opt))
    assert C.sizeof(opt) == 4 + 16 + 4 + 4
    assert opt.level == 0 and list(opt.precision) == [0.0] * 4 and opt.max_distance == F(9.2103) and opt.invalid_distance < 0
    capi.lib().dvo_amd_default_pose_score_options(None)  # a no-op
    made = capi.pose_score_options(2, precision=[[1.0, 2.0], [3.0, 4.0]], max_distance=5.0, invalid_distance=0.0)
    assert (made.level, list(made.precision), made.max_distance, made.invalid_distance) == (2, [1.0, 3.0, 2.0, 4.0], 5.0, 0.0)
    assert list(capi.pose_score_options(1, precision=[1.0, 3.0, 2.0, 4.0]).precision) == [1.0, 3.0, 2.0, 4.0]  # four floats: column-major

    class HandResult:  # level 1 ran two iterations, level 0 did not run: it takes level 1's
        Levels = [{"Id": 1, "Iterations": [{"TDistributionPrecision": np.eye(2)}, {"TDistributionPrecision": np.array([[2.0, 0.5], [0.25, 9.0]])}]}]

    assert list(capi.pose_score_options(0, result=HandResult()).precision) == [2.0, 0.25, 0.5, 9.0]
    assert list(capi.pose_score_options(1, result=HandResult()).precision) == [2.0, 0.25, 0.5, 9.0]


class Fakes:
    """zeroed buffers that stand for a context and two pyramids: an argument error is reported before any of them is looked at
    beyond its first words (refs, device, n_levels lead a pyramid: each gets two levels of size 0 x 0)"""

    def __init__(self, capi, m=3):
        self.keep = [C.create_string_buffer(1 << 20) for _ in range(3)]
        self.ctx, self.ref, self.cur = [C.c_void_p(C.addressof(b)) for b in self.keep]
        C.c_int.from_buffer(self.keep[1], 8).value = 2
        C.c_int.from_buffer(self.keep[2], 8).value = 2
        self.m = m
        self.T = (C.c_double * (16 * m))(*np.tile(np.eye(4).ravel(), m))
        self.opt = capi.pose_score_options(1, precision=[1500.0, 0.0, 0.0, 7000.0])
        self.scores = np.full(m, 0x5A5A5A5A, np.uint64).repeat(6)


def test_argument_errors_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    f = Fakes(capi)
    single, many = "dvo_amd_score_poses", "dvo_amd_score_poses_many"
    untouched = f.scores.copy()
    sp = f.scores.ctypes.data_as(C.c_void_p)

    def call(ctx=f.ctx, reference=f.ref, current=f.cur, m=f.m, T=f.T, o=f.opt, scores=sp):
        return L.dvo_amd_score_poses(ctx, reference, current, m, T, None if o is None else C.byref(o), scores)

    one_r, one_c, null_in = (C.c_void_p * 1)(f.ref), (C.c_void_p * 1)(f.cur), (C.c_void_p * 1)(None)
    ms = (C.c_int * 1)(f.m)

    def call_many(n=1, ctx=f.ctx, references=one_r, currents=one_c, m=ms, T=f.T, o=f.opt, scores=sp):
        return L.dvo_amd_score_poses_many(ctx, n, references, currents, m, T, None if o is None else (capi.PoseScoreOptions * 1)(o), scores)

    def refused(entry, rc, what, word=None):
        assert rc == INVALID, (entry, what, rc)
        reason = L.dvo_amd_last_error().decode()
        assert reason.startswith(entry + ": "), (entry, what, reason)
        assert word is None or word in reason, (entry, what, reason)
        assert np.array_equal(f.scores, untouched), (entry, what)

    for what, kw in {"ctx": dict(ctx=None), "reference": dict(reference=None), "current": dict(current=None), "T": dict(T=None),
                     "options": dict(o=None), "scores": dict(scores=None)}.items():
        refused(single, call(**kw), what, "NULL")
    for what, kw in {"ctx": dict(ctx=None), "references": dict(references=None), "currents": dict(currents=None), "m": dict(m=None),
                     "T": dict(T=None), "options": dict(o=None), "scores": dict(scores=None), "references[0]": dict(references=null_in),
                     "currents[0]": dict(currents=null_in)}.items():
        refused(many, call_many(**kw), what, "NULL")
    refused(many, call_many(n=-1), "n", "n < 0")
    for m in (0, -1):
        refused(single, call(m=m), m, "at least 1")
        refused(many, call_many(m=(C.c_int * 1)(m)), m, "at least 1")

    def with_option(**fields):
        bad = capi.PoseScoreOptions.from_buffer_copy(f.opt)
        for k, v in fields.items():
            if k == "precision":
                bad.precision[:] = v
            else:
                setattr(bad, k, v)
        return bad

    for level in (-1, 2, 7, 8, 1 << 20):  # the pyramids have levels 0 and 1
        refused(single, call(o=with_option(level=level)), level, "level")
        refused(many, call_many(o=with_option(level=level)), level, "level")
    shallow = C.create_string_buffer(1 << 20)  # a current with one level: the reference's level 1 is missing there
    C.c_int.from_buffer(shallow, 8).value = 1
    refused(single, call(current=C.c_void_p(C.addressof(shallow))), "shallow", "level")
    for what, P in {"unset": [0.0] * 4, "nan": [1.0, np.nan, 0.0, 1.0], "inf": [np.inf, 0.0, 0.0, 1.0]}.items():
        refused(single, call(o=with_option(precision=P)), what, "precision not set" if what == "unset" else "precision")
        refused(many, call_many(o=with_option(precision=P)), what, "precision")
    for v in (0.0, -1.0, np.nan, np.inf, 1024.5, 2048.0):
        refused(single, call(o=with_option(max_distance=v)), v, "max_distance")
        refused(many, call_many(o=with_option(max_distance=v)), v, "max_distance")
    for v in (np.nan, np.inf, -np.inf, 9.3, 100.0):  # (max_distance is 9.2103)
        refused(single, call(o=with_option(invalid_distance=v)), v, "invalid_distance")
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 7, 15, 16 * (f.m - 1) + 5):  # in the first and in the last hypothesis
            T = (C.c_double * (16 * f.m))(*np.tile(np.eye(4).ravel(), f.m))
            T[at] = bad
            refused(single, call(T=T), (bad, at), "transformation")
            refused(many, call_many(T=T), (bad, at), "transformation")
    # a context in the host-rcpps mode cannot be faked here (it needs the context's layout): the GPU tests refuse a real one
    if L.dvo_amd_device_count() == 0:
        # nothing left to refuse: the device is looked for, and the records stay as they were
        for o in (f.opt, with_option(max_distance=1024.0, invalid_distance=1024.0), with_option(invalid_distance=0.0),
                  with_option(level=0, invalid_distance=-7.0)):
            assert call(o=o) == NO_DEVICE and call_many(o=o) == NO_DEVICE
        assert call_many(n=0) == NO_DEVICE
        assert np.array_equal(f.scores, untouched)


# ---- CPU: ranking and the grid --------------------------------------------------------------------------------------------------

def test_rank_poses_is_a_stable_argsort_of_the_totals(capi):
    rng = np.random.default_rng(7)
    for m in (1, 2, 27, 300):
        scores = np.zeros(m, capi.POSE_SCORE_DTYPE)
        scores["total"] = rng.integers(0, 6, m).astype(np.uint64) * np.uint64(1 << 40) + np.uint64(3)  # many ties, beyond 32 bits
        for k in (0, 1, 5, m, m + 4):
            got = capi.rank_poses(scores, k)
            assert got.tolist() == ps.rank_ref(scores["total"], k).tolist() == np.argsort(scores["total"], kind="stable")[:k].tolist(), (m, k)
            assert len(got) == min(k, m)
    big = np.zeros(3, capi.POSE_SCORE_DTYPE)
    big["total"] = [np.uint64(1 << 63), np.uint64(5), np.uint64((1 << 63) + 1)]  # unsigned: 2^63 is large, not negative
    assert capi.rank_poses(big, 3).tolist() == [1, 0, 2]
    n = C.c_int(5)
    assert capi.lib().dvo_amd_rank_poses(None, 3, 1, (C.c_int * 3)(), C.byref(n)) == INVALID and n.value == 0
    assert capi.lib().dvo_amd_last_error().decode().startswith("dvo_amd_rank_poses: ")


def test_pose_grid_equals_a_numpy_loop_over_se3_exp(capi, synth):
    centre = synth.se3_exp([0.3, -0.2, 0.1, 0.2, -0.4, 0.3])
    for counts, steps in (((3, 1, 1, 1, 3, 3), (0.02, 0.0, 0.0, 0.0, np.deg2rad(2.0), np.deg2rad(2.0))),
                          ((3, 1, 5, 1, 1, 7), (0.1, 0.0, 0.05, 0.0, 0.0, np.deg2rad(5.0))),
                          ((1, 3, 3, 3, 3, 3), (0.0, 0.1, 0.2, 0.3, 0.2, 0.1)), ((1,) * 6, (0.5,) * 6)):
        axes = {name: (c, s) for name, c, s in zip(capi.POSE_GRID_AXES, counts, steps)}
        got = capi.pose_grid(centre, **axes)
        want = ps.grid_ref(synth.se3_exp, centre, counts, steps)
        assert got.shape == want.shape == (int(np.prod(counts)), 4, 4)
        assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()
        middle = (len(got) - 1) // 2
        assert got[middle].tobytes() == np.asarray(centre, np.float64).tobytes()  # the centre itself, bit for bit
        assert all(np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) for T in got)
    # wz runs fastest: the neighbours of the middle differ from it by a rotation about z
    got = capi.pose_grid(np.eye(4), **GRID)
    assert len(got) == 27 and np.array_equal(got[PLANTED], np.eye(4))
    assert np.allclose(got[PLANTED + 1], synth.se3_exp([0, 0, 0, 0, 0, np.deg2rad(2.0)]), atol=1e-15, rtol=0)
    assert np.allclose(got[PLANTED + 9], synth.se3_exp([0.02, 0, 0, 0, 0, 0]), atol=1e-15, rtol=0)
    assert np.array_equal(capi.pose_grid(), np.eye(4)[None])  # no axis, no centre: the identity alone
    for bad in (dict(vx=(2, 0.1)), dict(wz=(0, 0.1)), dict(wy=(-3, 0.1)), dict(vz=(4, 0.0))):
        with pytest.raises(capi.DvoAmdError) as err:
            capi.pose_grid(np.eye(4), **bad)
        assert err.value.status == INVALID and capi.lib().dvo_amd_last_error().decode().startswith("dvo_amd_pose_grid: ")
    with pytest.raises(TypeError):
        capi.pose_grid(np.eye(4), yaw=(3, 0.1))
    # a capacity that is too small is refused; the count alone needs no room
    opt = capi.PoseGridOptions()
    for a in range(6):
        opt.count[a], opt.step[a] = 3 if a < 2 else 1, 0.1
    n, T = C.c_int(), (C.c_double * 16)(*np.eye(4).ravel())
    out = (C.c_double * (16 * 9))()
    assert capi.lib().dvo_amd_pose_grid(C.byref(opt), T, None, 0, C.byref(n)) == 0 and n.value == 9
    assert capi.lib().dvo_amd_pose_grid(C.byref(opt), T, out, 8, C.byref(n)) == INVALID
    assert capi.lib().dvo_amd_pose_grid(C.byref(opt), T, out, 9, C.byref(n)) == 0 and n.value == 9


# ---- CPU: the restatement fed with the oracle -----------------------------------------------------------------------------------

def test_q_and_the_sums_by_hand():
    assert ps.q([0.0, 0.5, 1.0, 9.2103, 1024.0, -3.0, -0.0]).tolist() == [0, 512, 1024, int(np.floor(float(F(9.2103)) * 1024)), 1 << 20, 0, 0]
    assert ps.q(np.nextafter(F(1.0), F(0.0))) == 1023 and ps.q(F(1.0 / 1024.0)) == 1 and ps.q(np.nextafter(F(1.0 / 1024.0), F(0.0))) == 0
    outcome = np.array([[rm.UNEVALUATED, rm.INVALID, rm.INLIER], [rm.OUTLIER, rm.INLIER, rm.OUTLIER]], np.int8)
    distance = np.array([[np.nan, np.nan, 0.25], [50.0, 2.0, np.nan]], F)
    s = ps.score_ref(outcome, distance, max_distance=4.0, invalid_distance=1.0)
    assert s == dict(evaluated=5, invalid=1, inlier=2, outlier=2, cost=256 + 2048 + 2 * 4096, total=256 + 2048 + 2 * 4096 + 1024)
    assert ps.score_ref(outcome, distance, 4.0, -1.0)["total"] == s["cost"] + 4096 and ps.score_ref(outcome, distance, 4.0, 0.0)["total"] == s["cost"]


@pytest.mark.parametrize("name", sorted(SIZES))
def test_the_planted_pose_wins_at_the_coarsest_level_under_the_oracle(oracle_scenes, name):
    """a condition on the inputs: fed with the oracle's residuals, the planted pose has the strictly smallest total"""
    o = oracle_scenes[name]
    coarsest = o.s["levels"] - 1
    assert o.Ts[PLANTED].tobytes() == np.asarray(o.s["T_est"], np.float64).tobytes()
    records = o.restated(coarsest)
    totals = [r["total"] for r in records]
    order = ps.rank_ref(totals, 27)
    print(f"{name} level {coarsest}: best total {totals[order[0]]} (hypothesis {order[0]}), second {totals[order[1]]} "
          f"(hypothesis {order[1]}), margin {totals[order[1]] / totals[order[0]]:.3f}")
    assert order[0] == PLANTED and totals[order[0]] < totals[order[1]]
    assert len({r["evaluated"] for r in records}) == 1  # a property of the reference level alone


@pytest.mark.parametrize("name", sorted(SIZES))
def test_the_scenes_produce_every_outcome_on_every_level_scored(oracle_scenes, name):
    o = oracle_scenes[name]
    for l in scored_levels(o.s["levels"]):
        best = 0
        for r in o.restated(l):
            best = max(best, min(o.evaluated[l].size - r["evaluated"], r["invalid"], r["inlier"], r["outlier"]))
        assert best > 0, (name, l)
        costs = {r["cost"] for r in o.restated(l)}
        assert len(costs) > 20, (name, l)  # the hypotheses are told apart


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


def outcome_of(evaluated, plane, distance):
    """the outcome plane from dvo_amd_mask_from_residuals called with invalid_keep = 1, unevaluated_keep = 0 and its distances: a
    kept pixel is invalid (no distance) or an inlier; an evaluated pixel that is not kept is an outlier, whatever its distance"""
    outcome = np.full(evaluated.shape, rm.UNEVALUATED, np.int8)
    outcome[evaluated] = rm.OUTLIER
    outcome[evaluated & (plane == 1)] = rm.INLIER
    outcome[evaluated & (plane == 1) & np.isnan(distance)] = rm.INVALID
    assert not (plane[~evaluated] != 0).any()
    return outcome


class DeviceScene:
    """a scene on the device: the pyramids, a tracker, and per scored level the outcome and distance planes and the counts of
    dvo_amd_mask_from_residuals at each of the 27 hypotheses under the oracle's precision (computed once, shared)"""

    def __init__(self, capi, s, o):
        self.s, self.o, self.levels = s, o, s["levels"]
        self.reference = capi.RgbdImagePyramid(*s["ref"], s["K"], self.levels)
        self.current = capi.RgbdImagePyramid(*s["cur"], s["K"], self.levels)
        self.cfg = capi.Config(FirstLevel=self.levels - 1, LastLevel=1 if self.levels > 1 else 0, IntensityDerivativeThreshold=-1.0,
                               DepthDerivativeThreshold=-1.0)
        self.tracker = capi.DenseTracker(self.cfg)
        self.evaluated = {l: rm.evaluated_ref(*(self.reference.plane(l, k) for k in (1, 4, 5))) for l in scored_levels(self.levels)}
        self._planes = {}

    def options(self, capi, level, **kw):
        return capi.pose_score_options(level, precision=rm.precision_cm(self.o.P[level]), **kw)

    def planes(self, capi, max_distance=ps.MAX_DISTANCE):
        """{level: [(outcome, distance, counts) per hypothesis]} from dvo_amd_mask_from_residuals"""
        key = float(max_distance)
        if key not in self._planes:
            opt = capi.residual_mask_options(None, self.levels, max_distance=max_distance, invalid_keep=1)
            for l in range(self.levels):
                opt.precision[l][:] = list(rm.precision_cm(self.o.P[l])) if l in self.o.P else [1.0, 0.0, 0.0, 1.0]
            out = {l: [] for l in self.evaluated}
            for T in self.o.Ts:
                mask, counts, distance = capi.SelectionMask.from_residuals(self.tracker, self.reference, self.current, T=T, options=opt,
                                                                           counts=True, distance=True)
                for l in out:
                    out[l].append((outcome_of(self.evaluated[l], mask.download(l), distance[l]), distance[l],
                                   {k: int(counts[l][k]) for k in rm.COUNTS}))
            self._planes[key] = out
        return self._planes[key]

    def restated(self, capi, level, max_distance=ps.MAX_DISTANCE, invalid_distance=-1.0):
        return [ps.score_ref(outcome, distance, max_distance, invalid_distance) for outcome, distance, _ in self.planes(capi, max_distance)[level]]

    def score(self, capi, level, Ts=None, **kw):
        return self.tracker.score_poses(self.reference, self.current, self.o.Ts if Ts is None else Ts, self.options(capi, level, **kw))


@pytest.fixture(scope="module")
def device_scenes(gpu, scenes, oracle_scenes):
    return {name: DeviceScene(gpu, scenes[name], oracle_scenes[name]) for name in SIZES}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIZES))
def test_records_equal_the_restatement(gpu, device_scenes, name):
    """fed with dvo_amd_mask_from_residuals at each hypothesis, and again with the oracle's residuals; the four counts are
    dvo_amd_mask_from_residuals' own counts of that level at that T"""
    d = device_scenes[name]
    for l in scored_levels(d.levels):
        got = ps.as_ints(d.score(gpu, l))
        assert len(got) == 27
        assert got == d.restated(gpu, l), (name, l, "from_residuals")
        assert np.array_equal(d.evaluated[l], d.o.evaluated[l])
        assert got == d.o.restated(l), (name, l, "oracle")
        for j, (_, _, counts) in enumerate(d.planes(gpu)[l]):
            assert {k: got[j][k] for k in ("evaluated", "invalid", "inlier", "outlier")} == {k: counts[k] for k in ("evaluated", "invalid", "inlier", "outlier")}, (name, l, j)
        assert all(r["evaluated"] == int(d.evaluated[l].sum()) for r in got)


@pytest.mark.gpu
def test_an_odd_number_of_evaluated_pixels_leaves_the_last_one_invalid(gpu, synth):
    """Q3.  The same pair with one more NaN in the reference's depth flips the parity of every level it reaches.  In both parities
    the records equal the restatement; in the odd one `invalid` is one more than the classes that ignore Q3 count, wherever the
    last evaluated pixel has a valid residual.  Its residual without Q3 comes from dvo_amd_residuals behind a mask that drops the
    FIRST evaluated pixel: the point list is even again and reaches the last one."""
    w, h, levels = 80, 48, 3
    K = synth.intrinsics_for(w, h)
    (Ir, Zr), (Ic, Zc), T_gt = synth.make_pair(w, h)
    Zr = Zr.copy()
    Zr[32:, :] = np.nan  # the last evaluated pixel of every level lies inside the image, where the small motion keeps it in view
    Zr[24:, 48:] = np.nan
    T = np.linalg.inv(T_gt)
    Ts = gpu.pose_grid(T, wz=(3, np.deg2rad(2.0)))
    tracker = gpu.DenseTracker(gpu.Config(FirstLevel=2, LastLevel=0, IntensityDerivativeThreshold=-1.0, DepthDerivativeThreshold=-1.0))
    P = [1500.0, 0.0, 0.0, 7000.0]
    seen, one_more = set(), 0
    for extra_nan in (False, True):
        Z = Zr.copy()
        if extra_nan:
            Z[20, 40] = np.nan  # (an even pixel: it is a pixel of every level)
        reference, current = gpu.RgbdImagePyramid(Ir, Z, K, levels), gpu.RgbdImagePyramid(Ic, Zc, K, levels)
        evaluated = [rm.evaluated_ref(*(reference.plane(l, k) for k in (1, 4, 5))) for l in range(levels)]
        first_dropped = []
        for l in range(levels):
            keep = np.ones(evaluated[l].shape, np.uint8)
            keep.ravel()[np.flatnonzero(evaluated[l].ravel())[0]] = 0
            first_dropped.append(keep)
        mask = gpu.SelectionMask.from_levels(first_dropped)
        for l in range(levels):
            odd = int(evaluated[l].sum()) % 2 == 1
            seen.add(odd)
            got = ps.as_ints(tracker.score_poses(reference, current, Ts, gpu.pose_score_options(l, precision=P, max_distance=50.0)))
            images = [tracker.residuals(reference, current, l, Tj)[0] for Tj in Ts]
            assert got == ps.scores_ref(evaluated[l], images, P, 50.0), (extra_nan, l)
            if odd:
                last = np.flatnonzero(evaluated[l].ravel())[-1]
                for j, Tj in enumerate(Ts):
                    assert np.isnan(images[j].reshape(-1, 2)[last]).all()
                    without = images[j].copy()
                    without.reshape(-1, 2)[last] = tracker.residuals(reference, current, l, Tj, mask=mask)[0].reshape(-1, 2)[last]
                    ignoring = ps.scores_ref(evaluated[l], [without], P, 50.0)[0]
                    valid_there = not np.isnan(without.reshape(-1, 2)[last]).any()
                    assert got[j]["invalid"] == ignoring["invalid"] + (1 if valid_there else 0), (l, j)
                    assert got[j]["inlier"] + got[j]["outlier"] == ignoring["inlier"] + ignoring["outlier"] - (1 if valid_there else 0)
                    one_more += valid_there
    assert seen == {False, True} and one_more > 0


@pytest.mark.gpu
def test_tile_and_chunk_edges(gpu, synth, device_scenes):
    tile = gpu.POSE_SCORE_TILE
    a, b = device_scenes["80x48"], device_scenes["72x50"]
    # 80x48 level 0: 3840 pixels, three full chunks and a partial one; 72x50 level 1: 900 pixels, less than one chunk
    assert 80 * 48 == 3 * CHUNK + 768 and 36 * 25 < CHUNK
    for d, l in ((a, 0), (b, 1)):
        want = d.restated(gpu, l)
        for m in (1, tile - 1, tile, tile + 1, 2 * tile + 1):
            pick = [(5 * j + 13) % 27 for j in range(m)]  # hypotheses repeat to fill m; the first is the planted one
            got = ps.as_ints(d.score(gpu, l, Ts=d.o.Ts[pick]))
            assert got == [want[j] for j in pick], (d.s["name"], l, m)
    # a level of exactly one chunk: 64x16 at level 0
    s = make_scene(synth, "64x16", (64, 16, 1))
    assert s["w"] * s["h"] == CHUNK
    reference, current = gpu.RgbdImagePyramid(*s["ref"], s["K"], 1), gpu.RgbdImagePyramid(*s["cur"], s["K"], 1)
    tracker = gpu.DenseTracker(gpu.Config(FirstLevel=0, LastLevel=0, IntensityDerivativeThreshold=-1.0, DepthDerivativeThreshold=-1.0))
    Ts = gpu.pose_grid(s["T_est"], **GRID)
    P = [1500.0, 0.0, 0.0, 7000.0]
    evaluated = rm.evaluated_ref(*(reference.plane(0, k) for k in (1, 4, 5)))
    images = [tracker.residuals(reference, current, 0, T)[0] for T in Ts]
    want = ps.scores_ref(evaluated, images, P)
    assert min(want[PLANTED][k] for k in ("invalid", "inlier", "outlier")) > 0
    assert ps.as_ints(tracker.score_poses(reference, current, Ts, gpu.pose_score_options(0, precision=P))) == want


@pytest.mark.gpu
def test_the_limits(gpu, synth, device_scenes):
    d = device_scenes["80x48"]
    l = d.levels - 1
    # max_distance so small that every valid pixel is an outlier
    tiny = 2.0 ** -40
    got = ps.as_ints(d.score(gpu, l, max_distance=tiny))
    assert got == d.restated(gpu, l, tiny)
    assert all(r["inlier"] == 0 and r["outlier"] > 0 and r["cost"] == r["outlier"] * int(ps.q(F(tiny))) for r in got)
    small = 2.0 ** -8  # ... and one at which an outlier costs something: q = 4
    got = ps.as_ints(d.score(gpu, l, max_distance=small))
    assert got == d.restated(gpu, l, small)
    assert all(r["cost"] >= r["outlier"] * 4 > 0 and r["total"] == r["cost"] + r["invalid"] * 4 for r in got)
    # max_distance = 1024: q(max_distance) = 2^20, no overflow
    got = ps.as_ints(d.score(gpu, 0, max_distance=1024.0))
    assert got == d.restated(gpu, 0, 1024.0)
    assert all(r["total"] == r["cost"] + r["invalid"] * (1 << 20) for r in got) and max(r["total"] for r in got) > 1 << 26
    # invalid_distance = 0: total == cost
    got = ps.as_ints(d.score(gpu, l, invalid_distance=0.0))
    assert got == d.restated(gpu, l, invalid_distance=0.0) and all(r["total"] == r["cost"] for r in got)
    got = ps.as_ints(d.score(gpu, l, invalid_distance=2.5))
    assert got == d.restated(gpu, l, invalid_distance=2.5) and all(r["total"] == r["cost"] + r["invalid"] * 2560 for r in got)
    # a 180 degree turn about the axis between x and z swaps the optical axis with the x axis: (x, y, z) -> (z, -y, x), so that
    # |x' / z'| = |z / x| exceeds the half field of view for every pixel and all of them leave the image.  (A 180 degree turn
    # about x, y or z itself does not: the residual stage, like the reference's, has no test for the sign of the depth, and
    # (x, y, z) -> (-x, y, -z) projects to the same column -- the last lines hold the device to the rule there as well.)
    turn = synth.se3_exp(np.r_[0, 0, 0, np.pi * np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0)]) @ d.s["T_est"]
    for level in scored_levels(d.levels):
        r = ps.as_ints(d.score(gpu, level, Ts=[turn, d.s["T_est"]], invalid_distance=3.0))
        assert r[0]["inlier"] == r[0]["outlier"] == r[0]["cost"] == 0 and r[0]["invalid"] == r[0]["evaluated"] == int(d.evaluated[level].sum())
        assert r[0]["total"] == r[0]["invalid"] * 3072
        assert r[1] == d.restated(gpu, level, invalid_distance=3.0)[PLANTED]
    about_y = synth.se3_exp([0, 0, 0, 0, np.pi, 0]) @ d.s["T_est"]
    opt = gpu.residual_mask_options(None, d.levels, invalid_keep=1)
    for level in range(d.levels):
        opt.precision[level][:] = list(rm.precision_cm(d.o.P[l]))
    mask, _, distance = gpu.SelectionMask.from_residuals(d.tracker, d.reference, d.current, T=about_y, options=opt, counts=True, distance=True)
    want = ps.score_ref(outcome_of(d.evaluated[l], mask.download(l), distance[l]), distance[l])
    assert ps.as_ints(d.score(gpu, l, Ts=[about_y])) == [want] and want["invalid"] < want["evaluated"]


@pytest.mark.gpu
def test_many_equals_single_calls_and_two_calls_give_identical_bytes(gpu, device_scenes):
    a, b, c = device_scenes["80x48"], device_scenes["72x50"], device_scenes["64x32"]
    tile = gpu.POSE_SCORE_TILE
    pairs = [(a, a.options(gpu, 2), a.o.Ts), (b, b.options(gpu, 0, max_distance=3.0), b.o.Ts[:5]),
             (c, c.options(gpu, 2, invalid_distance=0.0), c.o.Ts[np.arange(tile + 3) % 27]),
             (a, a.options(gpu, 0, max_distance=100.0, invalid_distance=50.0), a.o.Ts[::-1]), (b, b.options(gpu, 1), b.o.Ts[13:14])]
    single = [d.tracker.score_poses(d.reference, d.current, Ts, o) for d, o, Ts in pairs]
    assert ps.as_ints(single[0]) == a.restated(gpu, 2) and ps.as_ints(single[4]) == [b.restated(gpu, 1)[13]]
    for order in (list(range(5)), [4, 2, 0, 3, 1], list(range(5))):
        many = a.tracker.score_poses_many([pairs[k][0].reference for k in order], [pairs[k][0].current for k in order],
                                          [pairs[k][2] for k in order], [pairs[k][1] for k in order])
        assert len(many) == 5
        for at, k in enumerate(order):
            assert many[at].tobytes() == single[k].tobytes(), (order, k)
    assert a.tracker.score_poses_many([], [], [], []) == []
    again = [d.tracker.score_poses(d.reference, d.current, Ts, o) for d, o, Ts in pairs]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(single, again))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIZES))
def test_the_planted_pose_ranks_first_on_the_device(gpu, device_scenes, name):
    d = device_scenes[name]
    coarsest = d.levels - 1
    records = d.score(gpu, coarsest)
    order = gpu.rank_poses(records, 5)
    assert order[0] == PLANTED and records["total"][order[0]] < records["total"][order[1]]
    assert order.tolist() == ps.rank_ref([r["total"] for r in d.restated(gpu, coarsest)], 5).tolist()
    assert order.tolist() == ps.rank_ref([r["total"] for r in d.o.restated(coarsest)], 5).tolist()


@pytest.mark.gpu
def test_refusals_and_what_the_call_leaves_alone(gpu, device_scenes):
    L = gpu.lib()
    a, b, other = device_scenes["80x48"], device_scenes["72x50"], device_scenes["64x32"]
    opt = a.options(gpu, 2)
    want = a.tracker.score_poses(a.reference, a.current, a.o.Ts, opt)
    beyond = gpu.pose_score_options(3, precision=rm.precision_cm(a.o.P[2]))
    for reference, current, o, word in ((a.reference, b.current, opt, "level"), (a.reference, other.current, opt, "in the current"),
                                        (a.reference, a.current, beyond, "level")):
        with pytest.raises(gpu.DvoAmdError) as err:
            a.tracker.score_poses(reference, current, a.o.Ts, o)
        assert err.value.status == INVALID and L.dvo_amd_last_error().decode().startswith("dvo_amd_score_poses_many: ")
        assert word in L.dvo_amd_last_error().decode()
    with pytest.raises(gpu.DvoAmdError) as err:  # one bad pair refuses the whole call
        a.tracker.score_poses_many([a.reference, a.reference], [a.current, b.current], [a.o.Ts, a.o.Ts], [opt, opt])
    assert err.value.status == INVALID
    # a tracker in the host-rcpps reciprocal mode is refused; back in the default mode it is served
    rcp = gpu.DenseTracker(a.cfg)
    rcp.set_reciprocal_mode("host_sse")
    with pytest.raises(gpu.DvoAmdError) as err:
        rcp.score_poses(a.reference, a.current, a.o.Ts, opt)
    assert err.value.status == INVALID and "reciprocal" in L.dvo_amd_last_error().decode()
    rcp.set_reciprocal_mode("exact")
    assert rcp.score_poses(a.reference, a.current, a.o.Ts, opt).tobytes() == want.tobytes()
    # the call needs no idle queue and holds no tracker state: a match submitted before it and waited on after it is the usual one;
    # the pyramids' planes and the context's configuration are what they were
    fresh_r, fresh_c = gpu.RgbdImagePyramid(*a.s["ref"], a.s["K"], 3), gpu.RgbdImagePyramid(*a.s["cur"], a.s["K"], 3)
    trk = gpu.DenseTracker(a.cfg)
    plain = trk.match(a.reference, a.current)
    before = [p.plane(l, k).copy() for p in (fresh_r, fresh_c) for l in range(3) for k in range(6)]
    cfg_before = gpu.CConfig()
    assert L.dvo_amd_get_config(trk._h, C.byref(cfg_before)) == 0
    submission = trk.submit([fresh_r], [fresh_c])
    during = trk.score_poses(fresh_r, fresh_c, a.o.Ts, opt)
    waited = trk.wait(submission)
    assert cases.same_result(waited[0], plain)
    assert during.tobytes() == want.tobytes()
    after = [p.plane(l, k) for p in (fresh_r, fresh_c) for l in range(3) for k in range(6)]
    assert all(rm.same_bits(x, y) for x, y in zip(before, after))
    cfg_after = gpu.CConfig()
    assert L.dvo_amd_get_config(trk._h, C.byref(cfg_after)) == 0
    assert bytes(cfg_before) == bytes(cfg_after)
    assert cases.same_result(trk.match(a.reference, a.current), plain)


@pytest.mark.gpu
def test_seed_proposals_carry_the_top_hypotheses_and_feed_the_validator(gpu, device_scenes):
    from dvo_slam_amd import constraints as cs

    a = device_scenes["80x48"]
    coarsest = a.levels - 1
    evaluation = lambda: cs.LogLikelihoodTrackingResultEvaluation(a.tracker.match(a.reference, a.current))  # noqa: E731
    keyframes = [cs.Keyframe(0, a.reference, np.eye(4), evaluation()), cs.Keyframe(1, a.current, np.eye(4), evaluation()),
                 cs.Keyframe(2, a.current, np.eye(4), evaluation())]
    opt = a.options(gpu, coarsest)
    k = 3
    proposals = cs.seed_proposals(a.tracker, keyframes, keyframes[0], [1, keyframes[2]], a.o.Ts, opt, k)
    assert len(proposals) == 2 * k
    records = a.tracker.score_poses(a.reference, a.current, a.o.Ts, opt)
    top = gpu.rank_poses(records, k)
    assert top[0] == PLANTED
    for c, candidate in enumerate((keyframes[1], keyframes[2])):
        for r in range(k):
            p = proposals[c * k + r]
            assert p.Reference is keyframes[0] and p.Current is candidate
            assert p.InitialTransformation.tobytes() == a.o.Ts[top[r]].tobytes(), (c, r)
    assert cs.seed_proposals(a.tracker, keyframes, keyframes[0], [], a.o.Ts, opt, k) == []
    # the list feeds the validator unchanged, next to proposalsForCandidates (no assertion on which survive)
    validator = cs.ConstraintProposalValidator(tracker=gpu.DenseTracker(a.cfg))
    stage_cfg = gpu.Config(FirstLevel=a.levels - 1, LastLevel=1, UseInitialEstimate=True, IntensityDerivativeThreshold=-1.0,
                           DepthDerivativeThreshold=-1.0)
    validator.createStage(1).trackingConfig(stage_cfg).keepAll().addVoter(cs.NaNResultVoter())
    survivors = validator.validate(proposals + cs.proposalsForCandidates(keyframes[0], [keyframes[1]]))
    assert isinstance(survivors, list) and all(isinstance(p, cs.ConstraintProposal) for p in survivors)
