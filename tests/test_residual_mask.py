"""Inlier masks from an alignment's residuals (include/dvo_amd.h, "Residual masks"): dvo_amd_mask_from_residuals / _many.  The
rule is pinned in the header and restated in tests/residual_mask_ref.py; every comparison in this file is equality -- of byte
planes, of integer counts, of float planes bit for bit (as uint32, NaN positions equal).  There is no tolerance anywhere.
CPU: the exports and the argument checks that need no device, the restatement against the oracle (its residuals, its weights),
the test scenes, the binding's level rule.  GPU: the library against the restatement fed with dvo_amd_residuals and, independently
of the library's own probe, with the oracle's residuals."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ops_ref  # noqa: E402
import residual_mask_ref as ref  # noqa: E402
import selection_mask_cases as cases  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_residual_mask_options", "dvo_amd_mask_from_residuals", "dvo_amd_mask_from_residuals_many"]
INVALID, NO_DEVICE = 1, 2
SIZES = {"80x48": (80, 48, 3), "72x50": (72, 50, 2), "64x32": (64, 32, 3)}  # (72x50: level 1 has the odd height 25)
KEEPS = [(0, 0), (1, 0), (0, 1), (1, 1)]  # (invalid_keep, unevaluated_keep)
# the kernel's tile (k_residual_mask, dvo_types.h): a lane owns 4 consecutive pixels of a row, a block of 256 lanes a chunk of
# 1024 consecutive pixels of the level in scan order (as k_mask_warp: there is no two-dimensional tile)
LANE_PIXELS, BLOCK = 4, 256
CHUNK = LANE_PIXELS * BLOCK


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


# ---- the scenes -----------------------------------------------------------------------------------------------------------------

def planted_rectangle(w, h):
    """(y0, y1, x0, x1) of the object planted into the current frame: a quarter of each side, off centre"""
    return h // 3, h // 3 + h // 4 + 1, w // 2, w // 2 + w // 4 + 1


def make_scene(synth, name):
    """A pair whose pose takes part of the reference out of the current image, NaN holes punched into both depth images, and an
    object planted into the current frame: a rectangle of its depth pushed 30 % farther (nearer, it would fail the occlusion test
    and be invalid, not an outlier) and of its intensity inverted.
    T_est = reference -> current, the estimate a perfect tracker would hold."""
    w, h, levels = SIZES[name]
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
    evaluated = ref.evaluated_ref(pr.plane(level, 1), pr.plane(level, 4), pr.plane(level, 5))
    _, res, valid = orc.compute_residuals(pr, pc, level, T, orc.RCP_EXACT, -1.0, -1.0)
    _, index = pr.select(level, -1.0, -1.0)
    assert np.array_equal(np.sort(index), np.flatnonzero(evaluated.ravel()))  # the validity selection is the predicate
    return evaluated, ref.residual_image((h, w), index, valid, res)


def oracle_precisions(orc, pr, pc, levels, T):
    """a precision per level as a tracker would hold it at T: the scale estimate of unit weights, then one robust round"""
    out = []
    for l in range(levels):
        first = orc.iteration(pr, pc, l, T, None, orc.RCP_EXACT, -1.0, -1.0)["precision"]
        out.append(orc.iteration(pr, pc, l, T, first, orc.RCP_EXACT, -1.0, -1.0)["precision"].astype(F))
    return out


@pytest.fixture(scope="module")
def scenes(synth):
    return {name: make_scene(synth, name) for name in SIZES}


@pytest.fixture(scope="module")
def oracle_scenes(orc, scenes):
    out = {}
    for name, s in scenes.items():
        pr, pc = orc.Pyramid(*s["ref"], s["K"], s["levels"]), orc.Pyramid(*s["cur"], s["K"], s["levels"])
        out[name] = dict(pr=pr, pc=pc, P=oracle_precisions(orc, pr, pc, s["levels"], s["T_est"]))
    return out


def rectangle_shares(outcome, w, h, level):
    """the outlier share of the evaluated pixels inside the planted rectangle (scaled to the level) and outside it"""
    y0, y1, x0, x1 = [v >> level for v in planted_rectangle(w, h)]
    inside = np.zeros(outcome.shape, bool)
    inside[y0:y1, x0:x1] = True
    evaluated = outcome != ref.UNEVALUATED
    share = lambda m: float(((outcome == ref.OUTLIER) & m).sum()) / max(1, int((evaluated & m).sum()))  # noqa: E731
    return share(inside), share(~inside)


# ---- CPU: exports and argument checks -------------------------------------------------------------------------------------------

def test_the_library_exports_the_entries_and_the_binding_covers_the_headers(capi):
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
    declared = set()
    for header in ("dvo_amd.h", "dvo_amd_debug.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared |= set(re.findall(r"\b(dvo_amd_[a-z0-9_]+)\s*\(", text))
    assert sorted(capi.EXPORTS) == sorted(declared)
    assert L.dvo_amd_abi_version() == 3
    assert capi.RESIDUAL_MASK_COUNTS == ref.COUNTS and capi.RESIDUAL_MASK_DTYPE.itemsize == 40
    assert F(capi.RESIDUAL_MASK_MAX_DISTANCE) == ref.MAX_DISTANCE
    header = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    assert "#define DVO_AMD_RESIDUAL_MASK_COUNTS 5" in header and "Residual masks" in header


def test_the_default_options_are_the_documented_ones(capi):
    opt = capi.ResidualMaskOptions()
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt))
    capi.lib().dvo_amd_default_residual_mask_options(C.byref(opt))
    assert C.sizeof(opt) == capi.MAX_LEVELS * 16 + capi.MAX_LEVELS * 4 + 8 == 168
    for l in range(capi.MAX_LEVELS):
        assert list(opt.precision[l]) == [0.0, 0.0, 0.0, 0.0]
        assert opt.max_distance[l] == F(9.2103)
    assert abs(-2.0 * np.log(0.01) - 9.2103) < 5e-5  # the 99 % point of chi-square with two degrees of freedom, to four places
    assert (opt.invalid_keep, opt.unevaluated_keep) == (0, 0)
    capi.lib().dvo_amd_default_residual_mask_options(None)  # a no-op


class Fakes:
    """zeroed buffers that stand for a context and two pyramids: an argument error is reported before any of them is looked at
    beyond its first words.  (refs, device, n_levels lead a pyramid: the reference gets one level so that its options are read)"""

    def __init__(self, capi):
        self.keep = [C.create_string_buffer(1 << 20) for _ in range(3)]
        self.ctx, self.ref, self.cur = [C.c_void_p(C.addressof(b)) for b in self.keep]
        C.c_int.from_buffer(self.keep[1], 8).value = 1
        C.c_int.from_buffer(self.keep[2], 8).value = 1
        self.T = (C.c_double * 16)(*np.eye(4).ravel())
        self.opt = capi.ResidualMaskOptions()
        capi.lib().dvo_amd_default_residual_mask_options(C.byref(self.opt))
        self.opt.precision[0][:] = [1500.0, 0.0, 0.0, 7000.0]


def _refused(L, entry, rc, handle, what, word=None):
    assert rc == INVALID, (entry, what, rc)
    assert not handle, (entry, what)
    reason = L.dvo_amd_last_error().decode()
    assert reason.startswith(entry + ": "), (entry, what, reason)
    if word:
        assert word in reason, (entry, what, reason)


def test_argument_errors_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    f = Fakes(capi)
    single, many = "dvo_amd_mask_from_residuals", "dvo_amd_mask_from_residuals_many"
    cnt = (C.c_longlong * 64)()
    opt = C.byref(f.opt)

    def call(ctx=f.ctx, reference=f.ref, current=f.cur, T=f.T, o=opt, with_out=True):
        h = C.c_void_p(0xDEAD)
        rc = L.dvo_amd_mask_from_residuals(ctx, reference, current, T, o, C.byref(h) if with_out else None, cnt, None)
        return rc, h.value if with_out else None

    for what, kw in {"ctx": dict(ctx=None), "reference": dict(reference=None), "current": dict(current=None), "T": dict(T=None),
                     "options": dict(o=None)}.items():
        _refused(L, single, *call(**kw), what, "NULL")
    assert call(with_out=False)[0] == INVALID
    one_r, one_c, null_in = (C.c_void_p * 1)(f.ref), (C.c_void_p * 1)(f.cur), (C.c_void_p * 1)(None)
    opts = (capi.ResidualMaskOptions * 1)(f.opt)

    def call_many(n=1, ctx=f.ctx, references=one_r, currents=one_c, T=f.T, o=opts, with_out=True):
        outs = (C.c_void_p * 1)(0xDEAD)
        rc = L.dvo_amd_mask_from_residuals_many(ctx, n, references, currents, T, o, outs if with_out else None, cnt)
        return rc, outs[0] if with_out else None

    for what, kw in {"ctx": dict(ctx=None), "references": dict(references=None), "currents": dict(currents=None), "T": dict(T=None),
                     "options": dict(o=None), "references[0]": dict(references=null_in), "currents[0]": dict(currents=null_in)}.items():
        _refused(L, many, *call_many(**kw), what, "NULL")
    assert call_many(with_out=False)[0] == INVALID
    _refused(L, many, call_many(n=-1)[0], None, "n < 0")  # (no output is touched: there is no telling how many there are)
    # a non-finite entry of T
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 7, 15):
            T = (C.c_double * 16)(*np.eye(4).ravel())
            T[at] = bad
            _refused(L, single, *call(T=T), (bad, at), "transformation")
            _refused(L, many, *call_many(T=T), (bad, at), "transformation")
    # the precision of a used level: not set, or not finite
    for what, P in {"unset": [0.0, 0.0, 0.0, 0.0], "nan": [1.0, np.nan, 0.0, 1.0], "inf": [np.inf, 0.0, 0.0, 1.0]}.items():
        bad = capi.ResidualMaskOptions.from_buffer_copy(f.opt)
        bad.precision[0][:] = P
        _refused(L, single, *call(o=C.byref(bad)), what, "precision not set" if what == "unset" else "precision")
        _refused(L, many, *call_many(o=(capi.ResidualMaskOptions * 1)(bad)), what, "precision")
    # max_distance: NaN or negative on any level
    for value, level in ((np.nan, 0), (-1.0, 0), (-np.inf, 3), (np.nan, capi.MAX_LEVELS - 1)):
        bad = capi.ResidualMaskOptions.from_buffer_copy(f.opt)
        bad.max_distance[level] = value
        _refused(L, single, *call(o=C.byref(bad)), (value, level), "max_distance")
    if L.dvo_amd_device_count() == 0:
        # nothing left to refuse: the device is looked for (+inf and 0 are allowed distances; an unused level's precision is not read)
        fine = capi.ResidualMaskOptions.from_buffer_copy(f.opt)
        fine.max_distance[0], fine.max_distance[1] = np.inf, 0.0
        fine.precision[1][:] = [np.nan] * 4
        rc, h = call(o=C.byref(fine))
        assert rc == NO_DEVICE and not h
        rc, h = call_many()
        assert rc == NO_DEVICE and not h
        assert call_many(n=0)[0] == NO_DEVICE  # (no pair: no output to clear)


# ---- CPU: the restatement against the oracle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SIZES))
def test_the_restatement_agrees_with_the_oracle(orc, scenes, oracle_scenes, name):
    """the residual-valid positions are the oracle's, and 7 / (5 + d) is the oracle's t-distribution weight for the same
    precision, bit for bit, in the exact-reciprocal mode: d is the quantity the tracker weights by"""
    s, o = scenes[name], oracle_scenes[name]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    for l in range(s["levels"]):
        evaluated, image = oracle_level(orc, o["pr"], o["pc"], l, s["T_est"])
        _, res, valid = orc.compute_residuals(o["pr"], o["pc"], l, s["T_est"], orc.RCP_EXACT, -1.0, -1.0)
        _, index = o["pr"].select(l, -1.0, -1.0)
        plane, distance, counts, outcome = ref.residual_mask_ref(evaluated, image, o["P"][l])
        has = ~np.isnan(distance)
        want = np.zeros(evaluated.size, bool)
        want[index[:len(valid)][valid.astype(bool)]] = True
        assert np.array_equal(has.ravel(), want) and counts["evaluated"] - counts["invalid"] == len(res) > 0, (name, l)
        assert len(valid) == len(index) - len(index) % 2  # Q3
        n = len(res)
        P = ref.precision_cm(o["P"][l])
        w, cov, P_out = np.zeros(n, F), np.zeros(4, F), np.zeros(4, F)
        orc.lib().orc_weights_scale_loglik(fp(np.ascontiguousarray(res)), n, fp(P), 0, orc.RCP_EXACT, fp(w), fp(cov), fp(P_out))
        d = distance.ravel()[index[:len(valid)][valid.astype(bool)]]  # in the oracle's order
        assert ref.same_bits(F(7.0) / (F(5.0) + d), w), (name, l)
        assert ref.same_bits(d, ref.distance_ref(res[:, 0], res[:, 1], P))


@pytest.mark.parametrize("name", sorted(SIZES))
def test_the_scenes_produce_every_outcome_on_every_level(orc, scenes, oracle_scenes, name):
    s, o = scenes[name], oracle_scenes[name]
    for l in range(s["levels"]):
        evaluated, image = oracle_level(orc, o["pr"], o["pc"], l, s["T_est"])
        _, _, counts, outcome = ref.residual_mask_ref(evaluated, image, o["P"][l])
        unevaluated = evaluated.size - counts["evaluated"]
        assert min(unevaluated, counts["invalid"], counts["inlier"], counts["outlier"]) > 0, (name, l, unevaluated, counts)
        inside, outside = rectangle_shares(outcome, s["w"], s["h"], l)
        print(f"{name} level {l}: outlier share inside the planted rectangle {inside:.3f}, outside {outside:.3f}; {counts}")
        assert inside > outside, (name, l, inside, outside)


class HandResult:
    def __init__(self, levels):
        self.Levels = [{"Id": l, "Iterations": [{"TDistributionPrecision": np.array([[l + 1.0, 0.5], [0.25, 10.0 * (l + 1) + k]])}
                                                 for k in range(n)]} for l, n in levels]
        self.Transformation = np.eye(4)


def test_residual_mask_options_takes_each_level_from_the_nearest_level_that_ran(capi):
    P = lambda l, k: [l + 1.0, 0.25, 0.5, 10.0 * (l + 1) + k]  # noqa: E731  column-major, the last iteration's
    r = HandResult([(3, 2), (2, 4), (1, 3)])  # the default configuration: level 0 does not run
    opt = capi.residual_mask_options(r, 4)
    assert [list(opt.precision[l]) for l in range(4)] == [P(1, 2), P(1, 2), P(2, 3), P(3, 1)]
    assert all(list(opt.precision[l]) == [0.0] * 4 for l in range(4, capi.MAX_LEVELS))
    assert all(opt.max_distance[l] == F(9.2103) for l in range(capi.MAX_LEVELS)) and (opt.invalid_keep, opt.unevaluated_keep) == (0, 0)
    r = HandResult([(4, 1), (3, 0), (1, 2)])  # level 3 recorded no iteration, levels 2 and 0 did not run: ties go to the finer level
    opt = capi.residual_mask_options(r, 5, max_distance=[1.0, 2.0], invalid_keep=1, unevaluated_keep=True)
    assert [list(opt.precision[l]) for l in range(5)] == [P(1, 1), P(1, 1), P(1, 1), P(4, 0), P(4, 0)]
    assert (opt.max_distance[0], opt.max_distance[1], opt.max_distance[2]) == (1.0, 2.0, F(9.2103))
    assert (opt.invalid_keep, opt.unevaluated_keep) == (1, 1)
    with pytest.raises(ValueError):
        capi.residual_mask_options(HandResult([(2, 0), (1, 0)]), 3)
    with pytest.raises(TypeError):
        capi.residual_mask_options(r, 3, unseen_keep=1)
    unset = capi.residual_mask_options(None, 3)
    assert all(list(unset.precision[l]) == [0.0] * 4 for l in range(capi.MAX_LEVELS))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


class DeviceScene:
    """a scene on the device: the pyramids, a tracker with the thresholds (-1, -1) for dvo_amd_residuals, the pose and the
    precisions of an actual match, two perturbed poses, and the restatements shared by the tests"""

    def __init__(self, capi, synth, s):
        self.s, self.levels = s, s["levels"]
        self.reference = capi.RgbdImagePyramid(*s["ref"], s["K"], self.levels)
        self.current = capi.RgbdImagePyramid(*s["cur"], s["K"], self.levels)
        self.cfg = capi.Config(FirstLevel=self.levels - 1, LastLevel=1 if self.levels > 1 else 0, IntensityDerivativeThreshold=-1.0,
                               DepthDerivativeThreshold=-1.0)
        self.tracker = capi.DenseTracker(self.cfg)
        self.result = self.tracker.match(self.reference, self.current)
        assert not self.result.isNaN()
        self.options = capi.residual_mask_options(self.result, self.levels)
        self.P = [np.array(list(self.options.precision[l]), F) for l in range(self.levels)]
        estimate = np.linalg.inv(self.result.Transformation)
        self.poses = {"match": estimate, "perturbed": synth.se3_exp(0.4 * synth.XI_GT_PAIR) @ estimate,
                      "far": synth.se3_exp(-2.5 * synth.XI_GT_PAIR) @ estimate}
        self.evaluated = [ref.evaluated_ref(*(self.reference.plane(l, k) for k in (1, 4, 5))) for l in range(self.levels)]
        self._res = {}

    def residuals(self, pose):
        """dvo_amd_residuals of every level at the pose (computed once, shared)"""
        if pose not in self._res:
            self._res[pose] = [self.tracker.residuals(self.reference, self.current, l, self.poses[pose])[0] for l in range(self.levels)]
        return self._res[pose]

    def restated(self, images, max_distance=None, keeps=(0, 0)):
        md = [ref.MAX_DISTANCE] * self.levels if max_distance is None else max_distance
        return [ref.residual_mask_ref(self.evaluated[l], images[l], self.P[l], md[l], *keeps) for l in range(self.levels)]

    def call(self, capi, pose, max_distance=None, keeps=(0, 0), **kw):
        opt = capi.ResidualMaskOptions.from_buffer_copy(self.options)
        if max_distance is not None:
            for l, v in enumerate(max_distance):
                opt.max_distance[l] = v
        opt.invalid_keep, opt.unevaluated_keep = keeps
        return capi.SelectionMask.from_residuals(self.tracker, self.reference, self.current, T=self.poses[pose], options=opt, **kw)


@pytest.fixture(scope="module")
def device_scenes(gpu, synth, scenes):
    return {name: DeviceScene(gpu, synth, scenes[name]) for name in SIZES}


def _counts(records):
    return [{k: int(r[k]) for k in ref.COUNTS} for r in records]


def _same(mask, want, what):
    info = mask.info()
    assert info["levels"] == len(want), what
    for l, p in enumerate(want):
        got = mask.download(l)
        assert got.shape == p.shape and np.array_equal(got, p), (what, l)
    assert info["kept"] == [int(p.sum()) for p in want], what


def _assert_equals_restatement(gpu, d, images, what):
    for pose in d.poses:
        for keeps in KEEPS:
            want = d.restated(images[pose], keeps=keeps)
            mask, counts, distance = d.call(gpu, pose, keeps=keeps, counts=True, distance=True)
            for l in range(d.levels):
                assert ref.same_bits(distance[l], want[l][1]), (what, pose, keeps, l)
            _same(mask, [w[0] for w in want], (what, pose, keeps))
            assert _counts(counts) == [w[2] for w in want], (what, pose, keeps)
            assert [c["kept"] for c in _counts(counts)] == mask.info()["kept"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIZES))
def test_planes_equal_the_restatement_of_dvo_amd_residuals(gpu, device_scenes, name):
    d = device_scenes[name]
    images = {pose: d.residuals(pose) for pose in d.poses}
    # at the pose of the match every outcome occurs on every level of the device's own planes, and each keep decides some pixel
    for l, (_, _, counts, _) in enumerate(d.restated(images["match"])):
        assert min(d.evaluated[l].size - counts["evaluated"], counts["invalid"], counts["inlier"], counts["outlier"]) > 0, (name, l, counts)
    _assert_equals_restatement(gpu, d, images, name)
    assert d.call(gpu, "match").info()["kept"] == [w[2]["kept"] for w in d.restated(images["match"])]  # the mask alone


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIZES))
def test_planes_equal_the_restatement_of_the_oracle(gpu, orc, device_scenes, oracle_scenes, name):
    """the same comparison fed with the oracle's residuals: independent of the library's own probe"""
    d, o = device_scenes[name], oracle_scenes[name]
    images = {}
    for pose, T in d.poses.items():
        levels = [oracle_level(orc, o["pr"], o["pc"], l, T) for l in range(d.levels)]
        assert all(np.array_equal(e, d.evaluated[l]) for l, (e, _) in enumerate(levels))
        images[pose] = [image for _, image in levels]
    _assert_equals_restatement(gpu, d, images, name)


@pytest.mark.gpu
def test_the_limits_of_max_distance(gpu, device_scenes):
    d = device_scenes["80x48"]
    images = d.residuals("match")
    inf, zero = [np.inf] * d.levels, [0.0] * d.levels
    for keeps in KEEPS:
        mask, counts = d.call(gpu, "match", max_distance=inf, keeps=keeps, counts=True)
        for l in range(d.levels):
            valid = ~np.isnan(images[l][..., 0])
            want = valid.astype(np.uint8)
            want[d.evaluated[l] & ~valid] = keeps[0]
            want[~d.evaluated[l]] = keeps[1]
            assert np.array_equal(mask.download(l), want), (keeps, l)
            assert _counts(counts)[l]["outlier"] == 0 and _counts(counts)[l]["inlier"] == int(valid.sum())
    _same(d.call(gpu, "match", max_distance=inf), [w[0] for w in d.restated(images, inf)], "inf")
    # 0 keeps only the pixels whose distance is exactly 0
    mask, counts, distance = d.call(gpu, "match", max_distance=zero, counts=True, distance=True)
    for l in range(d.levels):
        assert np.array_equal(mask.download(l), (distance[l] == 0).astype(np.uint8)), l
    _same(mask, [w[0] for w in d.restated(images, zero)], "zero")
    # the masks for increasing distances are nested, and strictly so somewhere
    steps = [0.0, 0.5, 2.0, 9.2103, 50.0, np.inf]
    planes = []
    for v in steps:
        m = d.call(gpu, "match", max_distance=[v] * d.levels)
        _same(m, [w[0] for w in d.restated(images, [v] * d.levels)], v)
        planes.append([m.download(l) for l in range(d.levels)])
    for a, b in zip(planes, planes[1:]):
        assert all((x <= y).all() for x, y in zip(a, b))
    assert all(int(planes[0][l].sum()) < int(planes[-1][l].sum()) for l in range(d.levels))


@pytest.mark.gpu
def test_across_the_kernel_chunks(gpu, synth, orc):
    """one plain single-level pair of 212x150: 31 800 pixels are 31 chunks of 1024 and a ragged last one of 56; a row of 212 pixels
    is 53 lanes, so rows straddle waves and chunks at every offset (a chunk is 4.83 rows: it spans columns and rows); the width is
    a multiple of 4 as every level's must be (check_levels), so a lane's four pixels never leave their row"""
    w, h = 212, 150
    assert w * h > 2 * CHUNK and (w * h) % CHUNK != 0 and CHUNK % w != 0 and w % LANE_PIXELS == 0 and w <= 320 and h <= 240
    K = synth.intrinsics_for(w, h)
    (Ir, Zr), (Ic, Zc), T_gt = synth.make_pair(w, h, xi_gt=2.0 * synth.XI_GT_PAIR)
    T = np.linalg.inv(T_gt)
    reference, current = gpu.RgbdImagePyramid(Ir, Zr, K, 1), gpu.RgbdImagePyramid(Ic, Zc, K, 1)
    tracker = gpu.DenseTracker(gpu.Config(FirstLevel=0, LastLevel=0, IntensityDerivativeThreshold=-1.0, DepthDerivativeThreshold=-1.0))
    pr, pc = orc.Pyramid(Ir, Zr, K, 1), orc.Pyramid(Ic, Zc, K, 1)
    evaluated, image = oracle_level(orc, pr, pc, 0, T)
    assert np.array_equal(evaluated, ref.evaluated_ref(*(reference.plane(0, k) for k in (1, 4, 5))))
    assert ref.same_bits(tracker.residuals(reference, current, 0, T)[0], image)
    P = oracle_precisions(orc, pr, pc, 1, T)[0]
    opt = gpu.residual_mask_options(None, 1, max_distance=3.0, invalid_keep=1)
    opt.precision[0][:] = list(ref.precision_cm(P))
    plane, distance, counts, outcome = ref.residual_mask_ref(evaluated, image, P, 3.0, 1, 0)
    assert min(counts["invalid"], counts["inlier"], counts["outlier"]) > 0
    for c in range(0, w * h, CHUNK):  # every chunk holds evaluated pixels and more than one outcome
        assert len(set(outcome.ravel()[c:c + CHUNK].tolist())) > 1, c
    mask, got_counts, got_distance = gpu.SelectionMask.from_residuals(tracker, reference, current, T=T, options=opt, counts=True,
                                                                      distance=True)
    assert ref.same_bits(got_distance[0], distance)
    _same(mask, [plane], "chunks")
    assert _counts(got_counts) == [counts]


@pytest.mark.gpu
def test_an_odd_number_of_evaluated_pixels_leaves_the_last_one_invalid(gpu, synth):
    """Q3: the tracker's point list never reaches an odd trailing point, so dvo_amd_residuals has no residual there.  The same
    pair with one more NaN in the reference's depth flips the parity of every level it reaches."""
    w, h, levels = 80, 48, 3
    K = synth.intrinsics_for(w, h)
    (Ir, Zr), (Ic, Zc), T_gt = synth.make_pair(w, h)
    T = np.linalg.inv(T_gt)
    tracker = gpu.DenseTracker(gpu.Config(FirstLevel=2, LastLevel=0, IntensityDerivativeThreshold=-1.0, DepthDerivativeThreshold=-1.0))
    opt = gpu.residual_mask_options(None, levels, max_distance=np.inf)
    for l in range(levels):
        opt.precision[l][:] = [1500.0, 0.0, 0.0, 7000.0]
    seen = set()
    for extra_nan in (False, True):
        Z = Zr.copy()
        if extra_nan:
            Z[20, 40] = np.nan  # (an even pixel: it is a pixel of every level)
        reference, current = gpu.RgbdImagePyramid(Ir, Z, K, levels), gpu.RgbdImagePyramid(Ic, Zc, K, levels)
        mask, counts, distance = gpu.SelectionMask.from_residuals(tracker, reference, current, T=T, options=opt, counts=True, distance=True)
        for l in range(levels):
            evaluated = ref.evaluated_ref(*(reference.plane(l, k) for k in (1, 4, 5)))
            image = tracker.residuals(reference, current, l, T)[0]
            plane, want_d, want_c, _ = ref.residual_mask_ref(evaluated, image, [1500.0, 0.0, 0.0, 7000.0], np.inf)
            assert ref.same_bits(distance[l], want_d) and np.array_equal(mask.download(l), plane) and _counts(counts)[l] == want_c, (extra_nan, l)
            odd = int(evaluated.sum()) % 2 == 1
            seen.add(odd)
            if odd:
                last = np.flatnonzero(evaluated.ravel())[-1]
                assert np.isnan(distance[l].ravel()[last]) and mask.download(l).ravel()[last] == 0
    assert seen == {False, True}


@pytest.mark.gpu
def test_many_equals_single_calls(gpu, synth, device_scenes):
    a, b, c = device_scenes["80x48"], device_scenes["72x50"], device_scenes["64x32"]

    def options(d, **kw):
        opt = gpu.ResidualMaskOptions.from_buffer_copy(d.options)
        for k, v in kw.items():
            if k == "max_distance":
                for l in range(gpu.MAX_LEVELS):
                    opt.max_distance[l] = v
            else:
                setattr(opt, k, v)
        return opt

    pairs = [(a, "match", options(a)), (b, "perturbed", options(b, invalid_keep=1)), (c, "far", options(c, max_distance=2.0)),
             (a, "far", options(a, unevaluated_keep=1, max_distance=np.inf)), (b, "match", options(b, max_distance=0.5, invalid_keep=1))]
    single = [gpu.SelectionMask.from_residuals(d.tracker, d.reference, d.current, T=d.poses[p], options=o, counts=True) for d, p, o in pairs]
    for order in (list(range(5)), [4, 2, 0, 3, 1], list(range(5))):
        masks, counts = gpu.SelectionMask.from_residuals_many(a.tracker, [pairs[k][0].reference for k in order],
                                                              [pairs[k][0].current for k in order],
                                                              Ts=[pairs[k][0].poses[pairs[k][1]] for k in order],
                                                              options=[pairs[k][2] for k in order], counts=True)
        assert len(masks) == len(counts) == 5
        for at, k in enumerate(order):
            want = single[k][0]
            _same(masks[at], [want.download(l) for l in range(want.info()["levels"])], (order, k))
            assert masks[at].info() == want.info()
            assert _counts(counts[at]) == _counts(single[k][1]), (order, k)
    assert gpu.SelectionMask.from_residuals_many(a.tracker, [], [], Ts=[], options=[]) == []
    # result= in the place of T and of the options: the inverse of the transformation the match returned, its precisions
    from_result = gpu.SelectionMask.from_residuals_many(a.tracker, [a.reference, b.reference], [a.current, b.current], results=[a.result, b.result])
    for m, d in zip(from_result, (a, b)):
        want = gpu.SelectionMask.from_residuals(d.tracker, d.reference, d.current, result=d.result)
        _same(m, [want.download(l) for l in range(d.levels)], "result=")
        _same(m, [w[0] for w in d.restated(d.residuals("match"))], "result= against the restatement")


@pytest.mark.gpu
def test_the_result_is_an_ordinary_mask(gpu, device_scenes):
    """info / download, match_masked and match_many_masked behind it, &, erode and warp of it: each agrees with its restatement"""
    d = device_scenes["80x48"]
    want = [w[0] for w in d.restated(d.residuals("match"))]
    inliers = d.call(gpu, "match")
    _same(inliers, want, "inliers")
    assert inliers.info()["width"] == 80 and inliers.info()["height"] == 48 and inliers.info()["levels"] == 3
    uploaded = gpu.SelectionMask.from_levels(want)
    trk = d.tracker
    got = trk.match(d.reference, d.current, mask=inliers)
    assert not got.isNaN() and cases.same_result(got, trk.match(d.reference, d.current, mask=uploaded))
    assert not cases.same_result(got, d.result)  # the mask changed the alignment
    many = trk.match_batch([d.reference, d.reference], [d.current, d.current], masks=[inliers, None])
    assert cases.same_result(many[0], got) and cases.same_result(many[1], d.result)
    rect = np.zeros((48, 80), np.uint8)
    rect[8:40, 10:70] = 1
    _same(inliers & gpu.SelectionMask.from_level0(rect, 3),
          [mask_ops_ref.combine_ref(p, q, mask_ops_ref.AND) for p, q in zip(want, cases.mask_pyramid(rect, 3, False))], "&")
    _same(inliers.erode(1), [mask_ops_ref.morph_ref(p, mask_ops_ref.ERODE, r) for p, r in zip(want, mask_ops_ref.level_radii(1, 3))], "erode")
    T = d.result.Transformation  # current (target) -> reference (source): as the match returned it
    warped, counts = inliers.warp(d.reference, d.current, T, counts=True)
    restated = [mask_ops_ref.warp_ref(want[l], (d.current.plane(l, 1), tuple(d.current.level_info(l)[2])),
                                      (d.reference.plane(l, 1), tuple(d.reference.level_info(l)[2])), T) for l in range(3)]
    _same(warped, [p for p, _ in restated], "warp")
    assert [{k: int(r[k]) for k in mask_ops_ref.WARP_COUNTS} for r in counts] == [c for _, c in restated]


@pytest.mark.gpu
def test_keeping_everything_gives_the_unmasked_alignment(gpu, device_scenes):
    for name in sorted(SIZES):
        d = device_scenes[name]
        everything = d.call(gpu, "match", max_distance=[np.inf] * d.levels, keeps=(1, 1))
        info = everything.info()
        assert info["kept"] == [(d.s["w"] >> l) * (d.s["h"] >> l) for l in range(d.levels)]
        assert cases.same_result(d.tracker.match(d.reference, d.current, mask=everything), d.result), name


@pytest.mark.gpu
def test_refusals_and_what_the_call_leaves_alone(gpu, device_scenes):
    L = gpu.lib()
    a, b = device_scenes["80x48"], device_scenes["72x50"]

    def raw(tracker, reference, current, T, opt):
        h = C.c_void_p(0xDEAD)
        Tc = np.ascontiguousarray(np.asarray(T, np.float64).T)
        rc = L.dvo_amd_mask_from_residuals(tracker._h, reference._h, current._h, Tc.ctypes.data_as(C.POINTER(C.c_double)), C.byref(opt),
                                           C.byref(h), None, None)
        assert rc == 0 or not h.value
        if rc == 0:
            L.dvo_amd_mask_release(h)
        return rc

    T = a.poses["match"]
    assert raw(a.tracker, a.reference, a.current, T, a.options) == 0  # (counts and distance may be NULL)
    assert raw(a.tracker, a.reference, b.current, T, a.options) == INVALID  # a current with fewer levels and another size
    assert L.dvo_amd_last_error().decode().startswith("dvo_amd_mask_from_residuals: ")
    shallow = gpu.RgbdImagePyramid(*a.s["cur"], a.s["K"], 2)
    assert raw(a.tracker, a.reference, shallow, T, a.options) == INVALID and "levels" in L.dvo_amd_last_error().decode()
    assert raw(a.tracker, shallow, a.current, T, a.options) == 0  # the reference's levels count: a deeper current is fine
    other = device_scenes["64x32"]
    assert raw(a.tracker, a.reference, other.current, T, a.options) == INVALID  # same level count, another size
    unset = gpu.residual_mask_options(None, 3)
    assert raw(a.tracker, a.reference, a.current, T, unset) == INVALID and "precision not set" in L.dvo_amd_last_error().decode()
    with pytest.raises(gpu.DvoAmdError) as err:
        gpu.SelectionMask.from_residuals_many(a.tracker, [a.reference, a.reference], [a.current, b.current], Ts=[T, T],
                                              options=[a.options, a.options])
    assert err.value.status == INVALID  # one bad pair refuses the whole call
    # a tracker in the host-rcpps reciprocal mode is refused; back in the default mode it is served
    rcp = gpu.DenseTracker(a.cfg)
    rcp.set_reciprocal_mode("host_sse")
    assert raw(rcp, a.reference, a.current, T, a.options) == INVALID and "reciprocal" in L.dvo_amd_last_error().decode()
    rcp.set_reciprocal_mode("exact")
    assert raw(rcp, a.reference, a.current, T, a.options) == 0
    # the call builds no selection and needs no idle queue: a match submitted before and waited on after it is the usual one, and a
    # pyramid that has never been selected on still accepts its full number of masked selections afterwards
    fresh_r, fresh_c = gpu.RgbdImagePyramid(*a.s["ref"], a.s["K"], 3), gpu.RgbdImagePyramid(*a.s["cur"], a.s["K"], 3)
    trk = gpu.DenseTracker(a.cfg)
    submission = trk.submit([fresh_r], [fresh_c])
    mask = gpu.SelectionMask.from_residuals(trk, fresh_r, fresh_c, T=T, options=a.options)
    assert gpu.SelectionMask.from_residuals_many(trk, [fresh_r], [fresh_c], Ts=[T], options=[a.options])[0].info() == mask.info()
    waited = trk.wait(submission)
    assert cases.same_result(waited[0], a.result)
    _same(mask, [w[0] for w in a.restated(a.residuals("match"))], "while a match was queued")
    for k in range(gpu.MAX_MASKED_SELECTIONS):
        keep = np.ones((48, 80), np.uint8)
        keep[k, k] = 0
        fresh_r.select(0, -1.0, -1.0, mask=gpu.SelectionMask.from_level0(keep, 3))
