"""Depth filtering on the device (include/dvo_amd.h, "Depth filtering"): dvo_amd_pyramid_filter_depth and
dvo_amd_pyramid_filter_depth_many.  The rule is pinned in the header and restated in tests/depth_filter_ref.py.  Every comparison with
the library is equality -- of float planes bit for bit (NaN positions included), of support planes, of integer counts, of tracking
results.  The inequalities are the denoising bars, measured by the restatement on the CPU.
CPU: exports and layout, the argument checks that need no device, the restatement against its pixel loop, the coverage of the
scenes, the denoising.  GPU: the library against the restatement.

The figures behind the CPU bars (measured with the restatement on synth.sensor_frame(160, 120)):
  depth:   RMS error against synth.render's analytic depth over the 18 724 pixels where both are finite: raw 13.90 mm; radius 2,
           3 sigmas: 7.72 mm (ratio 0.556: the bar is sqrt(1 * 0.556) = 0.745); radius 4, 3 sigmas: 6.87 mm; radius 4, 5 sigmas: 5.14 mm
  normals: mean angle of normals_ref's r = 0 normals to the analytic ones over the 1 190 pixels of the interior eroded by 4 (the
           set of DESIGN.md 4.18): raw 27.42 degrees; on the plane filtered at radius 2, 3 sigmas: 12.84; at radius 4: 10.55
  pose:    synth.sensor_pair(640, 480), four levels, error against the ground truth on an MI355X: raw 5.680e-4, both pyramids
           filtered with the defaults 3.534e-4 (the bar is 1e-3 for both; the two are not compared)"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_filter_ref as ref  # noqa: E402
import normals_ref as nref  # noqa: E402
import selection_mask_cases as cases  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_depth_filter_options", "dvo_amd_pyramid_filter_depth", "dvo_amd_pyramid_filter_depth_many",
               "dvo_amd_debug_depth_filter_timing"]
INVALID, NO_DEVICE, MISMATCH = 1, 2, 8
# the options of the parity test: radius x min_support (a window of one pixel allows min_support 1 only) x (fill_radius)
WINDOWS = [(0, 1), (1, 1), (1, 4), (2, 1), (2, 4), (8, 1), (8, 4)]
FILLS = [0, 1, 8]
# the options under which the scenes must reach every count
COVERAGE = [dict(radius=2, min_support=4, fill_radius=1), dict(radius=1, min_support=4, fill_radius=8)]


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


# ---- CPU: exports and layout ------------------------------------------------------------------------------------------------------

def test_the_library_exports_the_entries_and_the_binding_covers_the_headers(capi):
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
    declared = set()
    for header in ("dvo_amd.h", "dvo_amd_debug.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared |= set(re.findall(r"\b(dvo_amd_[a-z0-9_]+)\s*\(", text))
    assert set(NEW_SYMBOLS) <= declared and sorted(capi.EXPORTS) == sorted(declared)
    assert L.dvo_amd_abi_version() == 3
    assert capi.DEPTH_FILTER_MAX_RADIUS == ref.MAX_RADIUS == 8
    assert capi.DEPTH_FILTER_COUNTS == ref.COUNTS and capi.DEPTH_FILTER_DTYPE.itemsize == 40
    header = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    for define, value in (("DVO_AMD_DEPTH_FILTER_MAX_RADIUS", 8), ("DVO_AMD_DEPTH_FILTER_COUNTS", 5)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define
    assert callable(capi.RgbdImagePyramid.filter_depth) and callable(capi.filter_depth_many) and callable(capi.depth_filter_timing)


def test_the_default_options_are_the_documented_ones(capi):
    opt = capi.DepthFilterOptions()
    assert C.sizeof(opt) == 20
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt))
    capi.lib().dvo_amd_default_depth_filter_options(C.byref(opt))
    assert (opt.radius, opt.range_sigmas, opt.min_support, opt.fill_radius, opt.min_fill_support) == (2, 3.0, 1, 0, 3)
    for k, v in ref.DEFAULTS.items():  # the restatement's defaults are the library's
        assert F(getattr(opt, k)) == F(v), k
    capi.lib().dvo_amd_default_depth_filter_options(None)  # a no-op
    assert capi.depth_filter_options(radius=4, range_sigmas=5).range_sigmas == 5.0
    with pytest.raises(TypeError):
        capi.depth_filter_options(sigma=1)


# ---- CPU: the argument checks -----------------------------------------------------------------------------------------------------

class Fakes:
    """zeroed buffers that stand for pyramids (refs, device, n_levels lead a pyramid): an argument error is reported before any of
    them is looked at beyond its device"""

    def __init__(self, n=3):
        self.keep = [C.create_string_buffer(1 << 16) for _ in range(n)]
        for b in self.keep:
            C.c_int.from_buffer(b, 8).value = 1
        self.one = C.c_void_p(C.addressof(self.keep[0]))
        self.all = (C.c_void_p * n)(*[C.addressof(b) for b in self.keep])
        self.n = n

    def on_device(self, k, device):
        C.c_int.from_buffer(self.keep[k], 4).value = device


def test_argument_errors_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    f = Fakes()
    single, many = "dvo_amd_pyramid_filter_depth", "dvo_amd_pyramid_filter_depth_many"
    cnt = (C.c_longlong * 16)()
    good = capi.depth_filter_options()

    def call(p=f.one, opt=good, with_out=True):
        h = C.c_void_p(0xDEAD)
        rc = L.dvo_amd_pyramid_filter_depth(p, None if opt is None else C.byref(opt), C.byref(h) if with_out else None, cnt, None)
        return rc, h.value if with_out else None

    def call_many(n=f.n, p=f.all, opt=good, with_out=True):
        outs = (C.c_void_p * 3)(0xDEAD, 0xDEAD, 0xDEAD)
        rc = L.dvo_amd_pyramid_filter_depth_many(n, p, None if opt is None else C.byref(opt), outs if with_out else None, cnt, None)
        return rc, (outs[0] or outs[1] or outs[2]) if with_out else None

    def refused(entry, got, what, word=None):
        rc, handle = got
        assert rc == INVALID, (entry, what, rc)
        assert not handle, (entry, what)
        reason = L.dvo_amd_last_error().decode()
        assert reason.startswith(entry + ": "), (entry, what, reason)
        assert word is None or word in reason, (entry, what, reason)

    refused(single, call(p=None), "pyramid", "NULL")
    refused(single, call(opt=None), "options", "NULL")
    assert call(with_out=False)[0] == INVALID
    refused(many, call_many(p=None), "pyramids", "NULL")
    refused(many, call_many(opt=None), "options", "NULL")
    refused(many, call_many(p=(C.c_void_p * 3)(f.all[0], None, f.all[2])), "pyramids[1]", "NULL")
    assert call_many(with_out=False)[0] == INVALID
    refused(many, (call_many(n=-1)[0], None), "n < 0", "negative")  # (a negative count names no output to clear)
    bad = [("radius", -1, {}), ("radius", 9, {}), ("fill_radius", -1, {}), ("fill_radius", 9, {}),
           ("range_sigmas", 0.0, {}), ("range_sigmas", -1.0, {}), ("range_sigmas", np.nan, {}), ("range_sigmas", np.inf, {}),
           ("min_support", 0, {}), ("min_support", 26, {}), ("min_support", 2, dict(radius=0)), ("min_support", 290, dict(radius=8)),
           ("min_fill_support", 0, dict(fill_radius=1)), ("min_fill_support", 10, dict(fill_radius=1)),
           ("min_fill_support", 290, dict(fill_radius=8))]
    for field, value, more in bad:
        opt = capi.depth_filter_options(**dict(more, **{field: value}))
        refused(single, call(opt=opt), (field, value), field)
        refused(many, call_many(opt=opt), (field, value), field)
    # the order: an argument error comes before a device mismatch, and a mismatch before the device is looked for
    f.on_device(2, 1)
    refused(many, call_many(opt=capi.depth_filter_options(radius=9)), "a bad radius on two devices", "radius")
    assert call_many() == (MISMATCH, None)
    f.on_device(2, 0)
    # legal at their edges (min_fill_support is not read without a fill): nothing left to refuse, the device is looked for
    if L.dvo_amd_device_count() == 0:
        for kw in (dict(radius=0, min_support=1), dict(radius=8, min_support=289), dict(min_fill_support=0), dict(min_fill_support=99),
                   dict(fill_radius=8, min_fill_support=289), dict(range_sigmas=1e-3)):
            assert call(opt=capi.depth_filter_options(**kw)) == (NO_DEVICE, None), kw
        assert call_many() == (NO_DEVICE, None)
        assert call_many(n=0) == (NO_DEVICE, 0xDEAD)  # (no output is touched where there is none)


# ---- CPU: the restatement, the scenes, the denoising --------------------------------------------------------------------------------

def test_the_restatement_matches_the_pixel_loop():
    """on every scene; the 160x120 frame with windows of 25 and 9, the small ones with the widest windows too"""
    for name, (_, Z, _, _) in ref.scenes().items():
        options = [dict(radius=2, min_support=4, fill_radius=1), dict(radius=1, range_sigmas=5.0, fill_radius=2, min_fill_support=1)]
        if name != "sensor":
            options += [dict(radius=8, min_support=4, fill_radius=8), dict(radius=0), dict(radius=3, min_support=49, fill_radius=1, min_fill_support=9)]
        for opt in options:
            a, b = ref.filter_ref(Z, **opt), ref.filter_loop(Z, **opt)
            assert ref.same(a, b), (name, opt)
            c = a[2]
            assert c["with_depth"] == c["kept"] + c["dropped"] == int(np.isfinite(Z).sum()) and c["filled"] <= c["holes"]
            assert c["with_depth"] + c["holes"] == Z.size and int((a[1] > 0).sum()) == c["with_depth"] and a[1].max() <= 289
            assert int(np.isfinite(a[0]).sum()) == c["kept"] + c["filled"]
            nans = ref.bits(a[0])[np.isnan(a[0])]
            assert (nans == 0x7FC00000).all()


def test_the_scenes_reach_every_count_and_every_tile_edge():
    S = ref.scenes()
    assert sorted((Z.shape[1], Z.shape[0]) for _, Z, _, _ in S.values()) == [(4, 2), (20, 12), (33, 9), (36, 9), (68, 36), (160, 120)]
    assert set(ref.DEVICE_SCENES) == set(S) - {"past"}
    for name in S:
        seen = dict.fromkeys(ref.COUNTS, 0)
        for opt in COVERAGE:
            for k, v in ref.scene_ref(name, **opt)[2].items():
                seen[k] += v
        print(name, seen)
        if name in ("sensor", "small", "past", "past36"):  # each of them reaches every count on its own
            assert all(v > 0 for v in seen.values()), (name, seen)
    for name in ("small", "past36"):  # rows, columns and blocks without depth
        Z = S[name][1]
        assert np.isnan(Z).all(axis=1).any()
    assert np.isnan(S["small"][1]).all(axis=0).any() and np.isnan(S["tiny"][1]).all(axis=0).any()
    assert np.isnan(S["sensor"][1][40:50, 106:116]).all()


def _sensor_truth(synth):
    Z = ref.scenes()["sensor"][1]
    truth = synth.render(160, 120, np.eye(4), nan_fraction=0, hole=False)[1]
    return Z, truth, np.isfinite(Z) & np.isfinite(truth)


def test_the_filter_lowers_the_depth_error_of_a_sensor_frame(synth):
    """the bar is the geometric mean of 1 and the ratio the restatement measured (module docstring): sqrt(0.556) = 0.745"""
    Z, truth, both = _sensor_truth(synth)
    assert both.sum() == 18724

    def rms(z):
        assert np.isfinite(z[both]).all()
        return float(np.sqrt(np.mean((z[both].astype(np.float64) - truth[both]) ** 2)))

    raw, r2, r4 = rms(Z), rms(ref.scene_ref("sensor", radius=2)[0]), rms(ref.scene_ref("sensor", radius=4)[0])
    wide = rms(ref.scene_ref("sensor", radius=4, range_sigmas=5.0)[0])
    print("rms: raw %.2f mm, radius 2 / 3 sigmas %.2f mm (ratio %.3f), radius 4 / 3 sigmas %.2f mm, radius 4 / 5 sigmas %.2f mm"
          % (1e3 * raw, 1e3 * r2, r2 / raw, 1e3 * r4, 1e3 * wide))
    assert r2 < 0.745 * raw, (raw, r2)
    assert r4 <= r2, (r2, r4)
    assert np.array_equal(ref.bits(ref.scene_ref("sensor", radius=0)[0]), ref.bits(Z))  # radius 0: the input, bit for bit


def test_the_filter_lowers_the_normal_error_of_a_sensor_frame(synth):
    """normals_ref's r = 0 normals over the interior eroded by 4, the set behind DESIGN.md 4.18's 27.4 degrees"""
    Z = ref.scenes()["sensor"][1]
    K = synth.intrinsics_for(160, 120)
    which = nref.corner_planes(160, 120, K)
    deep = nref.erode(nref.interior(synth.render(160, 120)[1], which), 4)
    assert deep.sum() == 1190

    def mean_angle(z):
        err = nref.angle_deg(nref.normals_ref(z, K, 0)[0], which)[deep]
        assert not np.isnan(err).any()
        return float(err.mean())

    raw, filtered = mean_angle(Z), mean_angle(ref.scene_ref("sensor", radius=2)[0])
    print("mean angle over %d pixels: raw %.2f degrees, filtered (radius 2, 3 sigmas) %.2f degrees" % (deep.sum(), raw, filtered))
    assert filtered < raw


def test_an_edge_is_kept_and_its_flying_pixels_are_what_is_dropped():
    """(the restatement's side of the GPU test of the same name)"""
    for w, h, radii in ((68, 20, (1, 2, 3)), (68, 8, (8,))):
        _edge_case(lambda Z, **opt: ref.filter_ref(Z, **opt), w, h, radii)


def _edge_case(run, w, h, radii):
    """run(Z, **opt) -> (filtered, support, counts).  Two planes at 1.0 and 1.5 m that meet at column 33, one past a tile border"""
    clean = ref.step_plane(w, h, 33, flying=False)
    for r in (0, 1, 2, 8):
        out, _, c = run(clean, radius=r)
        assert np.array_equal(ref.bits(out), ref.bits(clean)), r
        assert c == dict(with_depth=w * h, kept=w * h, dropped=0, holes=0, filled=0), r
    # the flying pixels cycle with period 4: within 3 rows, and anywhere in a plane of 8 rows, fewer than 3 pixels agree with one
    Z = ref.step_plane(w, h, 33)
    flying = np.zeros((h, w), bool)
    flying[:, 33] = True
    for r in radii:
        out, support, c = run(Z, radius=r, min_support=3)
        assert np.array_equal(np.isnan(out), flying), r
        assert np.array_equal(ref.bits(out)[~flying], ref.bits(Z)[~flying]), r
        assert c == dict(with_depth=w * h, kept=w * h - h, dropped=h, holes=0, filled=0), r
        assert support[flying].max() <= 2 and support[~flying].min() >= 3
        out, _, c = run(Z, radius=r)  # min_support 1: nothing is ever dropped, and nothing moves
        assert np.array_equal(ref.bits(out), ref.bits(Z)) and c["dropped"] == 0, r


def _fill_case(run):
    """a hole in a constant wall, a hole astride the step, a hole wider than the window"""
    w, h = 68, 20
    wall = np.full((h, w), 1.5, F)
    wall[9:11, 30:34] = np.nan  # (astride a tile border)
    out, _, c = run(wall, radius=2, fill_radius=2)
    assert np.array_equal(ref.bits(out), ref.bits(np.full((h, w), 1.5, F)))
    assert c == dict(with_depth=w * h - 8, kept=w * h - 8, dropped=0, holes=8, filled=8)
    step = ref.step_plane(w, h, 33, flying=False)
    step[4:7, 32:35] = np.nan
    out, _, c = run(step, radius=1, fill_radius=2)
    assert (out[4:7, 32:35] == F(1.5)).all() and c["filled"] == c["holes"] == 9
    rest = np.isfinite(step)
    assert np.array_equal(ref.bits(out)[rest], ref.bits(step)[rest])
    wide = np.full((h, w), 1.5, F)
    wide[5:14, 20:29] = np.nan  # 9x9: its centre is 5 pixels from the wall
    for fr, left in ((1, 49), (3, 9), (4, 1), (5, 0)):
        out, _, c = run(wide, radius=0, fill_radius=fr, min_fill_support=1)
        assert c["holes"] == 81 and c["filled"] == 81 - left, fr
        assert np.isnan(out[9, 24]) == (fr < 5) and int(np.isnan(out).sum()) == left, fr
        assert (out[np.isfinite(out)] == F(1.5)).all()
    out, _, c = run(wall, radius=2)  # without a fill holes stay holes
    assert c["filled"] == 0 and np.array_equal(np.isnan(out), np.isnan(wall))


def test_holes_are_filled_from_the_farthest_surface():
    """(the restatement's side of the GPU test of the same name)"""
    _fill_case(lambda Z, **opt: ref.filter_ref(Z, **opt))


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


@pytest.fixture(scope="module")
def resident(gpu):
    """the scenes a pyramid can be made of, on the device"""
    S = ref.scenes()
    return {name: gpu.RgbdImagePyramid(S[name][0], S[name][1], S[name][2], S[name][3], timestamp=3.25 + k)
            for k, name in enumerate(ref.DEVICE_SCENES)}


def _device(gpu, p, **opt):
    """(pyramid, filtered plane, support, counts as a dict)"""
    q, c, support = p.filter_depth(opt, counts=True, support=True)
    return q, q.plane(0, 1), support, {k: int(c[k]) for k in ref.COUNTS}


def _runner(gpu):
    """the library as _edge_case and _fill_case call it: a one-level pyramid of the plane, filtered"""
    def run(Z, **opt):
        h, w = Z.shape
        p = gpu.RgbdImagePyramid(np.zeros((h, w), F), Z, (64.0, 64.0, w / 2.0, h / 2.0), 1)
        return _device(gpu, p, **opt)[1:]
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("name", ref.DEVICE_SCENES)
def test_the_filter_equals_the_restatement(gpu, resident, name):
    for radius, min_support in WINDOWS:
        for fill in FILLS:
            opt = dict(radius=radius, min_support=min_support, fill_radius=fill)
            want = ref.scene_ref(name, **opt)
            _, plane, support, counts = _device(gpu, resident[name], **opt)
            assert plane.dtype == F and np.array_equal(ref.bits(plane), ref.bits(want[0])), (name, opt)
            assert support.dtype == np.uint16 and np.array_equal(support, want[1]), (name, opt)
            assert counts == want[2], (name, opt)
    for opt in (dict(), dict(radius=4, range_sigmas=5.0, fill_radius=2, min_fill_support=1), dict(radius=3, range_sigmas=0.5, min_support=2)):
        want = ref.scene_ref(name, **opt)
        _, plane, support, counts = _device(gpu, resident[name], **opt)
        assert np.array_equal(ref.bits(plane), ref.bits(want[0])) and np.array_equal(support, want[1]) and counts == want[2], (name, opt)


@pytest.mark.gpu
def test_a_width_no_pyramid_can_have_is_refused_where_the_pyramid_is_made(gpu):
    """the 33x9 scene never reaches the filter: a pyramid's width is a multiple of 4, and `past36` stands in for it on the device"""
    I, Z, K, levels = ref.scenes()["past"]
    with pytest.raises(gpu.DvoAmdError) as err:
        gpu.RgbdImagePyramid(I, Z, K, levels)
    assert err.value.status == INVALID


@pytest.mark.gpu
def test_the_result_is_an_ordinary_pyramid(gpu, resident, synth):
    p = resident["sensor"]
    I0, Z0, K, levels = ref.scenes()["sensor"]
    opt = dict(radius=2, min_support=2, fill_radius=1)
    cfg = gpu.Config(FirstLevel=levels - 1, LastLevel=0)
    trk = gpu.DenseTracker(cfg)
    other = gpu.RgbdImagePyramid.from_raw(*synth.sensor_frame(160, 120, synth.se3_exp(synth.XI_STEP_STREAM), frame_id=1), K, levels)
    before = [[p.plane(l, k) for k in range(6)] for l in range(levels)]
    tracked_before = trk.match(p, other)
    got, plane, _, _ = _device(gpu, p, **opt)
    want = ref.scene_ref("sensor", **opt)[0]
    host = gpu.RgbdImagePyramid(I0, want, K, levels, timestamp=p.timestamp())
    assert got.levels() == host.levels() == levels and got.timestamp() == p.timestamp()
    for l in range(levels):
        assert got.level_info(l)[:2] == host.level_info(l)[:2] == p.level_info(l)[:2]
        assert np.array_equal(got.level_info(l)[2], p.level_info(l)[2])
        for k in range(6):
            assert np.array_equal(got.plane(l, k), host.plane(l, k), equal_nan=True), (l, k)
    assert np.array_equal(ref.bits(got.plane(0, 0)), ref.bits(I0)) and not np.array_equal(plane, Z0, equal_nan=True)
    for l in range(levels):
        thresholds = (cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold)
        a, b = got.select(l, *thresholds), host.select(l, *thresholds)
        assert a[0] == b[0] > 0 and np.array_equal(a[1], b[1])
    tracked = trk.match(got, other)
    assert not tracked.isNaN() and cases.same_result(tracked, trk.match(host, other))
    # radius 0 without a fill reproduces the input pyramid, plane for plane
    same = p.filter_depth(dict(radius=0))
    assert isinstance(same, gpu.RgbdImagePyramid)
    for l in range(levels):
        for k in range(6):
            assert np.array_equal(ref.bits(same.plane(l, k)), ref.bits(before[l][k])), (l, k)
    assert cases.same_result(trk.match(same, other), tracked_before)
    # the input is only read
    for l in range(levels):
        for k in range(6):
            assert np.array_equal(ref.bits(p.plane(l, k)), ref.bits(before[l][k])), (l, k)


@pytest.mark.gpu
def test_an_edge_is_kept_and_its_flying_pixels_are_what_is_dropped_on_the_device(gpu):
    for w, h, radii in ((68, 20, (1, 2, 3)), (68, 8, (8,))):
        _edge_case(_runner(gpu), w, h, radii)


@pytest.mark.gpu
def test_holes_are_filled_from_the_farthest_surface_on_the_device(gpu, resident):
    _fill_case(_runner(gpu))
    for name in ref.DEVICE_SCENES:  # `filled` and `holes` are the restatement's
        opt = dict(radius=1, fill_radius=2, min_fill_support=2)
        want = ref.scene_ref(name, **opt)[2]
        counts = _device(gpu, resident[name], **opt)[3]
        assert (counts["holes"], counts["filled"]) == (want["holes"], want["filled"]) and want["holes"] > 0, name


@pytest.mark.gpu
def test_the_many_form_equals_single_calls(gpu, resident):
    """pyramids of five sizes in one call, in two orders, one of them twice; with and without the optional outputs"""
    opt = dict(radius=2, min_support=4, fill_radius=1)
    single = {name: _device(gpu, resident[name], **opt) for name in ref.DEVICE_SCENES}
    for order in (list(ref.DEVICE_SCENES), ["least", "sensor", "tiny", "sensor", "past36", "small"]):
        made, counts, support = gpu.filter_depth_many([resident[name] for name in order], opt, counts=True, support=True)
        assert len(made) == len(counts) == len(support) == len(order)
        for at, name in enumerate(order):
            want = single[name]
            for l in range(made[at].levels()):
                assert np.array_equal(ref.bits(made[at].plane(l, 1)), ref.bits(want[0].plane(l, 1))), (order, at, l)
            assert made[at].timestamp() == resident[name].timestamp()
            assert np.array_equal(support[at], want[2]) and {k: int(counts[at][k]) for k in ref.COUNTS} == want[3], (order, at)
            assert want[3] == ref.scene_ref(name, **opt)[2]
    plain = gpu.filter_depth_many([resident["tiny"], resident["small"]], opt)
    assert len(plain) == 2 and all(isinstance(q, gpu.RgbdImagePyramid) for q in plain)
    assert np.array_equal(ref.bits(plain[1].plane(0, 1)), ref.bits(single["small"][1]))
    assert gpu.filter_depth_many([]) == []
    # a support plane for some pyramids of a call only
    L = gpu.lib()
    got = np.zeros((12, 20), np.uint16)
    outs = (C.c_void_p * 2)()
    sup = (C.c_void_p * 2)(None, got.ctypes.data)
    o = gpu.depth_filter_options(**opt)
    assert L.dvo_amd_pyramid_filter_depth_many(2, (C.c_void_p * 2)(resident["small"]._h, resident["tiny"]._h), C.byref(o), outs, None, sup) == 0
    assert outs[0] and outs[1] and np.array_equal(got, single["tiny"][2])
    for h in outs:
        L.dvo_amd_pyramid_release(C.c_void_p(h))


@pytest.mark.gpu
def test_two_runs_give_the_same_bits(gpu, resident):
    for name in ("sensor", "small"):
        opt = dict(radius=8, min_support=4, fill_radius=8)
        a, b = _device(gpu, resident[name], **opt), _device(gpu, resident[name], **opt)
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3], name


@pytest.mark.gpu
def test_inputs_on_another_device_are_refused(gpu, resident):
    L = gpu.lib()
    if L.dvo_amd_device_count() > 1:
        I, Z, K, levels = ref.scenes()["small"]
        elsewhere = gpu.RgbdImagePyramid(I, Z, K, levels, device=1)
        with pytest.raises(gpu.DvoAmdError) as err:
            gpu.filter_depth_many([resident["small"], elsewhere])
        assert err.value.status == MISMATCH
        alone = elsewhere.filter_depth()  # ... and a call stays on the device of its pyramids
        assert np.array_equal(ref.bits(alone.plane(0, 1)), ref.bits(ref.scene_ref("small")[0]))
    # with resident pyramids too a mismatch is found before any device work: a stand-in that claims another device
    fake = C.create_string_buffer(1 << 16)
    C.c_int.from_buffer(fake, 4).value = 1
    C.c_int.from_buffer(fake, 8).value = 1
    outs = (C.c_void_p * 2)(0xDEAD, 0xDEAD)
    o = gpu.depth_filter_options()
    assert L.dvo_amd_pyramid_filter_depth_many(2, (C.c_void_p * 2)(resident["small"]._h, C.addressof(fake)), C.byref(o), outs, None,
                                               None) == MISMATCH
    assert not outs[0] and not outs[1]
    # a bad argument next to a resident pyramid: refused, and the output stays NULL
    h = C.c_void_p(0xDEAD)
    o = gpu.depth_filter_options(radius=1, min_support=10)
    assert L.dvo_amd_pyramid_filter_depth(resident["small"]._h, C.byref(o), C.byref(h), None, None) == INVALID and not h.value


@pytest.mark.gpu
def test_a_filtered_pair_tracks_under_the_sensor_regimes_bar(gpu, synth):
    """synth.sensor_pair(640, 480), four levels, both pyramids filtered with the defaults (both in one call): the pose error stays
    under the 1e-3 the raw pair is held to (tests/test_sensor_regime.py).  Measured: see DESIGN.md 4.19 (printed here; the two
    figures are not compared)"""
    (gr, zr), (gc, zc), Tgt = synth.sensor_pair(640, 480)
    K = synth.intrinsics_for(640, 480)
    ref_p, cur_p = gpu.RgbdImagePyramid.from_raw(gr, zr, K, 4), gpu.RgbdImagePyramid.from_raw(gc, zc, K, 4)
    trk = gpu.DenseTracker(gpu.Config(FirstLevel=3, LastLevel=0))
    raw = trk.match(ref_p, cur_p)
    (fr, fc), counts = gpu.filter_depth_many([ref_p, cur_p], counts=True)
    got = trk.match(fr, fc)
    e_raw, e_filtered = synth.pose_error(Tgt, raw.Transformation), synth.pose_error(Tgt, got.Transformation)
    print("pose error: raw %.3e, filtered %.3e; counts %s" % (e_raw, e_filtered, counts))
    assert not got.isNaN() and e_filtered < 1e-3
    assert int(counts[0]["with_depth"] + counts[0]["holes"]) == 640 * 480 and int(counts[0]["dropped"]) == 0


@pytest.mark.gpu
def test_tum_load_filters_after_ingest_when_asked_to(gpu, synth, tmp_path):
    """tum.load and tum.load_batch with depth_filter=: what filter_depth makes of the pyramid they return without it"""
    from dvo_slam_amd import tum
    from test_tum import write_png

    w, h, levels = 68, 36, 1
    K = synth.intrinsics_for(w, h)
    os.makedirs(str(tmp_path / "rgb")), os.makedirs(str(tmp_path / "depth"))
    entries = []
    for f in range(2):
        grey, raw = synth.sensor_frame(w, h, frame_id=30 + f, channels=3)
        write_png(str(tmp_path / "rgb" / f"{f}.png"), grey[..., ::-1], 8, 2)
        write_png(str(tmp_path / "depth" / f"{f}.png"), raw[..., None], 16, 0)
        entries.append(tum.RgbdPair(10.0 + f, f"rgb/{f}.png", 10.0 + f, f"depth/{f}.png"))
    opt = dict(radius=2, fill_radius=1)
    plain = tum.load_batch(entries, K, levels, base=str(tmp_path))
    batched = tum.load_batch(entries, K, levels, base=str(tmp_path), depth_filter=opt)
    for f, e in enumerate(entries):
        one = tum.load(K, str(tmp_path / e.RgbFile), str(tmp_path / e.DepthFile), levels, timestamp=e.RgbTimestamp, depth_filter=opt)
        want = ref.filter_ref(plain[f].plane(0, 1), **opt)[0]
        assert not np.array_equal(ref.bits(want), ref.bits(plain[f].plane(0, 1)))
        for got in (one, batched[f]):
            assert got.timestamp() == 10.0 + f
            assert np.array_equal(ref.bits(got.plane(0, 1)), ref.bits(want)), f
            assert np.array_equal(ref.bits(got.plane(0, 0)), ref.bits(plain[f].plane(0, 0))), f
    defaults = tum.load(K, str(tmp_path / "rgb/0.png"), str(tmp_path / "depth/0.png"), levels, depth_filter={})
    assert np.array_equal(ref.bits(defaults.plane(0, 1)), ref.bits(ref.filter_ref(plain[0].plane(0, 1))[0]))


@pytest.mark.gpu
def test_device_time_is_reported_when_asked_for(gpu, resident):
    gpu.depth_filter_timing(True)
    try:
        resident["sensor"].filter_depth()
        assert 0.0 < gpu.depth_filter_timing(True) < 1000.0
    finally:
        gpu.depth_filter_timing(False)
