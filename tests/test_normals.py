"""Surface normals on the device (include/dvo_amd.h, "Surface normals"): dvo_amd_pyramid_normals, dvo_amd_mask_from_normals,
dvo_amd_point_cloud_normals, dvo_amd_write_pcd_normals.  The rule is pinned in the header and restated in tests/normals_ref.py.
Every comparison with the library is bit equality on uint32 views, NaN positions and NaN bits included; byte planes and integer
counts are compared as they are.
CPU: exports and layout, the argument checks that need no device, the restatement against its pixel loop, the rule against the
analytic normals of the noise-free room corner, what the window gains on a sensor frame, the PCD writer byte for byte.
GPU: the library against the restatement.

The figures behind the two CPU bars (measured with the restatement, 160x120):
  truth: worst angle to the analytic normal over the 16 221 interior pixels of synth.render(160, 120), r = 0: 9.44e-5 degrees
         (fp32 rounding of the points; the far wall's pixels come out exact); the bar is twice that
  gain:  mean angle over the interior eroded by 4 of synth.sensor_frame(160, 120, frame_id=0), ratio 0.02:
         r = 0: 27.4 degrees, r = 1: 7.9, r = 3: 2.3 (1 190 pixels)"""
import ctypes as C
import functools
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_ref as ref  # noqa: E402
import selection_mask_cases as cases  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_normal_options", "dvo_amd_pyramid_normals", "dvo_amd_mask_from_normals",
               "dvo_amd_point_cloud_normals", "dvo_amd_write_pcd_normals", "dvo_amd_debug_normals_timing"]
INVALID, NO_DEVICE, MISMATCH = 1, 2, 8
TRUTH_WORST_DEG = 9.45e-5  # the restatement's worst interior error on the noise-free scene (module docstring)


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


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
    assert (capi.NORMAL_FACING_AXIS, capi.NORMAL_FACING_RAY, capi.NORMAL_MAX_RADIUS) == (ref.FACING_AXIS, ref.FACING_RAY, ref.MAX_RADIUS)
    assert capi.NORMAL_MASK_DTYPE.itemsize == 24
    header = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    for define, value in (("DVO_AMD_NORMAL_MAX_RADIUS", 8), ("DVO_AMD_NORMAL_FACING_AXIS", 0), ("DVO_AMD_NORMAL_FACING_RAY", 1)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define


def test_the_default_options_are_all_zero(capi):
    opt = capi.NormalOptions()
    assert C.sizeof(opt) == 4 * capi.MAX_LEVELS + 12
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt))
    capi.lib().dvo_amd_default_normal_options(C.byref(opt))
    assert bytes(opt) == bytes(C.sizeof(opt))
    capi.lib().dvo_amd_default_normal_options(None)  # a no-op
    made = capi.normal_options(radius=(3, 2, 1), depth_step_ratio=0.02, facing=capi.NORMAL_FACING_RAY, toward_camera=1)
    assert list(made.radius) == [3, 2, 1, 0, 0, 0, 0, 0] and made.depth_step_ratio == F(0.02) and (made.facing, made.toward_camera) == (1, 1)
    assert list(capi.normal_options(radius=2).radius) == [2] * capi.MAX_LEVELS
    with pytest.raises(TypeError):
        capi.normal_options(window=3)


# ---- CPU: the argument checks -----------------------------------------------------------------------------------------------------

class Fakes:
    """zeroed buffers that stand for a one-level pyramid on device 0 (refs, device, n_levels lead a pyramid) and for contexts (the
    device leads a context): an argument error is reported before either is looked at any further"""

    def __init__(self):
        self.keep = [C.create_string_buffer(1 << 16) for _ in range(3)]
        C.c_int.from_buffer(self.keep[0], 8).value = 1   # the pyramid's level count
        C.c_int.from_buffer(self.keep[2], 0).value = 1   # the second context's device
        self.pyr, self.ctx, self.ctx_elsewhere = [C.c_void_p(C.addressof(b)) for b in self.keep]


BAD_OPTIONS = [("radius", dict(radius=-1)), ("radius", dict(radius=9)), ("radius", dict(radius=(1 << 30,))),
               ("depth_step_ratio", dict(depth_step_ratio=-0.5)), ("depth_step_ratio", dict(depth_step_ratio=np.nan)),
               ("depth_step_ratio", dict(depth_step_ratio=np.inf)), ("facing", dict(facing=2)), ("facing", dict(facing=-1))]


def test_argument_errors_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    f = Fakes()
    good = capi.normal_options(radius=(2, 9))  # (the radius of a level the pyramid does not have is not looked at)
    nrm, fac, pts = (C.c_float * 64)(), (C.c_float * 16)(), (C.c_float * 64)()
    cnt = (C.c_longlong * 24)()
    mf = (C.c_float * 8)(*[0.5] * 8)
    no_device = L.dvo_amd_device_count() == 0

    def refused(entry, rc, what, word=None):
        assert rc == INVALID, (entry, what, rc)
        reason = L.dvo_amd_last_error().decode()
        assert reason.startswith(entry + ": "), (entry, what, reason)
        assert word is None or word in reason, (entry, what, reason)

    # dvo_amd_pyramid_normals
    entry = "dvo_amd_pyramid_normals"

    def planes(p=f.pyr, level=0, opt=good):
        return L.dvo_amd_pyramid_normals(p, level, None if opt is None else C.byref(opt), nrm, fac, cnt)

    refused(entry, planes(p=None), "pyramid", "NULL")
    refused(entry, planes(opt=None), "options", "NULL")
    for level in (-1, 1, 8):
        refused(entry, planes(level=level), ("level", level), "level")
    for word, kw in BAD_OPTIONS:
        refused(entry, planes(opt=capi.normal_options(**kw)), kw, word)
    if no_device:
        assert planes() == NO_DEVICE

    # dvo_amd_mask_from_normals
    entry = "dvo_amd_mask_from_normals"

    def mask(p=f.pyr, opt=good, min_facing=mf, with_out=True, keep=0):
        h = C.c_void_p(0xDEAD)
        rc = L.dvo_amd_mask_from_normals(p, None if opt is None else C.byref(opt), min_facing, keep, C.byref(h) if with_out else None, cnt)
        assert not with_out or not h.value or rc == 0, (rc, h.value)  # *out is NULL on every failure
        return rc

    refused(entry, mask(p=None), "pyramid", "NULL")
    refused(entry, mask(opt=None), "options", "NULL")
    refused(entry, mask(min_facing=None), "min_facing", "NULL")
    refused(entry, mask(with_out=False), "out", "NULL")
    for word, kw in BAD_OPTIONS:
        refused(entry, mask(opt=capi.normal_options(**kw)), kw, word)
    refused(entry, mask(min_facing=(C.c_float * 8)(np.nan, *[0.5] * 7)), "min_facing[0]", "min_facing[0]")
    if no_device:
        assert mask(min_facing=(C.c_float * 8)(0.5, np.nan, *[0.5] * 6)) == NO_DEVICE  # (of a level the pyramid does not have)
        assert mask(min_facing=(C.c_float * 8)(-np.inf, *[np.inf] * 7), keep=1) == NO_DEVICE

    # dvo_amd_point_cloud_normals
    entry = "dvo_amd_point_cloud_normals"
    eye = (C.c_double * 16)(*np.eye(4).ravel())

    def cloud(ctx=f.ctx, p=f.pyr, level=0, pose=eye, opt=good, out=pts, normals=nrm):
        return L.dvo_amd_point_cloud_normals(ctx, p, level, pose, None, 0, None if opt is None else C.byref(opt), out, normals)

    for what, kw in {"context": dict(ctx=None), "pyramid": dict(p=None), "options": dict(opt=None), "out": dict(out=None),
                     "normals": dict(normals=None)}.items():
        refused(entry, cloud(**kw), what, "NULL")
    for level in (-1, 1):
        refused(entry, cloud(level=level), ("level", level), "level")
    for word, kw in BAD_OPTIONS:
        refused(entry, cloud(opt=capi.normal_options(**kw)), kw, word)
    bad_pose = (C.c_double * 16)(*np.eye(4).ravel())
    bad_pose[13] = np.nan
    refused(entry, cloud(pose=bad_pose), "pose", "non-finite")
    assert cloud(ctx=f.ctx_elsewhere) == MISMATCH  # behind every argument error, before the device is looked for
    if no_device:
        assert cloud() == NO_DEVICE and cloud(pose=None) == NO_DEVICE

    # the writer and the instrumentation
    refused("dvo_amd_write_pcd_normals", L.dvo_amd_write_pcd_normals(None, pts, nrm, 1, 1, 1), "path", "NULL")
    refused("dvo_amd_write_pcd_normals", L.dvo_amd_write_pcd_normals(b"/nowhere/x.pcd", pts, None, 1, 1, 1), "normals", "NULL")
    refused("dvo_amd_write_pcd_normals", L.dvo_amd_write_pcd_normals(b"/nowhere/x.pcd", pts, nrm, 3, 2, 2), "size", "width")
    assert L.dvo_amd_debug_normals_timing(-1, 0, None, None, None) == INVALID
    if no_device:
        assert L.dvo_amd_debug_normals_timing(0, 1, None, None, None) == NO_DEVICE
        assert L.dvo_amd_debug_normals_timing(0, 0, None, None, None) == 0


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------

def _random_plane(seed, w=12, h=10):
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:h, 0:w]
    Z = (F(1.5) + F(0.05) * u + F(0.08) * v + rng.normal(scale=0.02, size=(h, w))).astype(F)
    Z[rng.random((h, w)) < 0.12] = np.nan          # holes
    Z[h // 2:, w // 2:] += F(0.6)                   # a depth step for the ratio to cut at
    return Z, (F(11.0), F(10.5), F(5.7), F(4.6))


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("ratio", [0.0, 0.05])
def test_the_restatement_equals_its_pixel_loop(radius, ratio):
    for seed in (3, 4):
        Z, K = _random_plane(seed)
        for facing in (ref.FACING_AXIS, ref.FACING_RAY):
            for toward in (0, 1):
                a = ref.normals_ref(Z, K, radius, ratio, facing, toward)
                b = ref.normals_loop(Z, K, radius, ratio, facing, toward)
                what = (seed, radius, ratio, facing, toward)
                assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2], what
                undefined = np.isnan(a[0][..., 3])
                assert a[2] == (int((~undefined).sum()), int(undefined.sum())) and 0 < a[2][1] < Z.size, what
                # an undefined pixel is five quiet NaNs; a defined one has a unit normal with a zero behind it
                assert (ref.bits(a[0])[undefined] == 0x7FC00000).all() and (ref.bits(a[1])[undefined] == 0x7FC00000).all(), what
                assert (a[0][~undefined][:, 3] == 0).all() and np.isfinite(a[1][~undefined]).all(), what
                assert np.allclose(np.linalg.norm(a[0][~undefined][:, :3].astype(np.float64), axis=1), 1.0, atol=1e-6), what
    # the ratio cuts the window at the depth step, and only there
    Z, K = _random_plane(3)
    assert not same_bits(ref.normals_ref(Z, K, 2, 0.0)[0], ref.normals_ref(Z, K, 2, 0.05)[0])


@functools.lru_cache(maxsize=None)
def _corner():
    from dvo_slam_amd import synth

    w, h = 160, 120
    K = synth.intrinsics_for(w, h)
    which = ref.corner_planes(w, h, K)
    _, Z = synth.render(w, h)
    inside = ref.interior(Z, which)
    for a in (which, Z, inside):
        a.setflags(write=False)
    return synth, K, which, Z, inside


def test_on_exact_depth_the_rule_gives_the_planes_analytic_normals():
    _, K, which, Z, inside = _corner()
    N, facing, _ = ref.normals_ref(Z, K, 0)
    err = ref.angle_deg(N, which)[inside]
    print("truth: interior pixels %d, per plane %s, worst angle %.3e deg, mean %.3e deg"
          % (inside.sum(), [int((inside & (which == k)).sum()) for k in range(3)], err.max(), err.mean()))
    assert inside.sum() > 15000 and all((inside & (which == k)).sum() > 200 for k in range(3))
    assert not np.isnan(err).any()
    assert err.max() < 2 * TRUTH_WORST_DEG
    # the reference's `angles` on the far wall, whose normal is the optical axis
    assert (facing[inside & (which == 1)] == 1).all()


def test_the_window_more_than_halves_the_error_on_a_sensor_frame():
    synth, K, which, _, inside = _corner()
    _, Z = synth.raw_to_float(*synth.sensor_frame(160, 120, frame_id=0))
    deep = ref.erode(inside, 4)
    mean = {}
    for r in (0, 1, 3):
        err = ref.angle_deg(ref.normals_ref(Z, K, r, 0.02)[0], which)[deep]
        assert not np.isnan(err).any(), r
        mean[r] = err.mean()
    print("gain: pixels %d, mean angle in degrees: r = 0: %.2f, r = 1: %.2f, r = 3: %.2f" % (deep.sum(), mean[0], mean[1], mean[3]))
    assert deep.sum() > 500
    assert mean[3] < 0.5 * mean[0]
    assert mean[3] < mean[1] < mean[0]


def test_the_pcd_writer_is_byte_exact(tmp_path):
    from dvo_slam_amd import tum

    xyz = np.array([[0.5, -1.25, 2.0], [np.nan, np.nan, np.nan], [3.0, 4.0, -5.5]], F)
    rgb = np.array([0x00102030, 0, 0x00FFEEDD], np.uint32)
    nrm = np.array([[0.0, 0.6, -0.8, 0.0], [np.nan] * 4, [1.0, 0.0, 0.0, 0.0]], F)
    path = str(tmp_path / "cloud.pcd")
    tum.write_pcd(path, xyz, rgb, normals=nrm)
    want = (b"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb normal_x normal_y normal_z curvature\n"
            b"SIZE 4 4 4 4 4 4 4 4\nTYPE F F F F F F F F\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH 3\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\n"
            b"POINTS 3\nDATA binary\n")
    for p, c, n in zip(xyz, rgb, nrm):
        want += struct.pack("<3fI", *p, int(c)) + struct.pack("<3f", *n[:3]) + struct.pack("<f", 0.0)
    assert open(path, "rb").read() == want
    # organized: [h, w, ...] arrays give WIDTH w, HEIGHT h
    tum.write_pcd(path, np.zeros((2, 3, 3), F), np.zeros((2, 3), np.uint32), normals=np.zeros((2, 3, 4), F))
    got = open(path, "rb").read()
    assert b"WIDTH 3\nHEIGHT 2\n" in got and b"POINTS 6\n" in got and got.endswith(bytes(6 * 32))
    with pytest.raises(ValueError):
        tum.write_pcd(path, xyz, rgb, normals=nrm[:2])


# ---- GPU: the library against the restatement -------------------------------------------------------------------------------------

RADII = (3, 2, 1, 0)


@pytest.fixture(scope="module")
def frame(capi, synth):
    """the 160x120 sensor frame as a four-level pyramid, and every level's (Z, K) as the device holds them"""
    img, raw = synth.sensor_frame(160, 120, frame_id=0)
    pyr = capi.RgbdImagePyramid.from_raw(img, raw, synth.intrinsics_for(160, 120), 4)
    return pyr, _levels(pyr)


def _levels(pyr):
    out = []
    for l in range(pyr.levels()):
        Z = pyr.plane(l, 1)
        Z.setflags(write=False)
        out.append((Z, tuple(pyr.level_info(l)[2])))
    return out


@functools.lru_cache(maxsize=None)
def _restated(key, level, radius, ratio, facing, toward):
    Z, K = _restated.planes[key][level]
    out = ref.normals_ref(Z, K, radius, ratio, facing, toward)
    out[0].setflags(write=False), out[1].setflags(write=False)
    return out


_restated.planes = {}


def _check_planes(pyr, key, radii, ratio=0.0, facing=0, toward=0):
    _restated.planes.setdefault(key, _levels(pyr))
    opt = dict(radius=radii, depth_step_ratio=ratio, facing=facing, toward_camera=toward)
    for level in range(pyr.levels()):
        N, f, cnt = pyr.normals(level, **opt)
        rN, rf, rc = _restated(key, level, radii[level], ratio, facing, toward)
        what = (key, level, radii[level], ratio, facing, toward)
        assert same_bits(N, rN), what
        assert same_bits(f, rf), what
        assert (cnt["defined"], cnt["undefined"]) == rc and sum(rc) == rN.shape[0] * rN.shape[1], what


@pytest.mark.gpu
@pytest.mark.parametrize("facing", [ref.FACING_AXIS, ref.FACING_RAY])
@pytest.mark.parametrize("toward", [0, 1])
@pytest.mark.parametrize("ratio", [0.0, 0.02])
def test_a_sensor_frames_normals_equal_the_restatement_on_every_level(capi, frame, facing, toward, ratio):
    """160x120 spans five tiles across and fifteen down; every level has its own radius"""
    pyr, _ = frame
    _check_planes(pyr, "frame", RADII, ratio, facing, toward)
    N, f, cnt = pyr.normals(0, radius=RADII, depth_step_ratio=ratio, facing=facing, toward_camera=toward)
    assert 0 < cnt["undefined"] < cnt["defined"]


def _float_pyramid(capi, synth, w, h, frame_id, holes=None):
    _, Z = synth.raw_to_float(*synth.sensor_frame(w, h, frame_id=frame_id))
    if holes is not None:
        Z = holes(Z.copy())
    return capi.RgbdImagePyramid(np.zeros((h, w), F), Z, synth.intrinsics_for(w, h), 1)


@pytest.mark.gpu
def test_partial_tiles_clipped_windows_and_the_smallest_level(capi, synth):
    # 68x36: the width is no multiple of a wave, the last tile of a row and the last row of tiles are partial
    _check_planes(_float_pyramid(capi, synth, 68, 36, 5), "68x36", (2,), 0.02, ref.FACING_RAY, 1)
    _check_planes(_float_pyramid(capi, synth, 68, 36, 5), "68x36", (2,))
    # 20x12 under a 17x17 window: wider than most of the plane, clipped on every side
    _check_planes(_float_pyramid(capi, synth, 20, 12, 6), "20x12", (8,), 0.05, ref.FACING_RAY)
    _check_planes(_float_pyramid(capi, synth, 20, 12, 6), "20x12", (8,))
    # 4x2, the smallest level there is: every index of the stencil is clamped somewhere
    rng = np.random.default_rng(8)
    Z = (F(1) + rng.random((2, 4))).astype(F)
    tiny = capi.RgbdImagePyramid(np.zeros((2, 4), F), Z, (F(3.2), F(3.2), F(1.6), F(1.3)), 1)
    for r in (0, 8):
        for facing in (ref.FACING_AXIS, ref.FACING_RAY):
            _check_planes(tiny, "4x2", (r,), 0.0, facing, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [0, 1, 4])
def test_missing_rows_columns_blocks_and_a_plane_without_depth(capi, synth, radius):
    def holes(Z):
        Z[17, :] = np.nan
        Z[:, 40] = np.nan
        Z[5:10, 50:55] = np.nan
        return Z

    pyr = _float_pyramid(capi, synth, 68, 36, 7, holes)
    for ratio in (0.0, 0.02):
        _check_planes(pyr, "holes", (radius,), ratio, ref.FACING_RAY)
    N, f, cnt = pyr.normals(0, radius=radius)
    assert np.isnan(N[17]).all() and np.isnan(N[:, 40]).all() and np.isnan(N[5:10, 50:55]).all() and np.isnan(f[17]).all()
    assert cnt["defined"] + cnt["undefined"] == 68 * 36 and cnt["undefined"] >= 68 + 36 - 1 + 25
    empty = _float_pyramid(capi, synth, 68, 36, 7, lambda Z: np.full_like(Z, np.nan))
    _check_planes(empty, "empty", (radius,))
    N, f, cnt = empty.normals(0, radius=radius)
    assert (ref.bits(N) == 0x7FC00000).all() and (ref.bits(f) == 0x7FC00000).all() and cnt == {"defined": 0, "undefined": 68 * 36}


@pytest.mark.gpu
@pytest.mark.parametrize("undefined_keep", [0, 1])
@pytest.mark.parametrize("min_facing", [0.0, 0.5, 0.9])
def test_the_mask_equals_the_restatement_and_is_built_in_one_launch(capi, frame, min_facing, undefined_keep):
    pyr, levels = frame
    for facing in (ref.FACING_AXIS, ref.FACING_RAY):
        opt = dict(radius=RADII, depth_step_ratio=0.02, facing=facing, toward_camera=0)
        mask, cnt = capi.SelectionMask.from_normals(pyr, min_facing, opt, undefined_keep=bool(undefined_keep), counts=True)
        timing = capi.normals_timing(enable=False)
        assert (timing["launches"], timing["synchronisations"]) == (1, 1)
        info = mask.info()
        assert (info["width"], info["height"], info["levels"]) == (160, 120, 4)
        for l, (Z, K) in enumerate(levels):
            want, (n_def, n_und, n_kept) = ref.mask_ref(Z, K, min_facing, undefined_keep, radius=RADII[l], ratio=0.02, facing=facing)
            what = (facing, min_facing, undefined_keep, l)
            assert same_bits(mask.download(l), want), what
            assert tuple(int(v) for v in cnt[l]) == (n_def, n_und, n_kept) and info["kept"][l] == n_kept, what
            assert n_def + n_und == Z.size and n_kept == int(want.sum()), what
    # one value per level
    per_level = capi.SelectionMask.from_normals(pyr, [0.0, 0.5, 0.9, 0.5], dict(radius=RADII))
    for l, mf in enumerate((0.0, 0.5, 0.9, 0.5)):
        assert same_bits(per_level.download(l), ref.mask_ref(levels[l][0], levels[l][1], mf, 0, radius=RADII[l])[0]), l


@pytest.mark.gpu
def test_the_device_time_of_a_call_is_reported_once_timing_is_on(capi, frame):
    pyr, _ = frame
    capi.normals_timing(enable=True)
    pyr.normals(0, radius=3)
    t = capi.normals_timing(enable=False)
    assert (t["launches"], t["synchronisations"]) == (1, 1) and 0.0 < t["ms"] < 100.0


@pytest.mark.gpu
def test_a_match_behind_the_mask_is_the_match_behind_its_bytes(capi, synth):
    """the mask is an ordinary one: uploaded again byte for byte with dvo_amd_mask_create_levels it selects the same points"""
    w, h, levels = 80, 60, 2
    (gr, zr), (gc, zc), _ = synth.sensor_pair(w, h, xi_gt=synth.XI_GT_PAIR * 0.5)
    K = synth.intrinsics_for(w, h)
    reference, current = capi.RgbdImagePyramid.from_raw(gr, zr, K, levels), capi.RgbdImagePyramid.from_raw(gc, zc, K, levels)
    trk = capi.DenseTracker(capi.Config(FirstLevel=levels - 1, LastLevel=0))
    mask = capi.SelectionMask.from_normals(reference, 0.6, dict(radius=(2, 1), depth_step_ratio=0.02, facing=ref.FACING_RAY))
    planes = [mask.download(l) for l in range(levels)]
    assert all(0 < p.sum() < p.size for p in planes)
    uploaded = capi.SelectionMask.from_levels(planes)
    behind, again, plain = trk.match(reference, current, mask=mask), trk.match(reference, current, mask=uploaded), trk.match(reference, current)
    assert not behind.isNaN()
    assert cases.same_result(behind, again)
    assert not cases.same_result(behind, plain)  # (the mask did drop points)
    # the pipeline the mask is for: eroded, it still selects
    assert not trk.match(reference, current, mask=mask.erode(1)).isNaN()


def _y_rotation(deg, t):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T[:3, 3] = t
    return T


@pytest.fixture(scope="module")
def cloud_frame(capi, synth):
    img, raw = synth.sensor_frame(80, 60, frame_id=3)
    return capi.RgbdImagePyramid.from_raw(img, raw, synth.intrinsics_for(80, 60), 2)


@pytest.mark.gpu
@pytest.mark.parametrize("pose", ["identity", "rotated"])
def test_the_clouds_points_are_the_plain_clouds_and_its_normals_the_restatement_rotated(capi, cloud_frame, pose):
    pyr = cloud_frame
    T = None if pose == "identity" else _y_rotation(30.0, [0.3, -0.2, 0.5])
    rng = np.random.default_rng(5)
    for level, bgr in ((0, rng.integers(0, 256, size=(60, 80, 3), dtype=np.uint8)), (1, None)):
        opt = dict(radius=(2, 1), depth_step_ratio=0.02, facing=ref.FACING_RAY, toward_camera=1)
        xyz, rgb, nrm = pyr.point_cloud(pose=T, bgr=bgr, level=level, normals=opt)
        pxyz, prgb = pyr.point_cloud(pose=T, bgr=bgr, level=level)
        assert same_bits(xyz, pxyz) and same_bits(rgb, prgb), (pose, level)
        Z, K = pyr.plane(level, 1), pyr.level_info(level)[2]
        N = ref.normals_ref(Z, K, (2, 1)[level], 0.02, ref.FACING_RAY, 1)[0]
        assert same_bits(nrm, ref.rotate_ref(N, T)), (pose, level)
        assert same_bits(np.isnan(nrm[..., 3]), np.isnan(N[..., 3])) and 0 < np.isnan(N[..., 3]).sum() < Z.size
    # normals=True: the reference's rule
    _, _, nrm = pyr.point_cloud(pose=T, normals=True)
    assert same_bits(nrm, ref.rotate_ref(ref.normals_ref(pyr.plane(0, 1), pyr.level_info(0)[2])[0], T))


@pytest.mark.gpu
def test_two_calls_and_a_second_context_give_the_same_bits(capi, frame, cloud_frame):
    pyr, _ = frame
    opt = dict(radius=RADII, depth_step_ratio=0.02, facing=ref.FACING_RAY, toward_camera=1)
    for level in range(4):
        a, b = pyr.normals(level, **opt), pyr.normals(level, **opt)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2], level
    m1, c1 = capi.SelectionMask.from_normals(pyr, 0.5, opt, counts=True)
    m2, c2 = capi.SelectionMask.from_normals(pyr, 0.5, opt, counts=True)
    assert all(same_bits(m1.download(l), m2.download(l)) for l in range(4)) and same_bits(c1, c2)
    T = _y_rotation(30.0, [0.3, -0.2, 0.5])
    first = cloud_frame.point_cloud(pose=T, normals=opt, tracker=capi.DenseTracker())
    second = cloud_frame.point_cloud(pose=T, normals=opt, tracker=capi.DenseTracker())
    assert all(same_bits(x, y) for x, y in zip(first, second))
