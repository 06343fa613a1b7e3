"""The keyframe map rendered into a camera view (dvo_amd.h: dvo_amd_map_render, dvo_amd_map_render_pyramid).

The rule is pinned operation by operation in the header and restated in tests/map_render_ref.py; equality is same_bits of
tests/test_map_cloud.py and there is no tolerance anywhere in this file.
CPU: the restatement against its independent per-pixel form on random clouds and on crafted cases, each of which asserts that
it really hits its case; without a GPU both entries fail loudly.
GPU: KeyframeMap.render against render_ref(*map.extract(), ...) on all four planes and the stats."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from map_render_ref import (default_near, make_view, near_limit, render_brute, render_ref)  # noqa: E402
from test_map_cloud import same_bits  # noqa: E402

F = np.float32
PLANES = ("depth", "rgb", "intensity", "index")


def assert_same_render(a, b, what=None):
    assert a["stats"] == b["stats"], (what, a["stats"], b["stats"])
    for p in PLANES:
        assert same_bits(a[p], b[p]), (what, p, int((a[p].view(np.uint32) != b[p].view(np.uint32)).sum()))


def _both(xyz, rgb, leaf, pose, view, what=None):
    ref, brute = render_ref(xyz, rgb, leaf, pose, view), render_brute(xyz, rgb, leaf, pose, view)
    assert_same_render(ref, brute, what)
    st = ref["stats"]
    assert st["voxels"] == len(xyz) == st["behind_near"] + st["outside"] + st["drawn"]
    assert st["covered_pixels"] == int((ref["index"] >= 0).sum()) == int(np.isfinite(ref["depth"]).sum())
    return ref, brute


def _colours(rng, n):
    return rng.integers(0, 1 << 24, size=n, dtype=np.uint32)


def _frustum_cloud(rng, n, view, zmin=0.4, zmax=6.0, spill=1.3):
    """n points in (and a little around) the view's frustum, in camera coordinates"""
    z = rng.uniform(zmin, zmax, n)
    u = rng.uniform(-spill + 1, spill, n) * view.width
    v = rng.uniform(-spill + 1, spill, n) * view.height
    xyz = np.stack([(u - view.ox) / view.fx * z, (v - view.oy) / view.fy * z, z], axis=1).astype(F)
    return xyz, _colours(rng, n)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,K", [((33, 17), (40, 40, 16.3, 8.1)), ((64, 48), (60.5, 58.25, 31.5, 23.75))])
def test_restatement_matches_per_pixel_form_on_random_clouds(synth, size, K):
    leaf = 0.05
    view = make_view(size[0], size[1], K, default_near(leaf, K))
    pose = synth.se3_exp([0.3, -0.2, 0.1, 0.05, -0.08, 0.03])
    rng = np.random.default_rng(7)
    seen = {"multi": 0, "fallback": 0, "clamped": 0, "outside": 0, "side": 0}
    for n in (0, 1, 63, 64, 65, 1000):
        cam, rgb = _frustum_cloud(rng, n, view)
        world = (cam.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]).astype(F)  # the voxels where the camera at `pose` sees them
        ref, _ = _both(world, rgb, leaf, pose, view, n)
        if n == 0:
            assert ref["stats"]["covered_pixels"] == 0 and (ref["index"] == -1).all() and np.isnan(ref["depth"]).all()
        seen["multi"] += ref["info"]["multi"]
        seen["fallback"] += ref["info"]["fallback"]
        seen["clamped"] += ref["info"]["clamped"]
        seen["outside"] += ref["stats"]["outside"]
        seen["side"] = max(seen["side"], ref["info"]["max_side"])
    assert all(v > 0 for v in seen.values()) and seen["side"] >= 3, seen


def test_equal_depths_go_to_the_lower_rank():
    leaf, K = 0.05, (60, 60, 16, 8)
    view = make_view(33, 17, K, default_near(leaf, K))
    # four voxels at one depth with overlapping 3-pixel footprints, and the same again behind a nearer one
    xyz = np.array([[0.02, 0, 1], [0, 0, 1], [0.03, 0.02, 1], [0, 0.03, 1], [0.1, 0.1, 0.5], [0.11, 0.1, 0.5], [0.1, 0.1, 1]], F)
    rgb = np.arange(1, 8, dtype=np.uint32) * 0x10203
    ref, brute = _both(xyz, rgb, leaf, None, view)
    assert brute["info"]["ties"] >= 4                                  # pixels whose least depth is shared by several voxels
    both = (ref["info"]["candidates"] > 1)
    assert both.sum() >= 4
    assert ref["index"][8, 16] == 0 and ref["index"][8, 15] == 1        # (16, 8): voxels 0..3 cover it, rank 0 wins
    assert ref["depth"][8, 16] == F(1) and ref["rgb"][8, 16] == rgb[0]
    swapped = render_ref(xyz[[1, 0, 2, 3, 4, 5, 6]], rgb[[1, 0, 2, 3, 4, 5, 6]], leaf, None, view)
    assert swapped["index"][8, 16] == 0 and swapped["rgb"][8, 16] == rgb[1]  # the rank decides, not the voxel


def test_near_plane_is_inclusive():
    leaf, K = 0.05, (40, 40, 16.3, 8.1)
    near = F(0.75)
    view = make_view(33, 17, K, near)
    below = np.nextafter(near, F(0))
    xyz = np.array([[0, 0, near], [0.2, 0, below], [-0.2, 0.1, np.nextafter(near, F(1))]], F)
    ref, _ = _both(xyz, _colours(np.random.default_rng(1), 3), leaf, None, view)
    assert ref["stats"]["behind_near"] == 1 and ref["stats"]["drawn"] == 2
    assert 0 in ref["index"] and 2 in ref["index"] and 1 not in ref["index"]
    assert ref["depth"][ref["index"] == 0].view(np.uint32)[0] == near.view(np.uint32)


def test_footprints_without_a_pixel_centre_take_the_nearest_pixel():
    leaf, K = 0.01, (40, 40, 16.3, 8.1)
    view = make_view(33, 17, K, default_near(leaf, K))
    rng = np.random.default_rng(3)
    xyz, rgb = _frustum_cloud(rng, 200, view, zmin=2.0, zmax=3.0, spill=1.0)   # footprints of 0.13 .. 0.2 pixels
    ref, _ = _both(xyz, rgb, leaf, None, view)
    assert ref["info"]["fallback"] > 150 and ref["info"]["max_side"] == 1
    assert ref["stats"]["covered_pixels"] > 100
    one = np.array([[0.0, 0.0, 2.0]], F)                                        # u = 16.3, v = 8.1: no centre within 0.1
    r1 = render_ref(one, rgb[:1], leaf, None, view)
    assert r1["info"]["fallback"] == 1 and r1["index"][8, 16] == 0 and r1["stats"]["covered_pixels"] == 1


def test_footprints_cut_by_each_border():
    leaf, K = 0.1, (40, 40, 16.0, 8.0)
    view = make_view(33, 17, K, default_near(leaf, K))                          # at z = 1 a footprint is 4 pixels wide
    z = 1.0
    at = lambda u, v: [(u - 16.0) / 40.0 * z, (v - 8.0) / 40.0 * z, z]          # noqa: E731
    cases = {"left": at(-1.5, 8), "right": at(33.5, 8), "top": at(16, -1.5), "bottom": at(16, 17.5), "corner": at(-1, -1)}
    rgb = _colours(np.random.default_rng(5), 1)
    for name, p in cases.items():
        ref, _ = _both(np.array([p], F), rgb, leaf, None, view, name)
        assert ref["info"]["clamped"] == 1 and ref["stats"]["drawn"] == 1, name
        assert 0 < ref["stats"]["covered_pixels"] < 25, name                    # a part of the 5 x 5 centres it would cover
    ref, _ = _both(np.array(list(cases.values()) + [at(-3.0, 8), at(36.0, 8), at(16, -3.0), at(16, 20.0)], F),
                   _colours(np.random.default_rng(5), 9), leaf, None, view)
    assert ref["info"]["clamped"] == 5 and ref["stats"]["outside"] == 4


def test_projections_far_outside_the_int_range_and_nan_centroids():
    leaf, K = 0.05, (40, 40, 16.3, 8.1)
    view = make_view(33, 17, K, default_near(leaf, K))
    xyz = np.array([[1e30, 0, 1], [-1e30, 0, 1], [0, 3e38, 1], [0, -3e38, 1], [1e12, -1e12, 0.5], [0, 0, 1],
                    [np.nan, 0, 1], [0, np.nan, 1], [0, 0, np.nan], [np.inf, 0, 1], [0, 0, -1]], F)
    ref, _ = _both(xyz, _colours(np.random.default_rng(9), len(xyz)), leaf, None, view)
    # NaN and infinite coordinates reach cz through 0 * x: the near test is false for NaN
    assert ref["stats"] == {"voxels": 11, "behind_near": 5, "outside": 5, "drawn": 1, "covered_pixels": ref["stats"]["covered_pixels"]}
    assert set(np.unique(ref["index"])) == {-1, 5}


def test_render_entries_fail_loudly_without_a_gpu():
    from dvo_slam_amd import capi

    L = capi.lib()
    if L.dvo_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    view, st, h = capi.CView(4, 2, 1.0, 1.0, 0.0, 0.0, 1.0), capi.CRenderStats(), C.c_void_p()
    assert L.dvo_amd_map_render(None, None, C.byref(view), None, None, None, None, C.byref(st)) == 2
    assert L.dvo_amd_map_render_pyramid(None, None, C.byref(view), 1, 0.0, C.byref(h), C.byref(st)) == 2 and not h.value


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capi_gpu():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


def _step_pose(synth, k, scale=1.0):
    return synth.se3_exp(np.array([0.02 * k, -0.01 * k, 0.015 * k, 0.01 * k, -0.02 * k, 0.005 * k]) * scale)


@pytest.fixture(scope="module")
def frames(capi_gpu, synth):
    """the 8 overlapping 160x120 keyframes of tests/test_keyframe_map.py: small pose steps, a BGR image on every other one"""
    pyrs, bgrs = [], []
    for k in range(8):
        I, Z = synth.render(160, 120, _step_pose(synth, k), frame_id=k)
        bgr, raw = synth.to_raw(I, Z)
        pyrs.append(capi_gpu.RgbdImagePyramid.from_raw(bgr, raw, synth.intrinsics_for(160, 120), 1))
        bgrs.append(bgr if k % 2 == 0 else None)
    return pyrs, [_step_pose(synth, k) for k in range(8)], bgrs


def _build(capi, frames, leaf, order=range(8)):
    pyrs, poses, bgrs = frames
    trk = capi.DenseTracker()
    m = capi.KeyframeMap(trk, leaf)
    for k in order:
        m.insert(k, pyrs[k], poses[k], bgrs[k])
    return m


@pytest.fixture(scope="module")
def maps(capi_gpu, frames):
    """one map per leaf, shared by the tests (a render never changes the map), with its extract"""
    out = {}
    for leaf in (0.02, 0.05):
        m = _build(capi_gpu, frames, leaf)
        out[leaf] = (m, m.extract())
    return out


def _view_args(synth, name):
    if name == "odd":
        return (40, 40, 16.3, 8.1), 33, 17
    w, h = (160, 120) if name == "full" else (80, 60)
    return synth.intrinsics_for(w, h), w, h


def _ref(ext, leaf, pose, K, w, h, near=None):
    return render_ref(ext[0], ext[1], leaf, pose, make_view(w, h, K, default_near(leaf, K) if near is None else near))


@pytest.mark.gpu
@pytest.mark.parametrize("leaf", [0.02, 0.05])
@pytest.mark.parametrize("name", ["full", "half", "odd"])
def test_views(capi_gpu, synth, maps, leaf, name):
    m, ext = maps[leaf]
    K, w, h = _view_args(synth, name)
    pose = _step_pose(synth, 3.5)                                                # halfway between keyframes 3 and 4
    ref = _ref(ext, leaf, pose, K, w, h)
    print(leaf, name, ref["stats"], {k: v for k, v in ref["info"].items() if k != "candidates"}, int(ref["info"]["candidates"].max()))
    assert ref["info"]["coverage"] > 0.9 and ref["info"]["multi"] >= 0.1 * w * h  # the depth test decides: it cannot be left out
    got = m.render(pose, K, w, h)
    assert_same_render(got, ref, (leaf, name))
    assert same_bits(m.extract()[0], ext[0]) and same_bits(m.extract()[1], ext[1])  # a render never changes the map


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(64, 48), (160, 120)])
def test_large_footprints(capi_gpu, synth, maps, size):
    """The scene lies 2.4 m and more from the halfway pose: at 4 x the keyframes' focal length the restatement finds sides of 9
    pixels and nothing behind near_z, at 12 x sides of 27 and a few hundred voxels behind it.  The conditions are the assertion."""
    leaf = 0.05
    m, ext = maps[leaf]
    f = F(12) * synth.intrinsics_for(160, 120)[0]
    K = (f, f, (size[0] - 1) / 2, (size[1] - 1) / 2)
    near = near_limit(leaf, K)                                                   # exactly at the limit: sides of up to 32 pixels
    pose = _step_pose(synth, 3.5)
    ref = _ref(ext, leaf, pose, K, size[0], size[1], near)
    print(ref["stats"], {k: v for k, v in ref["info"].items() if k != "candidates"})
    assert ref["info"]["max_side"] >= 16                                         # the path the whole wave walks
    assert ref["stats"]["behind_near"] > 0 and ref["info"]["clamped"] > 0 and ref["info"]["multi"] > 0
    got = m.render(pose, K, size[0], size[1], near=near)
    assert_same_render(got, ref)


@pytest.mark.gpu
def test_geometry_independence(capi_gpu, synth, frames, maps):
    leaf = 0.05
    m, ext = maps[leaf]
    pyrs, poses, bgrs = frames
    K, w, h = _view_args(synth, "half")
    pose = _step_pose(synth, 3.5)
    ref = _ref(ext, leaf, pose, K, w, h)
    first = m.render(pose, K, w, h)
    assert_same_render(first, ref, "first")
    assert_same_render(m.render(pose, K, w, h), ref, "warm")                     # twice in a row into a warm workspace
    Kb, wb, hb = _view_args(synth, "full")
    assert_same_render(m.render(pose, Kb, wb, hb), _ref(ext, leaf, pose, Kb, wb, hb), "larger")
    assert_same_render(m.render(pose, K, w, h), ref, "after the buffers grew")
    other = _build(capi_gpu, frames, leaf, order=[5, 2, 7, 0, 3, 6, 1, 4])       # another insertion order
    assert_same_render(other.render(pose, K, w, h), ref, "order")
    other.set_poses([2], [synth.se3_exp([0.2, 0.1, -0.1, 0.02, 0.03, -0.01]) @ poses[2]])
    moved = other.render(pose, K, w, h)
    assert not same_bits(moved["depth"], ref["depth"])
    assert_same_render(moved, render_ref(*other.extract(), leaf, pose, make_view(w, h, K, default_near(leaf, K))), "moved")
    other.set_poses([2], [poses[2]])                                             # and back
    assert_same_render(other.render(pose, K, w, h), ref, "moved back")


@pytest.mark.gpu
def test_plane_selection(capi_gpu, synth, maps):
    leaf = 0.05
    m, ext = maps[leaf]
    K, w, h = _view_args(synth, "odd")
    pose = _step_pose(synth, 3.5)
    full = m.render(pose, K, w, h)
    for mask in range(16):
        planes = tuple(p for b, p in enumerate(PLANES) if mask >> b & 1)
        got = m.render(pose, K, w, h, planes=planes)
        assert set(got) == set(planes) | {"stats"} and got["stats"] == full["stats"], planes
        assert all(same_bits(got[p], full[p]) for p in planes), planes
    L = capi_gpu.lib()                                                           # NULL stats
    view = capi_gpu.CView(w, h, *[float(k) for k in K], float(default_near(leaf, K)))
    depth = np.empty((h, w), F)
    assert L.dvo_amd_map_render(m._h, None, C.byref(view), depth.ctypes.data, None, None, None, None) == 0
    assert same_bits(depth, m.render(None, K, w, h)["depth"])


@pytest.mark.gpu
def test_empty_and_degenerate(capi_gpu, synth, frames, maps):
    leaf = 0.05
    K, w, h = _view_args(synth, "half")
    empty = capi_gpu.KeyframeMap(capi_gpu.DenseTracker(), leaf)
    got = empty.render(None, K, w, h)
    none = np.zeros((0, 3), F), np.zeros(0, np.uint32)
    assert_same_render(got, _ref(none, leaf, None, K, w, h), "empty")
    assert got["stats"] == {"voxels": 0, "behind_near": 0, "outside": 0, "drawn": 0, "covered_pixels": 0}
    assert np.isnan(got["depth"]).all() and (got["index"] == -1).all() and not got["rgb"].any() and not got["intensity"].any()
    m, ext = maps[leaf]
    away = _step_pose(synth, 3.5) @ np.diag([-1.0, 1.0, -1.0, 1.0])              # turned round: everything is behind the camera
    got = m.render(away, K, w, h)
    assert_same_render(got, _ref(ext, leaf, away, K, w, h), "away")
    assert got["stats"]["drawn"] == 0 and got["stats"]["covered_pixels"] == 0 and (got["index"] == -1).all()
    assert got["stats"]["voxels"] == len(ext[0]) > 0
    pose = _step_pose(synth, 3.5)
    got = m.render(pose, (40, 40, 0, 0), 1, 1)
    assert_same_render(got, _ref(ext, leaf, pose, (40, 40, 0, 0), 1, 1), "1x1")
    assert got["depth"].shape == (1, 1) and got["stats"]["covered_pixels"] == 1


@pytest.mark.gpu
def test_pyramid(capi_gpu, synth, frames, maps):
    leaf = 0.02
    m, ext = maps[leaf]
    K, w, h = _view_args(synth, "full")
    pose = _step_pose(synth, 3.5)
    flat = m.render(pose, K, w, h)
    pyr = m.render_pyramid(pose, K, w, h, 3, timestamp=12.5)
    assert pyr.levels() == 3 and pyr.timestamp() == 12.5 and pyr.render_stats == flat["stats"]
    assert same_bits(pyr.plane(0, 0), flat["intensity"]) and same_bits(pyr.plane(0, 1), flat["depth"])
    host = capi_gpu.RgbdImagePyramid(flat["intensity"], flat["depth"], K, 3)     # the host constructor on the same data
    for level in range(3):
        assert pyr.level_info(level)[:2] == host.level_info(level)[:2] and same_bits(pyr.level_info(level)[2], host.level_info(level)[2])
        for plane in range(6):
            assert same_bits(pyr.plane(level, plane), host.plane(level, plane)), (level, plane)
    I, Z = synth.render(w, h, pose, frame_id=11)                                 # a live frame at the view's pose
    live = capi_gpu.RgbdImagePyramid(I, Z, K, 3)
    cfg = capi_gpu.Config(FirstLevel=2, LastLevel=0)
    res = capi_gpu.DenseTracker(cfg).match(pyr, live)
    its = [len(L["Iterations"]) for L in res.Levels]
    print("match(model view, frame): iterations per level", its, "xi", capi_gpu.se3_log(res.Transformation))
    assert not res.isNaN() and len(its) == 3
    assert all(0 < n < cfg.MaxIterationsPerLevel for n in its), its              # no level ran into the iteration limit


@pytest.mark.gpu
def test_errors(capi_gpu, synth, frames, maps):
    leaf = 0.05
    m, ext = maps[leaf]
    K, w, h = _view_args(synth, "half")
    pose = _step_pose(synth, 3.5)
    near = default_near(leaf, K)

    def rejected(call, word=None):
        with pytest.raises(capi_gpu.DvoAmdError) as e:
            call()
        assert e.value.status == 1, e.value                                      # DVO_AMD_ERR_INVALID_ARGUMENT
        if word:
            assert word in capi_gpu.lib().dvo_amd_last_error().decode(), capi_gpu.lib().dvo_amd_last_error()

    inf, nan = float("inf"), float("nan")
    views = [((K, 0, h), "width"), ((K, w, 0), "width"), ((K, -3, h), "width"), ((K, 1 << 13, (1 << 13) + 1), "2^26"),
             (((0.0, K[1], K[2], K[3]), w, h), "fx"), (((K[0], -1.0, K[2], K[3]), w, h), "fy"), (((inf, K[1], K[2], K[3]), w, h), "fx"),
             (((K[0], nan, K[2], K[3]), w, h), "fy"), (((K[0], K[1], nan, K[3]), w, h), "ox"), (((K[0], K[1], K[2], inf), w, h), "oy")]
    for (Kv, wv, hv), word in views:
        rejected(lambda: m.render(pose, Kv, wv, hv, near=near), word)
        rejected(lambda: m.render_pyramid(pose, Kv, wv, hv, 1, near=near), word)
    for bad in (0.0, -1.0, inf, nan):
        rejected(lambda: m.render(pose, K, w, h, near=bad), "near_z")
        rejected(lambda: m.render_pyramid(pose, K, w, h, 1, near=bad), "near_z")
    for e in (0, 5, 13, 15):
        P = np.array(pose)
        P.flat[e] = nan if e % 2 else inf
        rejected(lambda: m.render(P, K, w, h), "pose")
        rejected(lambda: m.render_pyramid(P, K, w, h, 1), "pose")
    limit = near_limit(leaf, K)                                                  # the footprint bound: one ulp decides
    rejected(lambda: m.render(pose, K, w, h, near=np.nextafter(limit, F(0))), "32")
    rejected(lambda: m.render_pyramid(pose, K, w, h, 1, near=np.nextafter(limit, F(0))), "32")
    got = m.render(pose, K, w, h, near=limit)
    assert_same_render(got, _ref(ext, leaf, pose, K, w, h, limit), "at the limit")
    rejected(lambda: m.render_pyramid(pose, K, w, h, 0))                         # the pyramid's own rules
    rejected(lambda: m.render_pyramid(pose, K, w, h, 4), "levels")               # 80 -> 40 -> 20 -> 10: not a multiple of 4
    rejected(lambda: m.render_pyramid(pose, (40, 40, 16.3, 8.1), 33, 17, 1), "levels")
    # pairs queued on the context
    trk = m._trk
    K4 = synth.intrinsics_for(320, 240)
    ref = capi_gpu.RgbdImagePyramid.from_raw(*synth.sensor_frame(320, 240, None, frame_id=0), K4, 4)
    nxt = capi_gpu.RgbdImagePyramid.from_raw(*synth.sensor_frame(320, 240, synth.se3_exp(synth.XI_GT_PAIR * 0.5), frame_id=1), K4, 4)
    sub = trk.submit([ref] * 4, [nxt] * 4, in_flight=4)
    try:
        rejected(lambda: m.render(pose, K, w, h), "in flight")
        rejected(lambda: m.render_pyramid(pose, K, w, h, 1), "in flight")
    finally:
        trk.wait(sub)
    after = m.extract()
    assert same_bits(after[0], ext[0]) and same_bits(after[1], ext[1])           # failed renders left the map as it was
    assert_same_render(m.render(pose, K, w, h), _ref(ext, leaf, pose, K, w, h), "after the errors")
