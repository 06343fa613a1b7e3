"""Rectification at ingest: dvo_amd_remap_* and dvo_amd_pyramid_create_raw_remapped (include/dvo_amd.h).

The undistortion rule and the sampling rule are pinned operation by operation in the header and restated in
tests/rectify_ref.py.  Every comparison of planes, maps and counts in this file is equality of bits or of integers; the one
tolerance is the stated cap of 1e-3 px between the float32 rule and the same formula in float64 (a condition on the rule, which
the restatement alone measures at about 1e-4 px for fr1's coefficients).
CPU: the restatement against its independent pixel loop on random and crafted cases, each crafted case asserting that it hits
its case; the argument checks that need no remap object, and NO_DEVICE of the entries that can be reached without one.
GPU: the library against the restatement; the argument checks of dvo_amd_pyramid_create_raw_remapped that need a remap (a remap
cannot exist without a device, so they and that entry's device errors live here).

GPU shapes (output <- source): 4x2 <- 5x3 the smallest legal shape; 72x50 (two levels) <- 80x60 sizes differ; 64x32 (three
levels) <- 64x32; 260x3 <- 300x7: 65 four-pixel lanes, one lane past a wave, odd heights."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rectify_ref import (bits, grey_plane, identity_maps, inside_ref, remap_brute, remap_ref, same_planes,  # noqa: E402
                         undistort_map_ref)

F = np.float32
INVALID, NO_DEVICE, MISMATCH = 1, 2, 8
SCALE = 1.0 / 5000.0
FR1_DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)
TANGENTIAL = (0.0, 0.0, 0.011, -0.007, 0.0)
ZERO = (0.0, 0.0, 0.0, 0.0, 0.0)


def _below(v):
    return np.nextafter(F(v), F(-np.inf))


def _frame(rng, sw, sh, channels, holes=0.2):
    image = rng.integers(0, 256, (sh, sw) if channels == 1 else (sh, sw, 3)).astype(np.uint8)
    depth = rng.integers(1, 65536, (sh, sw)).astype(np.uint16)
    depth[rng.uniform(size=(sh, sw)) < holes] = 0
    return image, depth


def _random_maps(rng, w, h, sw, sh):
    """maps of which a chosen share of 20..80 % of the pixels lies inside the source; the others reach beyond it on every side,
    some of them far"""
    n = w * h
    k = int(rng.integers(-(-n // 5), n * 4 // 5 + 1))                     # ceil(n / 5) .. floor(4 n / 5)
    ins = np.zeros(n, bool)
    ins[rng.permutation(n)[:k]] = True
    mx = rng.uniform(0, sw - 1, n).astype(F)
    my = rng.uniform(0, sh - 1, n).astype(F)
    mx, my = np.minimum(mx, _below(sw - 1)), np.minimum(my, _below(sh - 1))  # (the cast may have rounded up onto the edge)
    on_grid = rng.uniform(size=n) < 0.15                                  # some positions on whole pixels
    mx[on_grid] = np.floor(mx[on_grid])
    out = ~ins
    side = rng.integers(0, 4, n)
    far = rng.uniform(size=n) < 0.2
    reach = np.where(far, F(1e6), F(3.0)).astype(F)
    mx[out & (side == 0)] = (-rng.uniform(1e-3, 1, n).astype(F) * reach)[out & (side == 0)]
    mx[out & (side == 1)] = (F(sw - 1) + rng.uniform(0, 1, n).astype(F) * reach)[out & (side == 1)]
    my[out & (side == 2)] = (-rng.uniform(1e-3, 1, n).astype(F) * reach)[out & (side == 2)]
    my[out & (side == 3)] = (F(sh - 1) + rng.uniform(0, 1, n).astype(F) * reach)[out & (side == 3)]
    return mx.reshape(h, w), my.reshape(h, w)


def _both(image, depth, mx, my, scale=SCALE, what=None):
    I, Z, info = remap_ref(image, depth, mx, my, scale, info=True)
    Ib, Zb, nb = remap_brute(image, depth, mx, my, scale)
    assert same_planes(I, Ib) and same_planes(Z, Zb) and info["n_inside"] == nb, what
    assert not np.isnan(I).any() and (I[~info["inside"]] == 0).all() and np.isnan(Z[~info["inside"]]).all(), what
    return I, Z, info


# ---- CPU: the restatement against its pixel loop ------------------------------------------------------------------------------------

def test_restatement_matches_the_pixel_loop_on_random_cases():
    rng = np.random.default_rng(21)
    sources = [(5, 3), (9, 7), (13, 8), (17, 11), (24, 17)]
    outputs = [(4, 2), (8, 5), (12, 9), (16, 3), (20, 15)]
    seen_holes = seen_far = 0
    for k in range(40):
        (sw, sh), (w, h) = sources[k % 5], outputs[(k * 2 + k // 5) % 5]
        channels = (1, 3)[(k // 2) % 2]
        image, depth = _frame(rng, sw, sh, channels)
        mx, my = _random_maps(rng, w, h, sw, sh)
        I, Z, info = _both(image, depth, mx, my, (SCALE, 0.001)[k % 2], k)
        share = info["n_inside"] / (w * h)
        assert 0.2 <= share <= 0.8, (k, share)                            # a condition on the inputs
        seen_holes += int((info["raw"][info["inside"]] == 0).sum())
        seen_far += int((np.abs(mx) > 1e4).sum() + (np.abs(my) > 1e4).sum())
    assert seen_holes > 20 and seen_far > 20                              # depth holes under a tap, maps far beyond the source


def _row_case(sx_values, sw=6, sh=3, sy=F(1.0), channels=1, seed=3):
    """a one-row output whose pixel k sits at (sx_values[k], sy) of a random sw x sh source"""
    rng = np.random.default_rng(seed)
    image, depth = _frame(rng, sw, sh, channels, holes=0.0)
    mx = np.asarray(sx_values, F).reshape(1, -1)
    my = np.full_like(mx, sy)
    return (image, depth, mx, my) + _both(image, depth, mx, my)


def test_edges_of_the_source_in_x():
    sw = 6
    sx = [F(0.0), F(-0.0), _below(0.0), F(sw - 1), _below(sw - 1)]
    image, depth, mx, my, I, Z, info = _row_case(sx, sw=sw)
    assert np.signbit(mx[0, 1]) and mx[0, 1] == 0 and mx[0, 2] < 0 and mx[0, 4] < sw - 1 == mx[0, 3]
    assert list(info["inside"][0]) == [True, True, False, False, True]
    assert I[0, 0] == I[0, 1] == image[1, 0] and list(info["x0"][0, [0, 1, 4]]) == [0, 0, sw - 2]
    assert bits(I)[0, 1] == bits(F(image[1, 0]))                           # -0.0 is position 0, not a negative zero in the plane
    assert 0 < info["ax"][0, 4] < 1 and info["px"][0, 4] == sw - 1          # one ulp inside: the nearest depth tap is the last column
    assert Z[0, 4] == F(depth[1, sw - 1]) * F(SCALE)


def test_edges_of_the_source_in_y():
    rng = np.random.default_rng(4)
    sw, sh = 5, 4
    image, depth = _frame(rng, sw, sh, 3, holes=0.0)
    my = np.asarray([F(0.0), F(-0.0), _below(0.0), F(sh - 1), _below(sh - 1)], F).reshape(1, -1)
    mx = np.full_like(my, F(2.0))
    I, Z, info = _both(image, depth, mx, my)
    assert list(info["inside"][0]) == [True, True, False, False, True]
    assert I[0, 0] == I[0, 1] == grey_plane(image)[0, 2] and info["y0"][0, 4] == sh - 2 and info["py"][0, 4] == sh - 1


def test_non_finite_and_huge_positions_are_outside():
    sx = [np.nan, np.inf, -np.inf, F(8e30), F(-8e30), F(2.0)]
    image, depth, mx, my, I, Z, info = _row_case(sx)
    assert np.isnan(mx[0, 0]) and np.isinf(mx[0, 1:3]).all() and mx[0, 3] == F(8e30)
    assert list(info["inside"][0]) == [False] * 5 + [True] and info["n_inside"] == 1
    # the same entries in map_y
    I2, Z2, info2 = _both(image, depth, np.full((1, 6), F(2.0)), np.asarray(sx, F).reshape(1, -1))
    assert list(info2["inside"][0]) == [False] * 5 + [False]               # (sy = 2.0 is the last row of a 3-row source: outside)
    I3, Z3, info3 = _both(image, depth, np.full((1, 6), F(2.0)), np.asarray(sx[:5] + [F(1.0)], F).reshape(1, -1))
    assert list(info3["inside"][0]) == [False] * 5 + [True]


def test_a_position_on_a_whole_pixel_is_the_tap_exactly():
    image, depth, mx, my, I, Z, info = _row_case([F(0.0), F(1.0), F(3.0), F(4.0)], sw=6, sh=3, sy=F(1.0), channels=3)
    g = grey_plane(image)
    assert (info["ax"] == 0).all() and (info["ay"] == 0).all()
    assert list(I[0]) == [F(g[1, 0]), F(g[1, 1]), F(g[1, 3]), F(g[1, 4])]
    assert list(Z[0]) == [F(depth[1, k]) * F(SCALE) for k in (0, 1, 3, 4)]


def test_nearest_depth_tap_rounds_half_up_in_float():
    tie, below_tie = F(1.5), F(0.49999997)
    assert below_tie < F(0.5) and below_tie + F(0.5) == F(1.0)             # the fp32 sum rounds up to 1
    assert np.floor(np.float64(below_tie) + 0.5) == 0                      # ... where exact arithmetic would stay at 0
    image, depth, mx, my, I, Z, info = _row_case([tie, below_tie, _below(1.5), F(2.5)])
    assert list(info["px"][0]) == [2, 1, 1, 3] and list(info["x0"][0]) == [1, 0, 1, 2]
    assert list(Z[0]) == [F(depth[1, k]) * F(SCALE) for k in (2, 1, 1, 3)]
    # the same in y
    rng = np.random.default_rng(8)
    image, depth = _frame(rng, 4, 5, 1, holes=0.0)
    my = np.asarray([tie, below_tie], F).reshape(1, 2)
    I, Z, info = _both(image, depth, np.full((1, 2), F(1.0)), my)
    assert list(info["py"][0]) == [2, 1] and list(Z[0]) == [F(depth[2, 1]) * F(SCALE), F(depth[1, 1]) * F(SCALE)]


def test_a_depth_hole_under_the_nearest_tap_and_the_reverse():
    rng = np.random.default_rng(9)
    image, depth = _frame(rng, 6, 4, 1, holes=0.0)
    # pixel 0 at (1.75, 1.25): nearest tap (2, 1) is a hole, the intensity taps (1..2, 1..2) are what they are
    # pixel 1 at (3.25, 1.25): nearest tap (3, 1) is measured, the other three depth pixels under the intensity taps are holes
    depth[1, 2] = 0
    depth[1, 4] = depth[2, 3] = depth[2, 4] = 0
    mx, my = np.asarray([[1.75, 3.25]], F), np.asarray([[1.25, 1.25]], F)
    I, Z, info = _both(image, depth, mx, my)
    assert info["inside"].all() and list(info["px"][0]) == [2, 3] and list(info["py"][0]) == [1, 1]
    assert np.isnan(Z[0, 0]) and I[0, 0] > 0 and list(info["raw"][0]) == [0, depth[1, 3]]
    assert Z[0, 1] == F(depth[1, 3]) * F(SCALE)                            # never blended with the holes next to it
    lo, hi = image[1:3, 1:3].min(), image[1:3, 1:3].max()
    assert lo <= I[0, 0] <= hi


def test_an_all_outside_map_and_the_identity_map():
    rng = np.random.default_rng(10)
    sw, sh = 8, 5
    for channels in (1, 3):
        image, depth = _frame(rng, sw, sh, channels)
        mx, my = identity_maps(sw, sh)
        I, Z, info = _both(image, depth, mx + F(sw), my)
        assert info["n_inside"] == 0 and (I == 0).all() and np.isnan(Z).all()
        I, Z, info = _both(image, depth, mx, my)
        assert info["n_inside"] == (sw - 1) * (sh - 1)
        g = grey_plane(image).astype(F)
        z = np.where(depth == 0, F(np.nan), depth.astype(F) * F(SCALE)).astype(F)
        assert same_planes(I[:-1, :-1], g[:-1, :-1]) and same_planes(Z[:-1, :-1], z[:-1, :-1])
        assert (I[-1] == 0).all() and (I[:, -1] == 0).all() and np.isnan(Z[-1]).all() and np.isnan(Z[:, -1]).all()


def test_float32_undistortion_stays_within_the_cap_of_the_float64_formula():
    from dvo_slam_amd import tum

    K = tum.TUM_FR1_INTRINSICS
    mx, my = undistort_map_ref((640, 480), K, (640, 480), K, FR1_DIST)
    mx64, my64 = undistort_map_ref((640, 480), K, (640, 480), K, FR1_DIST, dtype=np.float64)
    assert mx.dtype == F and mx64.dtype == np.float64
    err = max(np.abs(mx - mx64).max(), np.abs(my - my64).max())
    print("float32 against float64, fr1 at 640x480: %.3g px" % err)
    assert err <= 1e-3                                                     # the stated cap
    u, v = identity_maps(640, 480)
    shift = np.hypot(mx64 - u, my64 - v)
    assert 20 < shift[0, 0] < 40                                           # a corner pixel moves by tens of pixels: the lens matters


def test_zero_coefficients_give_the_identity():
    from dvo_slam_amd import tum

    K = tum.TUM_FR1_INTRINSICS
    u, v = identity_maps(640, 480)
    mx, my = undistort_map_ref((640, 480), K, (640, 480), K, ZERO)
    assert max(np.abs(mx - u).max(), np.abs(my - v).max()) <= 1e-3         # the same cap
    K2 = (512.0, 256.0, 320.0, 240.0)                                      # power-of-two focal lengths, whole principal point
    mx, my = undistort_map_ref((640, 480), K2, (640, 480), K2, ZERO)
    assert np.array_equal(mx, u) and np.array_equal(my, v)                  # exact


# ---- CPU: the library's argument checks -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _invalid(capi, rc, *words):
    assert rc == INVALID, rc
    text = capi.lib().dvo_amd_last_error().decode()
    assert all(w in text for w in words), text


def test_remap_create_argument_checks(capi):
    L = capi.lib()
    m = np.zeros((4, 16), F)
    h = C.c_void_p()
    ok = dict(device=0, width=8, height=4, map_x=_fp(m), map_y=_fp(m), stride=16, src_width=5, src_height=3, out=C.byref(h))

    def call(**kw):
        a = dict(ok, **kw)
        return L.dvo_amd_remap_create(a["device"], a["width"], a["height"], a["map_x"], a["map_y"], a["stride"], a["src_width"],
                                      a["src_height"], a["out"])

    for name in ("map_x", "map_y", "out"):
        _invalid(capi, call(**{name: None}), "dvo_amd_remap_create", "NULL")
    for kw in (dict(width=0), dict(width=6), dict(width=-4), dict(height=1), dict(width=1 << 16, height=1 << 15, stride=1 << 16)):
        _invalid(capi, call(**kw), "dvo_amd_remap_create:")
    _invalid(capi, call(stride=7), "stride")
    for kw in (dict(src_width=1), dict(src_height=1), dict(src_width=0), dict(src_height=-3), dict(src_width=(1 << 20) + 1)):
        _invalid(capi, call(**kw), "source")
    assert not h.value


def test_remap_create_undistort_argument_checks(capi):
    L = capi.lib()
    k = np.asarray([500, 500, 4, 2], F)
    d = np.zeros(5, F)
    h = C.c_void_p()
    ok = dict(device=0, width=8, height=4, k_out=k, src_width=9, src_height=5, k_src=k, dist=d, out=C.byref(h))

    def call(**kw):
        a = dict(ok, **kw)
        f = lambda v: None if v is None else _fp(v)
        return L.dvo_amd_remap_create_undistort(a["device"], a["width"], a["height"], f(a["k_out"]), a["src_width"], a["src_height"],
                                                f(a["k_src"]), f(a["dist"]), a["out"])

    for name in ("k_out", "k_src", "dist", "out"):
        _invalid(capi, call(**{name: None}), "dvo_amd_remap_create_undistort", "NULL")
    for kw in (dict(width=0), dict(width=10), dict(height=1), dict(src_width=1), dict(src_height=1)):
        _invalid(capi, call(**kw), "dvo_amd_remap_create_undistort:")
    for bad in (np.nan, np.inf, -np.inf):
        for name, n in (("k_out", 4), ("k_src", 4), ("dist", 5)):
            for at in range(n):
                v = (k if n == 4 else d).copy()
                v[at] = bad
                _invalid(capi, call(**{name: v}), "non-finite")
    for name in ("k_out", "k_src"):
        for at in (0, 1):
            for bad in (0.0, -500.0):
                v = k.copy()
                v[at] = bad
                _invalid(capi, call(**{name: v}), "positive")
    assert not h.value


def test_argument_checks_that_need_no_remap(capi):
    L = capi.lib()
    img, z = np.zeros((3, 5), np.uint8), np.zeros((3, 5), np.uint16)
    h = C.c_void_p()
    # a NULL remap, image, depth or out is refused before anything else is looked at
    for image, depth, out in ((None, z.ctypes.data, C.byref(h)), (img.ctypes.data, None, C.byref(h)), (img.ctypes.data, z.ctypes.data, C.byref(h)),
                              (img.ctypes.data, z.ctypes.data, None)):
        _invalid(capi, L.dvo_amd_pyramid_create_raw_remapped(0, image, 1, 5, depth, 5, SCALE, 0, None, 1.0, 1.0, 0.0, 0.0, 1, 0.0, out),
                 "dvo_amd_pyramid_create_raw_remapped", "NULL")
    ip = C.POINTER(C.c_int)
    _invalid(capi, L.dvo_amd_remap_info(None, ip(), ip(), ip(), ip(), ip()), "dvo_amd_remap_info")
    m = np.zeros(8, F)
    _invalid(capi, L.dvo_amd_remap_download(None, _fp(m), _fp(m)), "dvo_amd_remap_download")
    L.dvo_amd_remap_retain(None)                                           # both accept NULL, like the pyramid's
    L.dvo_amd_remap_release(None)


def test_remap_entries_fail_loudly_without_a_gpu(capi):
    if capi.lib().dvo_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    m = np.zeros((2, 4), F)
    with pytest.raises(capi.DvoAmdError) as e:
        capi.Remap.from_maps(m, m, (5, 3))
    assert e.value.status == NO_DEVICE
    with pytest.raises(capi.DvoAmdError) as e:
        capi.Remap.undistort((8, 4), (8, 8, 4, 2), (8, 4), (8, 8, 4, 2), ZERO)
    assert e.value.status == NO_DEVICE
    # (dvo_amd_pyramid_create_raw_remapped needs a remap, which needs a device: its NO_DEVICE cannot be reached from outside)


def test_header_and_binding_name_the_new_entries(capi):
    names = ["dvo_amd_remap_create", "dvo_amd_remap_create_undistort", "dvo_amd_remap_retain", "dvo_amd_remap_release",
             "dvo_amd_remap_info", "dvo_amd_remap_download", "dvo_amd_pyramid_create_raw_remapped"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dvo_amd.h")).read()
    for n in names:
        assert n + "(" in header and n in capi.EXPORTS and hasattr(capi.lib(), n), n
    assert capi.lib().dvo_amd_abi_version() == 3                           # purely additive


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

SHAPES = [((4, 2), (5, 3), 1), ((72, 50), (80, 60), 2), ((64, 32), (64, 32), 3), ((260, 3), (300, 7), 1)]
KINDS = ["host", "host_strided", "device", "device_offset_strided"]


def _crafted(mx, my, sw, sh):
    """the crafted positions of the CPU cases written over the first pixels of a random map (as many as the output holds)"""
    sx = [F(0.0), F(-0.0), _below(0.0), F(sw - 1), _below(sw - 1), np.nan, np.inf, -np.inf, F(8e30), F(1.0), F(1.5), F(0.49999997)]
    sy = [F(0.0), F(-0.0), _below(0.0), F(sh - 1), _below(sh - 1), np.nan, np.inf, -np.inf, F(8e30), F(1.0), F(1.5), F(0.49999997)]
    fx, fy = mx.reshape(-1), my.reshape(-1)
    n = min(len(sx), fx.size // 2)
    fx[:n], fy[:n] = sx[:n], F(1.0) if sh > 2 else F(0.5)
    fy[n:2 * n], fx[n:2 * n] = sy[:n], F(1.0)
    return mx, my


@pytest.fixture(scope="module")
def cases():
    """per shape and channel count: the frame, the maps, the restatement's planes and count -- computed once, never written to"""
    rng = np.random.default_rng(33)
    out = {}
    for (w, h), (sw, sh), levels in SHAPES:
        mx, my = _crafted(*_random_maps(rng, w, h, sw, sh), sw, sh)
        for channels in (1, 3):
            image, depth = _frame(rng, sw, sh, channels)
            I, Z, info = remap_ref(image, depth, mx, my, SCALE, info=True)
            for a in (image, depth, mx, my, I, Z):
                a.setflags(write=False)
            out[(w, h), channels] = dict(size=(w, h), src=(sw, sh), levels=levels, image=image, depth=depth, mx=mx, my=my, I=I, Z=Z,
                                         n_inside=info["n_inside"], K=(F(0.9 * w), F(0.95 * w), F(w / 2 - 0.3), F(h / 2 + 0.2)))
    return out


def _gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")


def _all_planes_equal(p, q, levels, what):
    assert p.levels() == q.levels() == levels
    for level in range(levels):
        assert p.level_info(level)[:2] == q.level_info(level)[:2] and np.array_equal(p.level_info(level)[2], q.level_info(level)[2])
        for plane in range(6):
            assert same_planes(p.plane(level, plane), q.plane(level, plane)), (what, level, plane)


def _ingest(capi, c, remap, kind):
    """the pyramid of case c through `remap`, the raw frame handed over in one of the four ways"""
    image, depth = c["image"], c["depth"]
    sw, sh = c["src"]
    channels = 1 if image.ndim == 2 else 3
    row = sw * channels
    if kind == "host":
        return capi.RgbdImagePyramid.from_raw(image, depth, c["K"], c["levels"], depth_scale=SCALE, remap=remap)
    istride, zstride = row + 5, sw + 3                                      # rows that break the 4- and 8-byte alignment
    wide_i = np.full((sh, istride), 0xAB, np.uint8)
    wide_i[:, :row] = image.reshape(sh, row)
    wide_z = np.full((sh, zstride), 0x1234, np.uint16)
    wide_z[:, :sw] = depth
    if kind == "host_strided":
        return capi.RgbdImagePyramid._raw(wide_i.ctypes.data, channels, istride, wide_z.ctypes.data, zstride, SCALE, 0, sw, sh, c["K"],
                                          c["levels"], 0, 0.0, remap)
    import torch

    if kind == "device":
        d_i, d_z = torch.from_numpy(image.copy()).cuda(), torch.from_numpy(depth.view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        return capi.RgbdImagePyramid.from_raw_device(d_i.data_ptr(), channels, d_z.data_ptr(), sw, sh, c["K"], c["levels"],
                                                     depth_scale=SCALE, remap=remap)
    # the base pointers one element past an aligned address, and the wide rows
    buf_i = torch.zeros(wide_i.size + 1, dtype=torch.uint8, device="cuda")
    buf_i[1:] = torch.from_numpy(wide_i.reshape(-1)).cuda()
    buf_z = torch.zeros(wide_z.size + 1, dtype=torch.int16, device="cuda")
    buf_z[1:] = torch.from_numpy(wide_z.view(np.int16).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return capi.RgbdImagePyramid.from_raw_device(buf_i.data_ptr() + 1, channels, buf_z.data_ptr() + 2, sw, sh, c["K"], c["levels"],
                                                 depth_scale=SCALE, image_stride_bytes=istride, depth_stride=zstride, remap=remap)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", [s[0] for s in SHAPES], ids=lambda s: "%dx%d" % s)
def test_remapped_pyramid_equals_the_host_constructor_on_the_restatement(capi, cases, shape, channels, kind):
    _gpu(capi)
    if kind.startswith("device"):
        pytest.importorskip("torch")
    c = cases[shape, channels]
    remap = capi.Remap.from_maps(c["mx"], c["my"], c["src"])
    info = remap.info()
    assert (info["width"], info["height"]) == c["size"] and (info["src_width"], info["src_height"]) == c["src"]
    assert info["n_inside"] == c["n_inside"] and 0 < c["n_inside"] < shape[0] * shape[1]
    dx, dy = remap.download()
    assert np.array_equal(bits(dx), bits(c["mx"])) and np.array_equal(bits(dy), bits(c["my"]))   # NaN and -0.0 entries included
    p = _ingest(capi, c, remap, kind)
    q = capi.RgbdImagePyramid(c["I"], c["Z"], c["K"], c["levels"])
    _all_planes_equal(p, q, c["levels"], (shape, channels, kind))
    assert same_planes(p.plane(0, 0), c["I"]) and same_planes(p.plane(0, 1), c["Z"])


@pytest.mark.gpu
@pytest.mark.parametrize("dist", [ZERO, FR1_DIST, TANGENTIAL], ids=["zero", "fr1", "tangential"])
def test_undistortion_map_equals_the_restatement_bit_for_bit(capi, dist):
    _gpu(capi)
    from dvo_slam_amd import tum

    for (w, h), (sw, sh), _ in SHAPES + [((640, 480), (640, 480), 4)]:
        if (w, h) == (640, 480):
            k_out = k_src = tum.TUM_FR1_INTRINSICS
        else:
            k_out = (0.81 * w, 0.83 * w, w / 2 - 0.3, h / 2 + 0.2)
            k_src = (0.8 * sw, 0.82 * sw, sw / 2 + 0.4, sh / 2 - 0.1)
        remap = capi.Remap.undistort((w, h), k_out, (sw, sh), k_src, dist)
        mx, my = undistort_map_ref((w, h), k_out, (sw, sh), k_src, dist)
        dx, dy = remap.download()
        assert np.array_equal(bits(dx), bits(mx)) and np.array_equal(bits(dy), bits(my)), (w, h, dist)
        n_inside = int(inside_ref(mx, my, (sw, sh)).sum())
        assert remap.info() == dict(width=w, height=h, src_width=sw, src_height=sh, n_inside=n_inside)
        if (w, h) == (640, 480):
            assert 0.5 * w * h < n_inside < w * h


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 3])
def test_identity_map_reproduces_the_plain_raw_ingest(capi, channels):
    _gpu(capi)
    rng = np.random.default_rng(35)
    w, h = 72, 50
    image, depth = _frame(rng, w, h, channels)
    K = (60.0, 61.0, 35.5, 24.5)
    mx, my = identity_maps(w, h)
    remap = capi.Remap.from_maps(mx, my, (w, h))
    assert remap.info()["n_inside"] == (w - 1) * (h - 1)
    p = capi.RgbdImagePyramid.from_raw(image, depth, K, 1, depth_scale=SCALE, remap=remap)
    q = capi.RgbdImagePyramid.from_raw(image, depth, K, 1, depth_scale=SCALE)
    for plane in (0, 1):
        a, b = p.plane(0, plane), q.plane(0, plane)
        assert same_planes(a[:-1, :-1], b[:-1, :-1])
        rim = np.concatenate([a[-1], a[:, -1]])
        assert (rim == 0).all() if plane == 0 else np.isnan(rim).all()
    all_out = capi.Remap.from_maps(mx + F(w), my, (w, h))
    assert all_out.info()["n_inside"] == 0
    p = capi.RgbdImagePyramid.from_raw(image, depth, K, 1, depth_scale=SCALE, remap=all_out)
    assert (p.plane(0, 0) == 0).all() and np.isnan(p.plane(0, 1)).all()


def _same_result(a, b):
    assert np.array_equal(a.Transformation, b.Transformation) and np.array_equal(a.Information, b.Information)
    assert a.LogLikelihood == b.LogLikelihood and a.isNaN() == b.isNaN() and len(a.Levels) == len(b.Levels)
    for la, lb in zip(a.Levels, b.Levels):
        assert (la["Id"], la["ValidPixels"], la["MaxValidPixels"], la["TerminationCriterion"], len(la["Iterations"])) == \
               (lb["Id"], lb["ValidPixels"], lb["MaxValidPixels"], lb["TerminationCriterion"], len(lb["Iterations"]))


@pytest.fixture(scope="module")
def sensor_case(synth):
    w, h = 160, 120
    (gr, zr), (gc, zc), _ = synth.sensor_pair(w, h, xi_gt=synth.XI_GT_PAIR * 0.5)
    K = synth.intrinsics_for(w, h)
    dist = (0.12, -0.2, 0.002, -0.001, 0.05)
    mx, my = undistort_map_ref((w, h), K, (w, h), K, dist)
    planes = [remap_ref(g, z, mx, my, SCALE) for g, z in ((gr, zr), (gc, zc))]
    return dict(size=(w, h), K=K, dist=dist, frames=((gr, zr), (gc, zc)), planes=planes, n_inside=int(inside_ref(mx, my, (w, h)).sum()))


@pytest.mark.gpu
def test_match_on_remapped_frames_equals_match_on_the_restatement_planes(capi, sensor_case):
    _gpu(capi)
    s = sensor_case
    remap = capi.Remap.undistort(s["size"], s["K"], s["size"], s["K"], s["dist"])
    assert remap.info()["n_inside"] == s["n_inside"] > 0.8 * 160 * 120
    trk = capi.DenseTracker(capi.Config(FirstLevel=2, LastLevel=0))
    ref, cur = [capi.RgbdImagePyramid.from_raw(g, z, s["K"], 3, depth_scale=SCALE, remap=remap) for g, z in s["frames"]]
    href, hcur = [capi.RgbdImagePyramid(I, Z, s["K"], 3) for I, Z in s["planes"]]
    a, b = trk.match(ref, cur), trk.match(href, hcur)
    assert not a.isNaN() and sum(len(l["Iterations"]) for l in a.Levels) >= 3
    _same_result(a, b)


@pytest.mark.gpu
def test_one_remap_shared_by_many_frames_and_two_trackers(capi, sensor_case, cases):
    _gpu(capi)
    s = sensor_case
    remap = capi.Remap.undistort(s["size"], s["K"], s["size"], s["K"], s["dist"])
    trackers = [capi.DenseTracker(capi.Config(FirstLevel=2, LastLevel=0)) for _ in range(2)]
    href, hcur = [capi.RgbdImagePyramid(I, Z, s["K"], 3) for I, Z in s["planes"]]
    want = trackers[0].match(href, hcur)
    small, small_map = cases[(4, 2), 3], None
    for k in range(3):
        # staging: this frame (160x120), then a smaller source (5x3) in the warm area, then this one again; the first round grows it
        ref, cur = [capi.RgbdImagePyramid.from_raw(g, z, s["K"], 3, depth_scale=SCALE, remap=remap) for g, z in s["frames"]]
        small_map = capi.Remap.from_maps(small["mx"], small["my"], small["src"])
        tiny = capi.RgbdImagePyramid.from_raw(small["image"], small["depth"], small["K"], 1, depth_scale=SCALE, remap=small_map)
        assert same_planes(tiny.plane(0, 0), small["I"]) and same_planes(tiny.plane(0, 1), small["Z"])
        _same_result(trackers[k % 2].match(ref, cur), want)
        _same_result(trackers[(k + 1) % 2].match(ref, cur), want)
    # a larger source than any before: the staging area is regrown, and the small one still works afterwards
    big = cases[(260, 3), 3]
    big_map = capi.Remap.from_maps(big["mx"], big["my"], big["src"])
    rng = np.random.default_rng(36)
    image, depth = _frame(rng, 320, 200, 3)
    mx, my = _random_maps(rng, 64, 32, 320, 200)
    wide = capi.Remap.from_maps(mx, my, (320, 200))
    I, Z = remap_ref(image, depth, mx, my, SCALE)
    p = capi.RgbdImagePyramid.from_raw(image, depth, (50, 50, 32, 16), 2, depth_scale=SCALE, remap=wide)
    assert same_planes(p.plane(0, 0), I) and same_planes(p.plane(0, 1), Z)
    for c, m in ((big, big_map), (small, small_map)):
        q = capi.RgbdImagePyramid.from_raw(c["image"], c["depth"], c["K"], 1, depth_scale=SCALE, remap=m)
        assert same_planes(q.plane(0, 0), c["I"]) and same_planes(q.plane(0, 1), c["Z"])
    # release order: the remap before the pyramid built through it, and the reverse
    ref = capi.RgbdImagePyramid.from_raw(*s["frames"][0], s["K"], 3, depth_scale=SCALE, remap=remap)
    cur = capi.RgbdImagePyramid.from_raw(*s["frames"][1], s["K"], 3, depth_scale=SCALE, remap=remap)
    del remap
    _same_result(trackers[0].match(ref, cur), want)
    remap = capi.Remap.undistort(s["size"], s["K"], s["size"], s["K"], s["dist"])
    cur = capi.RgbdImagePyramid.from_raw(*s["frames"][1], s["K"], 3, depth_scale=SCALE, remap=remap)
    del cur
    assert remap.info()["n_inside"] == s["n_inside"]
    # retain / release through the C ABI: the object outlives the first release
    L = capi.lib()
    L.dvo_amd_remap_retain(remap._h)
    L.dvo_amd_remap_release(remap._h)
    assert remap.download()[0].shape == (120, 160)


@pytest.mark.gpu
def test_argument_and_device_checks_that_need_a_remap(capi, cases):
    _gpu(capi)
    L = capi.lib()
    c = cases[(72, 50), 3]
    sw, sh = c["src"]
    remap = capi.Remap.from_maps(c["mx"], c["my"], c["src"])
    image, depth = c["image"], c["depth"]
    h = C.c_void_p()

    def call(device=0, channels=3, istride=sw * 3, zstride=sw, scale=SCALE, levels=2, rm=remap._h):
        return L.dvo_amd_pyramid_create_raw_remapped(device, image.ctypes.data, channels, istride, depth.ctypes.data, zstride, scale, 0, rm,
                                                     1.0, 1.0, 0.0, 0.0, levels, 0.0, C.byref(h))

    _invalid(capi, call(channels=2), "channels")
    _invalid(capi, call(channels=0), "channels")
    _invalid(capi, call(scale=0.0), "depth_scale")
    _invalid(capi, call(scale=float("nan")), "depth_scale")
    _invalid(capi, call(istride=sw * 3 - 1), "stride")
    _invalid(capi, call(zstride=sw - 1), "stride")
    _invalid(capi, call(channels=1, istride=sw - 1), "stride")
    _invalid(capi, call(levels=0), "levels")
    _invalid(capi, call(levels=9), "levels")
    _invalid(capi, call(levels=3), "level 2")                               # 72x50 holds two levels: 18 is no multiple of 4
    assert not h.value
    assert call(device=1) == MISMATCH and not h.value                       # a remap of device 0 asked to serve device 1
    assert call() == 0 and h.value
    L.dvo_amd_pyramid_release(h)
    # the Python binding refuses a raw frame that does not have the remap's source size before the library sees it
    with pytest.raises(ValueError):
        capi.RgbdImagePyramid.from_raw(image[:-1], depth[:-1], c["K"], 1, remap=remap)
