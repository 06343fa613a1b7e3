"""Depth-to-colour registration at ingest: dvo_amd_pyramid_create_raw_registered (include/dvo_amd.h).

The registration rule is pinned operation by operation in the header and restated in tests/register_ref.py.  Every comparison
of planes and counters in this file is equality of bits or of integers.  The tolerances are the fidelity test's: a median error
of one step of the 1/5000 m quantisation (2e-4 m) against the scene rendered at the colour camera, and a factor of 3 of the 4
that geometry gives between the footprint and the single-pixel coverage of a half-resolution depth frame; the restatement alone
measures them.
CPU: the restatement against its independent pixel loop on random and crafted cases, each crafted case asserting that it hits
its case; the identity consequence; the fidelity of the rule; every argument check and NO_DEVICE.
GPU: the library against the restatement.

GPU shapes (depth frame -> output): 1x1 -> 4x2 the smallest; 5x3 -> 4x2; 65x3 -> 64x32 one lane past a wave, three levels;
257x2 -> 72x50 one lane past a block, two levels; 80x60 -> 160x120 the half-resolution depth camera."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rectify_ref import grey_plane, remap_ref, same_planes  # noqa: E402
from register_ref import COUNTERS, bits, register_brute, register_ref, same_plane  # noqa: E402

F = np.float32
INVALID, NO_DEVICE, MISMATCH = 1, 2, 8
SCALE = 1.0 / 5000.0
EMPTY = 0x7FC00000
XI_DEPTH_TO_COLOUR = [0.025, 0.001, -0.004, 0.003, -0.005, 0.002]


def _below(v):
    return np.nextafter(F(v), F(-np.inf))


def _above(v):
    return np.nextafter(F(v), F(np.inf))


def _colour_K(w, h):
    return (F(0.9 * w), F(0.95 * h), F(w / 2 - 0.3), F(h / 2 + 0.2))


def _random_case(rng, dsize, size, fill, synth, holes=0.2):
    """a random depth frame, a small rigid transform and a depth camera whose field of view is wider than the colour camera's by
    a drawn factor, redrawn until 20..80 % of the measurements are drawn (a frame of fewer than 5 measurements cannot be asked
    for a share: it is taken as it comes)"""
    dw, dh = dsize
    w, h = size
    K = _colour_K(w, h)
    depth = rng.integers(1, 65536, (dh, dw)).astype(np.uint16)
    depth[rng.uniform(size=(dh, dw)) < holes] = 0
    if not depth.any():
        depth[0, 0] = 4000
    min_z = float(rng.choice([0.0, 2.0]))
    for _ in range(200):
        s = rng.uniform(0.45, 0.9, 2)
        K_depth = (F(s[0] * dw), F(s[1] * dh), F(dw / 2 + rng.uniform(-0.4, 0.4)), F(dh / 2 + rng.uniform(-0.4, 0.4)))
        T = synth.se3_exp(rng.uniform(-1, 1, 6) * [0.05, 0.05, 0.05, 0.02, 0.02, 0.02])
        case = dict(depth=depth, scale=SCALE, K_depth=K_depth, T=T, min_z=min_z, fill=fill, size=size, K=K)
        plane, st = _ref(case)
        if st["measurements"] < 5 or 0.2 * st["measurements"] <= st["drawn"] <= 0.8 * st["measurements"]:
            return case, plane, st
    raise AssertionError("no case with 20..80 % drawn")


def _args(c):
    return c["depth"], c["scale"], c["K_depth"], c["T"], c["min_z"], c["fill"], c["size"], c["K"]


def _ref(c, **kw):
    return register_ref(*_args(c), **kw)


def _both(c):
    a, sa = _ref(c)
    b, sb = register_brute(*_args(c))
    assert same_plane(a, b) and sa == sb, (sa, sb)
    assert sa["measurements"] == sa["behind"] + sa["outside"] + sa["drawn"] == int(np.count_nonzero(c["depth"]))
    assert sa["covered_pixels"] == int((bits(a) != EMPTY).sum())
    return a, sa


def test_restatement_matches_the_pixel_loop_on_random_cases(synth):
    rng = np.random.default_rng(41)
    shares = []
    for k in range(40):
        dsize = (1, 1) if k == 0 else (24, 17) if k == 1 else (int(rng.integers(1, 25)), int(rng.integers(1, 18)))
        size = (4, 2) if k == 0 else (20, 15) if k == 1 else (4 * int(rng.integers(1, 6)), int(rng.integers(2, 16)))
        case, _, st = _random_case(rng, dsize, size, k % 2, synth)
        _both(case)
        if st["measurements"] >= 5:
            assert 0.2 * st["measurements"] <= st["drawn"] <= 0.8 * st["measurements"]
            shares.append(st["drawn"] / st["measurements"])
    assert len(shares) >= 30


# ---- crafted cases: one measurement (or a few) whose colour-frame position is set through the translation ------------------------
# A 1x1 depth frame with k_depth = (1, 1, 0, 0), depth_scale 1 and T = (I | t) has rx = ry = 0, X = Y = 0 and so, exactly,
# cx = tx, cy = ty, cz = d + tz; with K = (1, 1, 0, 0) and cz = 1 that is uc = tx, vc = ty.

def _point(tx=1.0, ty=1.0, tz=0.0, d=1, size=(8, 4), fill=0, min_z=0.0, K=(1.0, 1.0, 0.0, 0.0), K_depth=(1.0, 1.0, 0.0, 0.0), scale=1.0):
    T = np.eye(4)
    T[:3, 3] = [float(tx), float(ty), float(tz)]
    return dict(depth=np.array([[d]], np.uint16), scale=scale, K_depth=K_depth, T=T, min_z=min_z, fill=fill, size=size, K=K)


def _pixels(plane):
    """{(x, y): value} of the covered pixels"""
    ys, xs = np.nonzero(bits(plane) != EMPTY)
    return {(int(x), int(y)): float(plane[y, x]) for x, y in zip(xs, ys)}


def _crafted():
    """(name, case, expected counters without measurements, expected pixels or None): shared by the CPU and the GPU test"""
    W, H = 8, 4
    out = []

    def add(name, case, behind, outside, drawn, pixels):
        out.append((name, case, dict(behind=behind, outside=outside, drawn=drawn), pixels))

    add("raw 0", _point(d=0), 0, 0, 0, {})
    add("cz exactly 0", _point(d=3, tz=-3.0), 1, 0, 0, {})
    add("cz negative", _point(d=3, tz=-5.0), 1, 0, 0, {})
    add("cz equal to min_z", _point(d=3, tz=-2.5, min_z=0.5), 1, 0, 0, {})
    add("cz one ulp above min_z", _point(tx=0.0, ty=0.0, d=3, tz=float(_above(-2.5)), min_z=0.5), 0, 0, 1, {(0, 0): float(F(3) + _above(-2.5))})
    for fill in (0, 1):
        # with fill the footprint of cz = z and mx = 1 is half a pixel wide: ceilf(uc - .5) .. floorf(uc + .5)
        add("uc + 0.5 on a whole number, fill %d" % fill, _point(tx=1.5, fill=fill), 0, 0, 1, {(2, 1): 1.0} if not fill else {(1, 1): 1.0, (2, 1): 1.0})
        add("uc + 0.5 one ulp below 0, fill %d" % fill, _point(tx=_below(-0.5), fill=fill), 0, 1, 0, {})
        add("uc + 0.5 on 0, fill %d" % fill, _point(tx=-0.5, fill=fill), 0, 0, 1, {(0, 1): 1.0})
        add("uc + 0.5 on width, fill %d" % fill, _point(tx=W - 0.5, fill=fill), 0, 1 - fill, fill, {} if not fill else {(W - 1, 1): 1.0})
        add("uc + 0.5 one ulp below width, fill %d" % fill, _point(tx=_below(W - 0.5), fill=fill), 0, 0, 1, {(W - 1, 1): 1.0})
        add("vc + 0.5 on a whole number, fill %d" % fill, _point(ty=1.5, fill=fill), 0, 0, 1, {(1, 2): 1.0} if not fill else {(1, 1): 1.0, (1, 2): 1.0})
        add("vc + 0.5 one ulp below 0, fill %d" % fill, _point(ty=_below(-0.5), fill=fill), 0, 1, 0, {})
        add("vc + 0.5 on height, fill %d" % fill, _point(ty=H - 0.5, fill=fill), 0, 1 - fill, fill, {} if not fill else {(1, H - 1): 1.0})
        add("vc + 0.5 one ulp below height, fill %d" % fill, _point(ty=_below(H - 0.5), fill=fill), 0, 0, 1, {(1, H - 1): 1.0})
        # cz = 1.4e-45 (a denormal depth_scale): cx / cz overflows
        add("uc infinite, fill %d" % fill, _point(scale=1e-45, fill=fill), 0, 1, 0, {})
        add("uc -infinite, fill %d" % fill, _point(tx=-1.0, scale=1e-45, fill=fill), 0, 1, 0, {})
    # two measurements on one pixel: a depth camera with a huge focal length sees both along (almost) one ray
    far = dict(K_depth=(1e6, 1e6, 0.0, 0.0), T=np.eye(4), min_z=0.0, size=(W, H), K=(1.0, 1.0, 2.0, 1.0), scale=SCALE)
    for fill in (0, 1):
        add("nearer first, fill %d" % fill, dict(far, depth=np.array([[1000, 2000]], np.uint16), fill=fill), 0, 0, 2, {(2, 1): float(F(1000) * F(SCALE))})
        add("nearer last, fill %d" % fill, dict(far, depth=np.array([[2000, 1000]], np.uint16), fill=fill), 0, 0, 2, {(2, 1): float(F(1000) * F(SCALE))})
        add("equal depths, fill %d" % fill, dict(far, depth=np.array([[1500, 1500]], np.uint16), fill=fill), 0, 0, 2, {(2, 1): float(F(1500) * F(SCALE))})
    # a whole frame collapsing onto one pixel: fx = fy = 1e-3
    rng = np.random.default_rng(42)
    frame = rng.integers(1, 65536, (6, 7)).astype(np.uint16)
    for fill in (0, 1):
        c = dict(depth=frame, scale=SCALE, K_depth=(5.0, 5.0, 3.0, 2.5), T=np.eye(4), min_z=0.0, fill=fill, size=(W, H),
                 K=(1e-3, 1e-3, 3.0, 2.0))
        add("collapse, fill %d" % fill, c, 0, 0, 42, {(3, 2): float(F(frame.min()) * F(SCALE))})
    # a footprint at the 4.0 cap: z / cz = 10, uc = 10, vc = 7 in 20x15: 9 x 9 pixel centres
    cz = float(F(10) + F(-9))
    add("footprint at the cap", _point(tx=10.0, ty=7.0, d=10, tz=-9.0, fill=1, size=(20, 15)), 0, 0, 1,
        {(x, y): cz for x in range(6, 15) for y in range(3, 12)})
    # a footprint whose range holds no pixel centre: hx = 0.5 * (0.4 * 1) = 0.2 around uc = 1.5 -> the nearest pixel, 2
    add("footprint without a centre", _point(tx=1.5 / 0.4, ty=1.5 / 0.4, fill=1, K=(0.4, 0.4, 0.0, 0.0)), 0, 0, 1, {(2, 2): 1.0})
    # a footprint at the cap clipped by each border of 20x15 (and by a corner)
    for name, tx, ty, xs, ys in (("left", 1.0, 7.0, range(0, 6), range(3, 12)), ("right", 18.0, 7.0, range(14, 20), range(3, 12)),
                                 ("top", 10.0, 1.0, range(6, 15), range(0, 6)), ("bottom", 10.0, 13.0, range(6, 15), range(9, 15)),
                                 ("corner", -3.0, -2.0, range(0, 2), range(0, 3))):
        add("footprint clipped: " + name, _point(tx=tx, ty=ty, d=10, tz=-9.0, fill=1, size=(20, 15)), 0, 0, 1,
            {(x, y): cz for x in xs for y in ys})
    add("footprint beyond the corner", _point(tx=-5.0, ty=-2.0, d=10, tz=-9.0, fill=1, size=(20, 15)), 0, 1, 0, {})
    return out


CRAFTED = _crafted()


@pytest.mark.parametrize("name,case,counters,pixels", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_crafted_case_hits_its_case(name, case, counters, pixels):
    plane, st = _both(case)
    assert {k: st[k] for k in counters} == counters, st
    assert _pixels(plane) == pixels


def test_the_crafted_positions_are_what_their_names_say():
    W = 8
    assert F(1.5) + F(0.5) == F(2.0) and _below(-0.5) + F(0.5) < 0 and F(W - 0.5) + F(0.5) == F(W)
    assert np.floor(_below(W - 0.5) + F(0.5)) == F(W - 1)
    z = F(1) * F(1e-45)
    assert 0 < z < np.finfo(F).tiny                                         # a denormal cz
    with np.errstate(over="ignore"):
        assert np.isinf(F(1) / z)


# ---- the identity consequence ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("size,K", [((64, 32), (64.0, 64.0, 31.0, 15.0)), ((160, 120), None)], ids=["pow2", "synth"])
def test_identity_registration_reproduces_the_plain_depth_plane(synth, size, K, fill):
    w, h = size
    K = K or synth.intrinsics_for(w, h)
    rng = np.random.default_rng(43)
    depth = rng.integers(1, 65536, (h, w)).astype(np.uint16)
    depth[rng.uniform(size=(h, w)) < 0.2] = 0
    plane, st = register_ref(depth, SCALE, K, np.eye(4), 0.0, fill, size, K)
    _, Z = synth.raw_to_float(np.zeros((h, w), np.uint8), depth)
    assert same_planes(plane, Z)
    assert st["drawn"] == st["measurements"] == st["covered_pixels"] == int(np.count_nonzero(depth))


# ---- fidelity of the rule on the synthetic scene --------------------------------------------------------------------------------------

def _depth_K(dw):
    s = dw / 640.0
    return (F(575.8 * s), F(575.8 * s), F(314.5 * s), F(235.5 * s))


def _scene(synth, dsize, size, T_colour=None, frame_id=0):
    """raw depth rendered at the depth camera, which sits at T_colour * T_depth_to_colour, and the depth the colour camera sees"""
    T = synth.se3_exp(XI_DEPTH_TO_COLOUR)
    Tc = np.eye(4) if T_colour is None else T_colour
    I, Z = synth.render(dsize[0], dsize[1], Tc @ T, nan_fraction=0.0, hole=False, K=_depth_K(dsize[0]), frame_id=frame_id)
    _, raw = synth.to_raw(I, Z)
    _, truth = synth.render(size[0], size[1], Tc, nan_fraction=0.0, hole=False, frame_id=frame_id)
    return raw, T, truth


@pytest.mark.parametrize("size", [(160, 120), (320, 240)], ids=lambda s: "%dx%d" % s)
def test_registered_depth_is_the_depth_the_colour_camera_sees(synth, size):
    raw, T, truth = _scene(synth, size, size)
    K = synth.intrinsics_for(*size)
    plane, st = register_ref(raw, SCALE, _depth_K(size[0]), T, 0.0, 0, size, K)
    plane64, st64 = register_ref(raw, SCALE, _depth_K(size[0]), T, 0.0, 0, size, K, dtype=np.float64)
    covered = ~np.isnan(plane)
    median = float(np.median(np.abs(plane[covered].astype(np.float64) - truth[covered])))
    mismatches = int((covered != ~np.isnan(plane64)).sum())
    print("median |registered - rendered| = %.3g m over %d pixels; float32 / float64 coverage mismatches: %d" % (median, covered.sum(), mismatches))
    assert covered.sum() > 0.5 * size[0] * size[1]
    assert median <= 2e-4                                                   # one step of the 1/5000 m quantisation
    assert mismatches == 0 and st == st64


def test_the_footprint_fills_a_half_resolution_depth_frame(synth):
    size, dsize = (160, 120), (80, 60)
    raw, T, _ = _scene(synth, dsize, size)
    K = synth.intrinsics_for(*size)
    share = [register_ref(raw, SCALE, _depth_K(dsize[0]), T, 0.0, fill, size, K)[1]["covered_pixels"] / (size[0] * size[1]) for fill in (0, 1)]
    print("covered share of the image: fill 0 %.3f, fill 1 %.3f" % tuple(share))
    assert share[1] >= 3 * share[0] > 0


# ---- CPU: the library's argument checks -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


def _invalid(capi, rc, *words):
    assert rc == INVALID, rc
    text = capi.lib().dvo_amd_last_error().decode()
    assert all(w in text for w in words), text


def _creg(capi, depth_size=(5, 3), K_depth=(4.0, 4.0, 2.5, 1.5), T=None, min_z=0.0, fill=0):
    return capi.Registration(depth_size=depth_size, K_depth=K_depth, T=np.eye(4) if T is None else T, min_z=min_z, fill=fill)._c()


def test_argument_checks(capi):
    L = capi.lib()
    img, z = np.zeros((4, 8, 3), np.uint8), np.ones((3, 6), np.uint16)
    h = C.c_void_p()
    st = capi.CRegistrationStats()
    ok = dict(device=0, image=img.ctypes.data, channels=3, istride=24, depth=z.ctypes.data, zstride=6, scale=SCALE, reg={}, width=8,
              height=4, K=(8.0, 8.0, 4.0, 2.0), levels=1, out=C.byref(h))

    def call(**kw):
        a = dict(ok, **kw)
        reg = None if a["reg"] is None else C.byref(_creg(capi, **a["reg"]))
        return L.dvo_amd_pyramid_create_raw_registered(a["device"], a["image"], a["channels"], a["istride"], a["depth"], a["zstride"],
                                                       a["scale"], 0, reg, None, a["width"], a["height"], *a["K"], a["levels"], 0.0,
                                                       a["out"], C.byref(st))

    for name in ("reg", "image", "depth", "out"):
        _invalid(capi, call(**{name: None}), "dvo_amd_pyramid_create_raw_registered", "NULL")
    for size in ((0, 3), (5, 0), (-1, 3), ((1 << 20) + 1, 3), (5, (1 << 20) + 1)):
        _invalid(capi, call(reg=dict(depth_size=size), zstride=1 << 21), "depth frame")
    _invalid(capi, call(zstride=4), "depth_stride")
    for bad in (np.nan, np.inf, -np.inf):
        for at in range(4):
            k = [4.0, 4.0, 2.5, 1.5]
            k[at] = bad
            _invalid(capi, call(reg=dict(K_depth=k)), "non-finite")
            k = [8.0, 8.0, 4.0, 2.0]
            k[at] = bad
            _invalid(capi, call(K=k), "non-finite")
        for r in range(3):
            for c in range(4):
                T = np.eye(4)
                T[r, c] = bad
                _invalid(capi, call(reg=dict(T=T)), "non-finite")
    T = np.eye(4)
    T[3, :] = np.nan                                                        # the last row is not read
    assert call(reg=dict(T=T)) in (0, NO_DEVICE)
    if h.value:
        L.dvo_amd_pyramid_release(h)
    for at in (0, 1):
        for bad in (0.0, -4.0):
            k = [4.0, 4.0, 2.5, 1.5]
            k[at] = bad
            _invalid(capi, call(reg=dict(K_depth=k)), "positive")
            k = [8.0, 8.0, 4.0, 2.0]
            k[at] = bad
            _invalid(capi, call(K=k), "positive")
    for bad in (-1e-3, np.nan, np.inf, -np.inf):
        _invalid(capi, call(reg=dict(min_z=bad)), "min_z")
    reg = _creg(capi)
    for bad in (2, -1):
        reg.fill = bad
        _invalid(capi, L.dvo_amd_pyramid_create_raw_registered(0, ok["image"], 3, 24, ok["depth"], 6, SCALE, 0, C.byref(reg), None, 8, 4, 8.0,
                                                               8.0, 4.0, 2.0, 1, 0.0, C.byref(h), None), "fill")
    _invalid(capi, call(istride=23), "stride")
    _invalid(capi, call(channels=1, istride=7), "stride")
    # everything dvo_amd_pyramid_create_raw rejects
    _invalid(capi, call(channels=2), "channels")
    _invalid(capi, call(scale=0.0), "depth_scale")
    _invalid(capi, call(scale=float("nan")), "depth_scale")
    _invalid(capi, call(levels=0), "levels")
    _invalid(capi, call(levels=9), "levels")
    _invalid(capi, call(levels=3), "level 2")                               # 8x4 holds two levels: the third would be 2x1
    _invalid(capi, call(width=6, istride=18), "level 0")
    _invalid(capi, call(width=0), "level 0")
    _invalid(capi, call(height=1), "level 0")
    assert not h.value
    assert [getattr(st, n) for n in COUNTERS] == [0] * 5


def test_a_level_too_small_is_named(capi):
    # 16x8 holds two levels (8x4), the third would be 4x2: legal; the fourth 2x1 is not
    L = capi.lib()
    img, z = np.zeros((8, 16), np.uint8), np.ones((1, 1), np.uint16)
    h = C.c_void_p()
    reg = _creg(capi, depth_size=(1, 1))
    rc = L.dvo_amd_pyramid_create_raw_registered(0, img.ctypes.data, 1, 16, z.ctypes.data, 1, SCALE, 0, C.byref(reg), None, 16, 8, 8.0, 8.0,
                                                 4.0, 2.0, 4, 0.0, C.byref(h), None)
    _invalid(capi, rc, "level 3")


def test_default_registration(capi):
    reg = capi.CRegistration()
    C.memset(C.byref(reg), 0xFF, C.sizeof(reg))
    capi.lib().dvo_amd_default_registration(C.byref(reg))
    assert (reg.depth_width, reg.depth_height, list(reg.k_depth), reg.min_z, reg.fill) == (0, 0, [0.0] * 4, 0.0, 0)
    assert np.array_equal(np.array(reg.T[:]).reshape(4, 4), np.eye(4))
    capi.lib().dvo_amd_default_registration(None)


def test_the_entry_fails_loudly_without_a_gpu(capi):
    if capi.lib().dvo_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    reg = capi.Registration(K_depth=(4.0, 4.0, 2.5, 1.5), T=np.eye(4))
    with pytest.raises(capi.DvoAmdError) as e:
        capi.RgbdImagePyramid.from_raw(np.zeros((4, 8), np.uint8), np.ones((3, 5), np.uint16), (8, 8, 4, 2), 1, registration=reg)
    assert e.value.status == NO_DEVICE


def test_header_and_binding_name_the_new_entries(capi):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dvo_amd.h")).read()
    for n in ("dvo_amd_default_registration", "dvo_amd_pyramid_create_raw_registered"):
        assert n + "(" in header and n in capi.EXPORTS and hasattr(capi.lib(), n), n
    assert capi.lib().dvo_amd_abi_version() == 3                            # purely additive


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

SHAPES = [((1, 1), (4, 2), 1), ((5, 3), (4, 2), 1), ((65, 3), (64, 32), 3), ((257, 2), (72, 50), 2), ((80, 60), (160, 120), 3)]
KINDS = ["host", "host_strided", "device", "device_offset_strided"]
REMAP_SRC = (80, 60)


def _gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")


def _image(rng, w, h, channels):
    return rng.integers(0, 256, (h, w) if channels == 1 else (h, w, 3)).astype(np.uint8)


def _random_maps(rng, w, h, sw, sh):
    """source positions of which about a fifth lies outside the source"""
    mx = rng.uniform(-0.1 * sw, 1.1 * sw, (h, w)).astype(F)
    my = rng.uniform(-0.1 * sh, 1.1 * sh, (h, w)).astype(F)
    return mx, my


def _overwrite_first_pixels(depth):
    """the depth values that take the rule's other paths, over the first pixels of a random frame (as many as it holds): no
    measurement, the smallest and the largest raw value, two equal neighbours"""
    flat = depth.reshape(-1)
    crafted = [0, 1, 65535, 3000, 3000, 0]
    n = min(len(crafted), flat.size - 1) if flat.size > 1 else 0
    flat[:n] = crafted[:n]
    return depth


@pytest.fixture(scope="module")
def cases(synth):
    """per shape and fill mode: the depth frame, the registration and the restatement's plane and counters; per output size and
    channel count an image -- computed once, never written to"""
    rng = np.random.default_rng(44)
    out = {}
    for dsize, size, levels in SHAPES:
        for fill in (0, 1):
            for _ in range(50):
                case, plane, st = _random_case(rng, dsize, size, fill, synth)
                _overwrite_first_pixels(case["depth"])
                plane, st = _ref(case)
                if st["measurements"] < 5 or (st["drawn"] and st["outside"]):
                    break
            for a in (case["depth"], plane):
                a.setflags(write=False)
            out[dsize, fill] = dict(case, levels=levels, Z=plane, stats=st)
        for channels in (1, 3):
            image = _image(rng, size[0], size[1], channels)
            image.setflags(write=False)
            out["image", size, channels] = image
    return out


def _all_planes_equal(p, q, levels, what):
    assert p.levels() == q.levels() == levels
    for level in range(levels):
        assert p.level_info(level)[:2] == q.level_info(level)[:2] and np.array_equal(p.level_info(level)[2], q.level_info(level)[2])
        for plane in range(6):
            assert same_planes(p.plane(level, plane), q.plane(level, plane)), (what, level, plane)


def _registration(capi, c):
    return capi.Registration(K_depth=c["K_depth"], T=c["T"], min_z=c["min_z"], fill=bool(c["fill"]))


def _ingest(capi, c, image, kind, levels, remap=None):
    """the registered pyramid of case c with `image`, the raw frame handed over in one of the four ways"""
    depth = c["depth"]
    dh, dw = depth.shape
    ih, iw = image.shape[:2]
    channels = 1 if image.ndim == 2 else 3
    row = iw * channels
    reg = _registration(capi, c)
    if kind == "host":
        return capi.RgbdImagePyramid.from_raw(image, depth, c["K"], levels, depth_scale=c["scale"], remap=remap, registration=reg)
    istride, zstride = row + 5, dw + 3                                      # rows that break the 4- and 8-byte alignment
    wide_i = np.full((ih, istride), 0xAB, np.uint8)
    wide_i[:, :row] = image.reshape(ih, row)
    wide_z = np.full((dh, zstride), 0x1234, np.uint16)
    wide_z[:, :dw] = depth
    if kind == "host_strided":
        return capi.RgbdImagePyramid._raw(wide_i.ctypes.data, channels, istride, wide_z.ctypes.data, zstride, c["scale"], 0, iw, ih, c["K"],
                                          levels, 0, 0.0, remap, reg, (dw, dh))
    import torch

    if kind == "device":
        d_i, d_z = torch.from_numpy(image.copy()).cuda(), torch.from_numpy(depth.view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        return capi.RgbdImagePyramid.from_raw_device(d_i.data_ptr(), channels, d_z.data_ptr(), iw, ih, c["K"], levels,
                                                     depth_scale=c["scale"], remap=remap, registration=reg, depth_size=(dw, dh))
    # the wide rows, the image's base pointer one byte and the depth's one element past an aligned address
    buf_i = torch.zeros(wide_i.size + 1, dtype=torch.uint8, device="cuda")
    buf_i[1:] = torch.from_numpy(wide_i.reshape(-1)).cuda()
    buf_z = torch.zeros(wide_z.size + 1, dtype=torch.int16, device="cuda")
    buf_z[1:] = torch.from_numpy(wide_z.view(np.int16).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return capi.RgbdImagePyramid.from_raw_device(buf_i.data_ptr() + 1, channels, buf_z.data_ptr() + 2, iw, ih, c["K"], levels,
                                                 depth_scale=c["scale"], image_stride_bytes=istride, depth_stride=zstride, remap=remap,
                                                 registration=reg, depth_size=(dw, dh))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("shape", [s[0] for s in SHAPES], ids=lambda s: "%dx%d" % s)
def test_registered_pyramid_equals_the_host_constructor_on_the_restatement(capi, cases, shape, fill, channels, kind):
    _gpu(capi)
    if kind.startswith("device"):
        pytest.importorskip("torch")
    c = cases[shape, fill]
    image = cases["image", c["size"], channels]
    p = _ingest(capi, c, image, kind, c["levels"])
    assert p.registration_stats == c["stats"]
    assert same_plane(p.plane(0, 1), c["Z"])                                # the empty pixels' NaN pattern included
    I = grey_plane(image).astype(F)
    q = capi.RgbdImagePyramid(I, c["Z"], c["K"], c["levels"])
    _all_planes_equal(p, q, c["levels"], (shape, fill, channels, kind))
    plain = capi.RgbdImagePyramid.from_raw(image, np.zeros(image.shape[:2], np.uint16), c["K"], 1, depth_scale=SCALE)
    assert same_planes(p.plane(0, 0), plain.plane(0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("fill", [0, 1])
def test_registered_pyramid_through_a_remap(capi, cases, fill, channels, kind):
    _gpu(capi)
    if kind.startswith("device"):
        pytest.importorskip("torch")
    c = dict(cases[(65, 3), fill])                                          # depth 65x3 ...
    size, levels = (72, 50), 2                                              # ... into 72x50 <- an 80x60 image
    c["size"], c["K"] = size, _colour_K(*size)
    Z, st = _ref(c)
    assert st["drawn"] > 0
    rng = np.random.default_rng(45 + channels)
    mx, my = _random_maps(rng, size[0], size[1], *REMAP_SRC)
    image = _image(rng, REMAP_SRC[0], REMAP_SRC[1], channels)
    I, _ = remap_ref(image, np.zeros(REMAP_SRC[::-1], np.uint16), mx, my, SCALE)
    remap = capi.Remap.from_maps(mx, my, REMAP_SRC)
    p = _ingest(capi, c, image, kind, levels, remap=remap)
    assert p.registration_stats == st
    q = capi.RgbdImagePyramid(I, Z, c["K"], levels)
    _all_planes_equal(p, q, levels, (fill, channels, kind))
    assert same_plane(p.plane(0, 1), Z)
    r = capi.RgbdImagePyramid.from_raw(image, np.zeros(REMAP_SRC[::-1], np.uint16), c["K"], 1, depth_scale=SCALE, remap=remap)
    assert same_planes(p.plane(0, 0), r.plane(0, 0))


@pytest.mark.gpu
def test_crafted_cases_on_the_device(capi):
    _gpu(capi)
    for name, case, counters, pixels in CRAFTED:
        w, h = case["size"]
        if w % 4:
            continue
        Z, st = _ref(case)
        p = capi.RgbdImagePyramid.from_raw(np.zeros((h, w), np.uint8), case["depth"], case["K"], 1, depth_scale=case["scale"],
                                           registration=_registration(capi, case))
        assert p.registration_stats == st and {k: st[k] for k in counters} == counters, name
        assert same_plane(p.plane(0, 1), Z) and _pixels(p.plane(0, 1)) == pixels, name


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [0, 1])
def test_4096_atomics_on_one_word_and_the_two_occlusion_orders(capi, fill):
    _gpu(capi)
    rng = np.random.default_rng(46)
    frame = rng.integers(1, 65536, (64, 64)).astype(np.uint16)
    c = dict(depth=frame, scale=SCALE, K_depth=(50.0, 50.0, 31.5, 31.5), T=np.eye(4), min_z=0.0, fill=fill, size=(8, 4),
             K=(1e-3, 1e-3, 3.0, 2.0))
    Z, st = _ref(c)
    assert st["drawn"] == 4096 and st["covered_pixels"] == 1 and _pixels(Z) == {(3, 2): float(F(frame.min()) * F(SCALE))}
    p = capi.RgbdImagePyramid.from_raw(np.zeros((4, 8), np.uint8), frame, c["K"], 1, registration=_registration(capi, c))
    assert p.registration_stats == st and same_plane(p.plane(0, 1), Z)
    # a near surface in front of a far one, seen from the side: whichever the scan meets first, the nearer depth stays
    for order in ((1000, 2000), (2000, 1000)):
        row = np.repeat(np.array(order, np.uint16), 40)[None, :].repeat(3, 0).copy()
        c = dict(depth=row, scale=SCALE, K_depth=(1e6, 1e6, 0.0, 0.0), T=np.eye(4), min_z=0.0, fill=fill, size=(8, 4),
                 K=(1.0, 1.0, 2.0, 1.0))
        Z, st = _ref(c)
        assert st["drawn"] == 240 and _pixels(Z) == {(2, 1): float(F(1000) * F(SCALE))}
        p = capi.RgbdImagePyramid.from_raw(np.zeros((4, 8), np.uint8), row, c["K"], 1, registration=_registration(capi, c))
        assert p.registration_stats == st and same_plane(p.plane(0, 1), Z)


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("channels", [1, 3])
def test_identity_registration_reproduces_the_plain_raw_ingest(capi, synth, channels, fill):
    _gpu(capi)
    rng = np.random.default_rng(47)
    for (w, h), K, levels in (((64, 32), (64.0, 64.0, 31.0, 15.0), 3), ((160, 120), synth.intrinsics_for(160, 120), 3)):
        image = _image(rng, w, h, channels)
        depth = rng.integers(1, 65536, (h, w)).astype(np.uint16)
        depth[rng.uniform(size=(h, w)) < 0.2] = 0
        reg = capi.Registration(K_depth=K, T=np.eye(4), fill=bool(fill))
        p = capi.RgbdImagePyramid.from_raw(image, depth, K, levels, depth_scale=SCALE, registration=reg)
        q = capi.RgbdImagePyramid.from_raw(image, depth, K, levels, depth_scale=SCALE)
        _all_planes_equal(p, q, levels, (w, h))
        n = int(np.count_nonzero(depth))
        assert p.registration_stats == dict(measurements=n, behind=0, outside=0, drawn=n, covered_pixels=n)
        assert q.registration_stats is None


def _same_result(a, b):
    assert np.array_equal(a.Transformation, b.Transformation) and np.array_equal(a.Information, b.Information)
    assert a.LogLikelihood == b.LogLikelihood and a.isNaN() == b.isNaN() and len(a.Levels) == len(b.Levels)
    for la, lb in zip(a.Levels, b.Levels):
        assert (la["Id"], la["ValidPixels"], la["MaxValidPixels"], la["TerminationCriterion"], len(la["Iterations"])) == \
               (lb["Id"], lb["ValidPixels"], lb["MaxValidPixels"], lb["TerminationCriterion"], len(lb["Iterations"]))


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [0, 1])
def test_match_on_registered_frames_equals_match_on_the_restatement_planes(capi, synth, fill):
    _gpu(capi)
    w, h = 160, 120
    (gr, _), (gc, _), T_gt = synth.sensor_pair(w, h, xi_gt=synth.XI_GT_PAIR * 0.5)
    K, Kd = synth.intrinsics_for(w, h), _depth_K(w)
    T = synth.se3_exp(XI_DEPTH_TO_COLOUR)
    # the depth camera's own frames: the sensor's noise and holes, rendered at the offset camera
    zr = synth.sensor_frame(w, h, T, frame_id=0, K=Kd)[1]
    zc = synth.sensor_frame(w, h, T_gt @ T, frame_id=1, K=Kd)[1]
    reg = capi.Registration(K_depth=Kd, T=T, fill=bool(fill))
    planes = [register_ref(z, SCALE, Kd, T, 0.0, fill, (w, h), K) for z in (zr, zc)]
    trk = capi.DenseTracker(capi.Config(FirstLevel=2, LastLevel=0))
    ref, cur = [capi.RgbdImagePyramid.from_raw(g, z, K, 3, depth_scale=SCALE, registration=reg) for g, z in ((gr, zr), (gc, zc))]
    href, hcur = [capi.RgbdImagePyramid(g.astype(F), Z, K, 3) for g, (Z, _) in zip((gr, gc), planes)]
    assert [p.registration_stats for p in (ref, cur)] == [st for _, st in planes]
    a, b = trk.match(ref, cur), trk.match(href, hcur)
    assert not a.isNaN() and sum(len(l["Iterations"]) for l in a.Levels) >= 3
    _same_result(a, b)


@pytest.mark.gpu
def test_staging_small_larger_small_and_a_remap_of_another_device(capi, cases):
    _gpu(capi)
    order = [(5, 3), (80, 60), (1, 1), (257, 2), (5, 3)]                    # the depth frame's staging grows, then serves smaller ones
    for dsize in order:
        c = cases[dsize, 1]
        p = _ingest(capi, c, cases["image", c["size"], 3], "host", 1)
        assert p.registration_stats == c["stats"] and same_plane(p.plane(0, 1), c["Z"]), dsize
    from rectify_ref import identity_maps

    L = capi.lib()
    c = cases[(5, 3), 0]
    image = cases["image", (4, 2), 1]
    remap = capi.Remap.from_maps(*identity_maps(4, 2), (4, 2))
    reg = _registration(capi, c)._c((5, 3))
    h = C.c_void_p()

    def call(device, width=4):
        return L.dvo_amd_pyramid_create_raw_registered(device, image.ctypes.data, 1, 4, c["depth"].ctypes.data, 5, SCALE, 0, C.byref(reg),
                                                       remap._h, width, 2, *[float(k) for k in c["K"]], 1, 0.0, C.byref(h), None)

    assert call(1) == MISMATCH and not h.value                              # a remap of device 0 asked to serve device 1
    _invalid(capi, call(0, width=8), "remap")                               # a remap whose output is not width x height
    assert call(0) == 0 and h.value
    L.dvo_amd_pyramid_release(h)
