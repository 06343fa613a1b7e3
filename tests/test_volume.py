"""The signed-distance volume on the device (include/dvo_amd.h, "A truncated signed-distance volume"): dvo_amd_volume_*.  The rules
are pinned in the header and restated twice in tests/volume_ref.py.  Every comparison with the library is equality -- records and
counts as integers, float planes and points on their bit patterns.  The only inequalities are the use (orderings of errors).
CPU: exports and layout, the argument checks that need no device, the two restatements against each other on crafted cases that
assert they hit their case, the contract on the restatement, the frustum box (also as a stand-alone program under UBSan), the
use.  GPU: the library against the restatement."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volume_ref as ref  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_volume_options", "dvo_amd_default_volume_raycast_options", "dvo_amd_volume_create", "dvo_amd_volume_destroy",
               "dvo_amd_volume_clear", "dvo_amd_volume_options_get", "dvo_amd_volume_integrate", "dvo_amd_volume_insert",
               "dvo_amd_volume_set_poses", "dvo_amd_volume_remove", "dvo_amd_volume_stats", "dvo_amd_volume_download",
               "dvo_amd_volume_raycast", "dvo_amd_volume_raycast_pyramid", "dvo_amd_volume_extract", "dvo_amd_debug_volume_timing"]
INVALID, NO_DEVICE, CAPACITY = 1, 2, 7
W, H = 64, 48
ROOM = dict(nx=64, ny=52, nz=56, voxel=0.05, origin=(-1.7, -1.35, 0.4), trunc=0.15, near_z=0.4, far_z=5.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(a, b):
    return a.dtype == b.dtype == F and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_view(a, b):
    return (same_bits(a["depth"], b["depth"]) and same_bits(a["intensity"], b["intensity"]) and a["weight"].dtype == b["weight"].dtype
            and np.array_equal(a["weight"], b["weight"]) and a["stats"] == b["stats"])


def up(v):
    return np.nextafter(F(v), F(np.inf))


def down(v):
    return np.nextafter(F(v), F(-np.inf))


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


@pytest.fixture(autouse=True)
def the_feature(capi):
    """every test of this file is about dvo_amd_volume: none of them passes against a library without it"""
    assert all(name in capi.EXPORTS and hasattr(capi.lib(), name) for name in NEW_SYMBOLS)


@functools.lru_cache(maxsize=None)
def stream():
    """eight 64x48 sensor frames along the stream: (frames as (Z, I, K, pose), K, poses)"""
    from dvo_slam_amd import synth

    K = tuple(float(k) for k in synth.intrinsics_for(W, H))
    poses = [synth.se3_exp(4 * synth.XI_STEP_STREAM * t) for t in range(8)]
    frames = []
    for t, T in enumerate(poses):
        grey, raw_z = synth.sensor_frame(W, H, T, frame_id=t)
        I, Z = synth.raw_to_float(grey, raw_z)
        frames.append((Z, I, K, T))
    return frames, K, poses


def rot_y(deg):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[0, 0], T[0, 2], T[2, 0], T[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    return T


# ---- CPU: exports, layout, argument checks ----------------------------------------------------------------------------------------

def test_exports_and_layout(capi):
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in capi.EXPORTS
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    assert all(re.search(r"\b%s\s*\(" % name, header) for name in NEW_SYMBOLS if "debug" not in name)
    assert L.dvo_amd_abi_version() == 3
    assert C.sizeof(capi.VolumeOptions) == 44 and capi.VolumeOptions.origin.offset == 16 and capi.VolumeOptions.weight.offset == 40
    assert C.sizeof(capi.VolumeRaycastOptions) == 12 and capi.VOLUME_VOXEL_DTYPE.itemsize == 16
    assert C.sizeof(capi.CVolumeRaycastStats) == 40 and capi.VOLUME_COUNTS_DTYPE.itemsize == 24
    o = capi.volume_options()
    assert (o.nx, o.ny, o.nz, o.weight) == (64, 64, 64, capi.VOLUME_WEIGHT_SENSOR)
    assert (F(o.voxel), F(o.trunc), F(o.near_z), F(o.far_z)) == (F(0.05), F(0.15), F(0.4), F(5.0))
    assert [F(v) for v in o.origin] == [F(-1.6), F(-1.6), F(0.4)]
    r = capi.volume_raycast_options()
    assert (F(r.step_fraction), r.min_weight, F(r.fill_intensity)) == (F(0.5), 1, F(0.0))
    with pytest.raises(TypeError):
        capi.volume_options(colour=1)


def test_argument_errors_fire_before_a_device_is_looked_for(capi):
    L = capi.lib()
    nan, inf = float("nan"), float("inf")

    def create(**kw):
        h = C.c_void_p()
        rc = L.dvo_amd_volume_create(0, C.byref(capi.volume_options(**kw)), C.byref(h))
        err = L.dvo_amd_last_error().decode()
        if h:
            L.dvo_amd_volume_destroy(h)
        return rc, err

    bad = [dict(nx=1), dict(ny=2049), dict(nz=0), dict(nx=2048, ny=2048, nz=512), dict(voxel=0.0), dict(voxel=nan), dict(trunc=inf),
           dict(near_z=-1.0), dict(far_z=nan), dict(trunc=0.04), dict(far_z=0.4), dict(far_z=0.3), dict(origin=(0.0, nan, 0.0)),
           dict(origin=(inf, 0.0, 0.0)), dict(weight=2), dict(weight=-1)]
    for kw in bad:
        rc, err = create(**kw)
        assert rc == INVALID and err.startswith("dvo_amd_volume_create: "), (kw, rc, err)
    assert L.dvo_amd_volume_create(0, None, C.byref(C.c_void_p())) == INVALID
    if L.dvo_amd_device_count() == 0:
        assert create()[0] == NO_DEVICE
        assert create(nx=2, ny=2, nz=2)[0] == NO_DEVICE
    # the other entries: what they check before they look at the volume, and the volume itself
    view = capi.CView(8, 8, 10.0, 10.0, 4.0, 4.0, 0.4)
    st = capi.CVolumeRaycastStats()
    for kw in (dict(step_fraction=0.0), dict(step_fraction=1.5), dict(step_fraction=nan), dict(min_weight=0), dict(fill_intensity=inf)):
        assert L.dvo_amd_volume_raycast(None, None, C.byref(view), C.byref(capi.volume_raycast_options(**kw)), None, None, None, C.byref(st)) == INVALID
        assert L.dvo_amd_last_error().decode().startswith("dvo_amd_volume_raycast: ")
    for v in (capi.CView(0, 8, 10.0, 10.0, 4.0, 4.0, 0.4), capi.CView(8, 8, 0.0, 10.0, 4.0, 4.0, 0.4), capi.CView(8, 8, 10.0, 10.0, nan, 4.0, 0.4),
              capi.CView(8, 8, 10.0, 10.0, 4.0, 4.0, 0.0)):
        assert L.dvo_amd_volume_raycast(None, None, C.byref(v), C.byref(capi.volume_raycast_options()), None, None, None, None) == INVALID
    pose = (C.c_double * 16)(*([nan] + [0.0] * 15))
    assert L.dvo_amd_volume_raycast(None, pose, C.byref(view), C.byref(capi.volume_raycast_options()), None, None, None, None) == INVALID
    assert "non-finite" in L.dvo_amd_last_error().decode()
    assert L.dvo_amd_volume_raycast(None, None, C.byref(view), C.byref(capi.volume_raycast_options()), None, None, None, None) == INVALID
    out = C.c_void_p()
    assert L.dvo_amd_volume_raycast_pyramid(None, None, C.byref(view), C.byref(capi.volume_raycast_options()), 1, 0.0, C.byref(out), None) == INVALID
    assert not out
    assert L.dvo_amd_volume_integrate(None, 0, None, 0, None, 1, None) == INVALID
    assert L.dvo_amd_volume_integrate(None, -1, None, 0, None, 1, None) == INVALID
    assert L.dvo_amd_last_error().decode() == "dvo_amd_volume_integrate: a negative count"
    assert L.dvo_amd_volume_insert(None, 0, None, None, 0, None, None) == INVALID
    assert L.dvo_amd_volume_set_poses(None, 0, None, None) == INVALID and L.dvo_amd_volume_remove(None, 0, None) == INVALID
    assert L.dvo_amd_volume_stats(None, None, None) == INVALID and L.dvo_amd_volume_clear(None) == INVALID
    n = C.c_longlong(5)
    assert L.dvo_amd_volume_download(None, None, None, 0, C.byref(n)) == INVALID and n.value == 0
    assert L.dvo_amd_volume_extract(None, 1, None, 0, C.byref(n), None) == INVALID
    assert L.dvo_amd_volume_options_get(None, None) == INVALID
    assert L.dvo_amd_debug_volume_timing(-1, 0, None, None, None) == INVALID
    assert L.dvo_amd_debug_volume_timing(0, 0, None, None, None) == 0
    if L.dvo_amd_device_count() == 0:
        assert L.dvo_amd_debug_volume_timing(0, 1, None, None, None) == NO_DEVICE


# ---- CPU: crafted cases, each asserting that it hits its case ---------------------------------------------------------------------

def one_voxel_case(Zs=1.0, Is=100.0, oz=1.0, ox=0.5, w=2, weight=ref.CONSTANT, trunc=0.25, near_z=0.5, far_z=4.0, pose=None, fx=2.0):
    """a 2x2x2 volume whose voxel (0,0,0) sits on the optical axis at depth oz, and a w x 2 frame of constant depth and grey value:
    (options, frame)"""
    opt = ref.Options(2, 2, 2, 0.25, (0.0, 0.0, oz), trunc, near_z, far_z, weight)
    return opt, (np.full((2, w), Zs, F), np.full((2, w), Is, F), (fx, 2.0, ox, 0.5), pose)


def one_voxel(**case):
    """(classes of the one frame, records) of a one-voxel case, after checking both restatements against each other"""
    opt, frame = one_voxel_case(**case)
    ra, rb = ref.empty(opt), ref.empty(opt)
    ca = ref.integrate(opt, ra, [frame])
    cb, classes = ref.integrate_scalar(opt, rb, [frame])
    assert np.array_equal(ra, rb) and np.array_equal(ca, cb)
    assert np.array_equal(classes[0], ref.classify(opt, frame)[0])
    assert ca[0, 0] == ca[0, 1] + ca[0, 2] == np.isin(classes[0], (ref.NEAR, ref.FREE)).sum()
    return classes[0], ref.public(ra)


def _far_pose():
    T = np.eye(4)
    T[0, 3] = -1e30
    return T


# The crafted integration cases: (parameters of one_voxel_case, class of voxel (0,0,0), its record or None).  The frustum-box tests
# below run the same list (box_cases): these are the places where a cull could drop a voxel that the rule keeps.
ONE_VOXEL_CASES = [
    # the near plane: a voxel exactly on near_z is taken, one ulp below it is behind
    (dict(oz=0.5, Zs=0.5), ref.NEAR, None),
    (dict(oz=down(0.5), Zs=0.5), ref.BEHIND, None),
    # d exactly -trunc is still seen (q = -2047), one ulp farther is hidden; d exactly +trunc is near (q = 2047), one ulp more free
    (dict(Zs=0.75), ref.NEAR, (1, -2047, 1, 1600)),
    (dict(Zs=down(0.75)), ref.HIDDEN, (0, 0, 0, 0)),
    (dict(Zs=1.25), ref.NEAR, (1, 2047, 1, 1600)),
    (dict(Zs=up(1.25)), ref.FREE, (1, 2047, 0, 0)),
    # the image border: px = -0.5 rounds to column 0, one ulp left of it and px = w - 0.5 (w = 2) are outside
    (dict(ox=-0.5), ref.NEAR, None),
    (dict(ox=down(-0.5)), ref.OUTSIDE, None),
    (dict(ox=1.5), ref.OUTSIDE, None),
    (dict(ox=down(1.5)), ref.NEAR, None),
    # Zs on far_z is used, one ulp beyond it is not; NaN depth and a non-finite grey value are no sample
    (dict(Zs=4.0), ref.FREE, None),
    (dict(Zs=up(4.0)), ref.NO_SAMPLE, None),
    (dict(Zs=np.nan), ref.NO_SAMPLE, None),
    (dict(Is=np.inf), ref.NO_SAMPLE, None),
    (dict(Is=np.nan), ref.NO_SAMPLE, None),
    # the sensor weight at both clamps: 256 at 0.4 m, 1 far away; the grey value at both clamps
    (dict(Zs=0.4, oz=0.4, near_z=0.25, weight=ref.SENSOR), ref.NEAR, (256, 0, 256, 256 * 1600)),
    (dict(Zs=7.9, oz=7.9, far_z=8.0, weight=ref.SENSOR), ref.NEAR, (1, 0, 1, 1600)),
    (dict(Is=300.0), ref.NEAR, (1, 0, 1, 4080)),
    (dict(Is=-5.0), ref.NEAR, (1, 0, 1, 0)),
    # a projection of 1e30 (and one that overflows) is outside, quietly
    (dict(pose=_far_pose()), ref.OUTSIDE, None),
    (dict(pose=_far_pose(), fx=1e30), ref.OUTSIDE, None),
]


def test_crafted_integration_cases_hit_their_case():
    reached = set()
    for case, want_cls, want_rec in ONE_VOXEL_CASES:
        cls, rec = one_voxel(**case)
        assert cls[0, 0, 0] == want_cls, case
        if want_rec is not None:
            assert tuple(rec[0, 0, 0]) == want_rec, case
        if "pose" in case:
            assert (cls == ref.OUTSIDE).all()
        reached.add(int(want_cls))
    assert reached == {ref.BEHIND, ref.OUTSIDE, ref.NO_SAMPLE, ref.HIDDEN, ref.NEAR, ref.FREE}
    assert one_voxel(oz=down(0.5), Zs=0.5)[0][1, 0, 0] != ref.BEHIND  # (only the voxel below near_z is behind)


def slab_volume(values, weights=None, grey=None, n=6):
    """records of an n x n x len(values) volume whose signed distance depends on z alone: F = values[iz] (in q / 2047 units of a
    weight-1 observation); weights[iz] = 0 leaves the slab unobserved"""
    opt = ref.Options(n, n, len(values), 0.25, (-0.5, -0.5, 1.0), 0.25, 0.5, 4.0, ref.CONSTANT)
    rec = ref.empty(opt)
    for iz, v in enumerate(values):
        w = 1 if weights is None else weights[iz]
        g = 1600 if grey is None else grey[iz]
        rec[iz, :, :, 0] = w
        rec[iz, :, :, 1] = np.int64(v * w) & 0xFFFFFFFF
        rec[iz, :, :, 2] = w if g is not None else 0
        rec[iz, :, :, 3] = (g or 0) * w
    return opt, rec


def both_raycasts(opt, rec, pose=None, K=(8.0, 8.0, 2.0, 2.0), w=5, h=5, **kw):
    a, b = ref.raycast(opt, rec, pose, K, w, h, **kw), ref.raycast_scalar(opt, rec, pose, K, w, h, **kw)
    assert same_view(a, b)
    s = a["stats"]
    assert s["pixels"] == w * h == s["hit"] + s["backface"] + s["missed"] and s["uncoloured"] <= s["hit"]
    return a


def test_crafted_raycast_cases_hit_their_case():
    # a front face between z = 1.5 and 1.75 (slabs 2 and 3): every ray hits, at the depth the interpolation gives
    opt, rec = slab_volume([2047, 1000, 500, -500, -1000, -2047])
    r = both_raycasts(opt, rec, near=1.0)
    assert r["stats"]["hit"] == 25 and r["stats"]["uncoloured"] == 0
    assert np.all((r["depth"] > F(1.5)) & (r["depth"] < F(1.75))) and np.all(r["intensity"] == F(100.0)) and np.all(r["weight"] == 1)
    # a hit between the first two samples: the march starts just in front of the face
    r = both_raycasts(opt, rec, near=1.56, step_fraction=1.0)
    assert r["stats"]["hit"] == 25 and np.all(r["depth"] < F(1.56) + opt.trunc)
    # a backface: negative in front, positive behind
    opt_b, rec_b = slab_volume([-2047, -1000, -500, 500, 1000, 2047])
    r = both_raycasts(opt_b, rec_b, near=1.01)
    assert r["stats"]["backface"] == 25 and np.isnan(r["depth"]).all()
    # a ray that leaves what is known and re-enters: slab 2 is unobserved, so f_prev is forgotten and the sign change across the gap
    # is no hit; with the gap observed it is one
    opt_g, rec_g = slab_volume([2047, 1000, 500, -500, -1000, -2047], weights=[1, 1, 0, 1, 1, 1])
    r = both_raycasts(opt_g, rec_g, near=1.0, step_fraction=1.0)
    assert r["stats"]["missed"] == 25 and r["stats"]["hit"] == 0
    r = both_raycasts(opt, rec, near=1.0, step_fraction=1.0)
    assert r["stats"]["hit"] == 25
    # ... and a ray that re-enters and then crosses: the gap lies in front of the face
    opt_h, rec_h = slab_volume([2047, 2047, 2047, 1000, 500, -500, -1000, -2047], weights=[1, 1, 0, 1, 1, 1, 1, 1])
    r = both_raycasts(opt_h, rec_h, K=(16.0, 16.0, 2.0, 2.0), near=1.0)
    assert r["stats"]["hit"] == 25 and np.all(r["depth"] > F(2.0))
    # min_weight turns observed voxels into unknown ones; an uncoloured hit has a depth and no intensity
    assert both_raycasts(opt, rec, near=1.0, min_weight=2)["stats"]["missed"] == 25
    opt_u, rec_u = slab_volume([2047, 1000, 500, -500, -1000, -2047], grey=[1600, 1600, 1600, None, 1600, 1600])
    r = both_raycasts(opt_u, rec_u, near=1.0)
    assert r["stats"]["uncoloured"] == 25 and np.isfinite(r["depth"]).all() and np.isnan(r["intensity"]).all()
    r = both_raycasts(opt_u, rec_u, near=1.0, fill=7.0)
    assert np.isnan(r["depth"]).all() and np.all(r["intensity"] == F(7.0))
    # a view turned away, and a view from outside through a corner
    assert both_raycasts(opt, rec, pose=rot_y(180.0), near=1.0)["stats"]["missed"] == 25
    side = np.eye(4)
    side[0, 3] = 0.9
    r = both_raycasts(opt, rec, pose=side, near=1.0)
    assert 0 < r["stats"]["hit"] < 25


def test_crafted_extract_cases_hit_their_case():
    opt, rec = slab_volume([2047, 1000, 0, -1000], n=3)  # Fb == 0 between slabs 1 and 2: s = 1, the point is voxel b's centre
    a, b = ref.extract(opt, rec), ref.extract_scalar(opt, rec)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    xyz, rgb, cnt = a
    assert cnt == dict(points=9, uncoloured=0) and np.all(bits(xyz[:, 2]) == bits(F(1.5))) and np.all(rgb == 0x646464)
    opt, rec = slab_volume([-2047, 0, 1000, 2047], n=3)  # Fa <= 0 && Fb > 0: the zero slab crosses towards the positive one
    xyz, rgb, cnt = ref.extract(opt, rec)
    assert cnt["points"] == 9 and np.all(bits(xyz[:, 2]) == bits(F(1.25)))
    opt, rec = slab_volume([2047, 1000, -1000, -2047], n=3, grey=[1600, None, 1600, 1600], weights=[1, 1, 1, 0])
    a, b = ref.extract(opt, rec), ref.extract_scalar(opt, rec)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    assert a[2] == dict(points=9, uncoloured=9) and np.all(a[1] == 0)
    assert ref.extract(opt, rec, min_weight=2)[2]["points"] == 0


# ---- CPU: the two restatements on real frames, and the contract on the restatement -------------------------------------------------

SMALL = dict(nx=12, ny=10, nz=8, voxel=0.1, origin=(-0.5, -0.4, 2.55), trunc=0.2, near_z=0.4, far_z=5.0)


def test_restatements_agree_on_sensor_frames():
    frames, K, poses = stream()
    for weight in (ref.CONSTANT, ref.SENSOR):
        opt = ref.Options(weight=weight, **SMALL)
        ra, rb = ref.empty(opt), ref.empty(opt)
        ca = ref.integrate(opt, ra, frames[:2])
        cb, _ = ref.integrate_scalar(opt, rb, frames[:2])
        assert np.array_equal(ra, rb) and np.array_equal(ca, cb) and ca[:, 1].min() > 0 and ca[:, 2].min() > 0
        Ks = (K[0] / 4, K[1] / 4, K[2] / 4, K[3] / 4)
        va, vb = ref.raycast(opt, ra, poses[0], Ks, 16, 12, near=2.0), ref.raycast_scalar(opt, ra, poses[0], Ks, 16, 12, near=2.0)
        assert same_view(va, vb) and va["stats"]["hit"] > 0
        ea, eb = ref.extract(opt, ra), ref.extract_scalar(opt, ra)
        assert same_bits(ea[0], eb[0]) and np.array_equal(ea[1], eb[1]) and ea[2] == eb[2] and ea[2]["points"] > 0


def test_contract_on_the_restatement():
    frames, K, poses = stream()
    opt = ref.Options(weight=ref.SENSOR, **ROOM)
    three = frames[:3]
    rec = ref.empty(opt)
    ref.integrate(opt, rec, three, +1)
    assert rec.any()
    once = rec.copy()
    ref.integrate(opt, rec, three, -1)
    assert not rec.any()  # -1 after +1: all zeros
    for order in ([2, 0, 1], [1, 2, 0]):  # any order, any batching
        r = ref.empty(opt)
        for k in order:
            ref.integrate(opt, r, [three[k]])
        assert np.array_equal(r, once)
    r = ref.empty(opt)
    ref.integrate(opt, r, three[:1])
    ref.integrate(opt, r, three[1:])
    assert np.array_equal(r, once)
    # a move equals remove plus insert: frame 1 to another pose
    moved = (three[1][0], three[1][1], K, poses[5])
    a = once.copy()
    ref.integrate(opt, a, [three[1], moved], signs=[-1, +1])
    b = ref.empty(opt)
    ref.integrate(opt, b, [three[0], moved, three[2]])
    assert np.array_equal(a, b) and not np.array_equal(a, once)
    # sums are taken modulo 2^32: a wrapped record still subtracts exactly
    w = ref.empty(opt)
    w[..., 1] = 0x7FFFFFF0
    before = w.copy()
    ref.integrate(opt, w, three, +1)
    ref.integrate(opt, w, three, -1)
    assert np.array_equal(w, before)


# ---- CPU: the frustum box ---------------------------------------------------------------------------------------------------------

def box_cases():
    """(M float32 [3, 4], K, w, h, options): the stream's poses in the room, a thin volume, every crafted integration case
    (ONE_VOXEL_CASES) and 200 random poses"""
    frames, K, poses = stream()
    room = ref.Options(weight=ref.SENSOR, **ROOM)
    thin = ref.Options(70, 5, 3, 0.05, (-1.7, 0.0, 1.0), 0.15, 0.4, 5.0, ref.CONSTANT)
    cases = [(ref.inverse_rows(T), K, W, H, room) for T in poses] + [(ref.inverse_rows(None), (2.0, 2.0, 0.5, 0.5), 2, 2, thin)]
    for case, _, _ in ONE_VOXEL_CASES:  # every crafted integration case: its volume, its camera, its pose
        opt, (Z, _, Kc, pose) = one_voxel_case(**case)
        cases.append((ref.inverse_rows(pose), Kc, Z.shape[1], Z.shape[0], opt))
    rng = np.random.RandomState(7)
    from dvo_slam_amd import synth
    for i in range(200):
        xi = np.concatenate([rng.uniform(-3.0, 3.0, 3), rng.uniform(-np.pi, np.pi, 3)])
        if i % 4 == 1:
            xi[:3] *= 0.2                      # the camera inside the volume
        if i % 4 == 2:
            xi[2] = 8.0 + rng.uniform(0, 4)    # the volume wholly behind, or in front and far away
        cases.append((ref.inverse_rows(synth.se3_exp(xi)), K, W, H, room if i % 3 else thin))
    return cases


def updated_by_rule(M, K, w, h, opt):
    """the voxels the rule can update for ANY image of this size (classify() takes M through the patched inverse_rows)"""
    always = (np.full((h, w), opt.far_z, F), np.zeros((h, w), F), K, None)  # the farthest sample hides the fewest voxels
    cls = ref.classify(opt, always)[0]
    return (cls == ref.NEAR) | (cls == ref.FREE)


def test_no_voxel_the_rule_updates_lies_outside_the_box(monkeypatch):
    for case, _, _ in ONE_VOXEL_CASES:  # the crafted cases with their own frames: what the rule updates there is inside the box
        opt, frame = one_voxel_case(**case)
        cls = ref.classify(opt, frame)[0]
        box = ref.frustum_box(ref.inverse_rows(frame[3]), frame[2], frame[0].shape[1], frame[0].shape[0], opt)
        assert not (((cls == ref.NEAR) | (cls == ref.FREE)) & ~ref.in_box(box, cls.shape)).any(), case
    n_empty = n_partial = 0
    for M, K, w, h, opt in box_cases():
        monkeypatch.setattr(ref, "inverse_rows", lambda pose, M=M: M)
        reach = updated_by_rule(M, K, w, h, opt)
        box = ref.frustum_box(M, K, w, h, opt)
        inside = ref.in_box(box, reach.shape)
        assert not (reach & ~inside).any()
        n_empty += not inside.any()
        n_partial += inside.any() and not inside.all()
        assert inside.any() or not reach.any()
    assert n_empty > 10 and n_partial > 10  # the box does cull


def box_line(M, K, w, h, opt, z_max=None):
    vals = [float(v) for v in np.asarray(M, np.float64).reshape(12)] + [float(F(k)) for k in K]
    tail = [float(opt.near_z), float(F(opt.far_z + opt.trunc)) if z_max is None else z_max] + [float(v) for v in opt.origin] + [float(opt.voxel)]
    fmt = lambda v: "nan" if v != v else ("inf" if v == float("inf") else ("-inf" if v == -float("inf") else float(v).hex()))  # noqa: E731
    return " ".join([fmt(v) for v in vals] + [str(w), str(h)] + [fmt(v) for v in tail] + [str(d) for d in opt.dims])


def test_the_box_code_is_clean_under_ubsan_and_equals_python(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++11", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
    if subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no UBSan runtime")
    exe = tmp_path / "volume_box"
    res = subprocess.run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "dvo_slam_amd", "csrc"),
                                          os.path.join(ROOT, "tests", "volume_box_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    cases = box_cases()
    room = cases[0][4]
    K = cases[0][1]
    eye = ref.inverse_rows(None).astype(np.float64)
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e300, 1e308):  # non-finite and huge input
        for at in ((0, 3), (2, 3), (1, 1), (2, 2)):
            M = eye.copy()
            M[at] = bad
            cases.append((M, K, W, H, room))
    cases.append((eye * 1e-3, K, W, H, room))                   # far from a rotation
    cases.append((eye, (1e-30, 1e30, 0.0, 0.0), W, H, room))
    cases.append((eye, (50.0, 50.0, 1e30, -1e30), W, H, room))
    huge = ref.Options(2048, 2048, 256, 1e-3, (1e6, -1e6, 0.0), 1.0, 0.4, 5.0, ref.CONSTANT)
    cases.append((eye, K, W, H, huge))
    lines = [box_line(*c) for c in cases]
    want = []
    for M, Kc, w, h, opt in cases:
        lo, hi = ref.frustum_box(np.asarray(M, np.float64), Kc, w, h, opt)
        want.append("%d %d %d %d %d %d" % (lo + hi))
    res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0 and "runtime error" not in res.stderr, res.stderr
    assert res.stdout.strip().splitlines() == want
    full = "0 0 0 63 51 55"
    assert want.count(full) >= 20 and "0 0 0 -1 -1 -1" in want


# ---- CPU: the use, as orderings ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def room_reference(n_frames):
    """the restatement's room after n frames in one call: (options, records, counts)"""
    frames, K, poses = stream()
    opt = ref.Options(weight=ref.SENSOR, **ROOM)
    rec = ref.empty(opt)
    counts = ref.integrate(opt, rec, frames[:n_frames])
    rec.setflags(write=False)
    return opt, rec, counts


def test_fusing_frames_denoises_the_model_view():
    from dvo_slam_amd import synth

    frames, K, poses = stream()
    _, Za = synth.render(W, H, poses[0], nan_fraction=0, hole=False)

    def view_rms(n):
        opt, rec, _ = room_reference(n)
        r = ref.raycast(opt, rec, poses[0], K, W, H)
        hit = np.isfinite(r["depth"])
        assert hit.sum() == r["stats"]["hit"]
        return float(np.sqrt(np.mean((r["depth"][hit].astype(np.float64) - Za[hit]) ** 2))), hit.mean(), r

    rms1, cov1, _ = view_rms(1)
    rms8, cov8, r8 = view_rms(8)
    Z0 = frames[0][0]
    valid = np.isfinite(Z0)
    raw = float(np.sqrt(np.mean((Z0[valid].astype(np.float64) - Za[valid]) ** 2)))
    print("rms 1 frame %.4f, 8 frames %.4f, raw %.4f; coverage %.3f / %.3f" % (rms1, rms8, raw, cov1, cov8))
    assert rms8 < rms1 and rms8 < raw
    assert cov8 >= 0.6
    assert r8["stats"]["uncoloured"] < r8["stats"]["hit"]
    opt, rec, _ = room_reference(8)
    xyz, rgb, cnt = ref.extract(opt, rec)
    far = np.minimum(np.minimum(np.abs(xyz[:, 1] - F(1.2)), np.abs(xyz[:, 2] - F(3.0))), np.abs(xyz[:, 0] + F(1.6)))
    assert cnt["points"] > 1000 and far.max() <= opt.trunc


# ---- GPU: the library against the restatement -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


class Resident:
    """the stream's pyramids on the device (uploaded once, two levels) and their level planes as the device holds them"""

    def __init__(self, capi):
        frames, K, poses = stream()
        self.capi, self.K, self.poses = capi, K, poses
        self.pyramids = [capi.RgbdImagePyramid(I, Z, K, 2) for Z, I, _, _ in frames]
        from dvo_slam_amd import synth
        self.K_other = (40.0, 38.0, 15.25, 12.5)
        grey, raw_z = synth.sensor_frame(32, 24, poses[3], frame_id=11, K=self.K_other)
        I, Z = synth.raw_to_float(grey, raw_z)
        self.other = capi.RgbdImagePyramid(I, Z, self.K_other, 1)
        self._planes = {}

    def frame(self, pyramid, level, pose):
        """the level as the restatement takes it"""
        key = (id(pyramid), level)
        if key not in self._planes:
            self._planes[key] = (pyramid.plane(level, 1), pyramid.plane(level, 0), tuple(pyramid.level_info(level)[2]))
        Z, I, K = self._planes[key]
        return Z, I, K, pose


@pytest.fixture(scope="module")
def resident(gpu):
    return Resident(gpu)


def records(vol, box=None):
    d = vol.download(box)
    return np.stack([d[n] for n in ("w_sum", "sd_sum", "iw_sum", "i_sum")], axis=-1)


def counts_of(c):
    return np.stack([c[n] for n in ("updated", "near", "free")], axis=-1)


@pytest.mark.gpu
def test_the_room_equals_the_restatement(gpu, resident):
    opt, rec, counts = room_reference(8)
    vol = gpu.SurfaceVolume(opt.fields())
    gpu.volume_timing(True)
    got = vol.integrate(resident.pyramids, resident.poses)
    t = gpu.volume_timing(True)
    assert (t["launches"], t["synchronisations"]) == (1, 1)  # eight frames, one launch
    frames = [resident.frame(p, 0, T) for p, T in zip(resident.pyramids, resident.poses)]
    assert all(np.array_equal(bits(f[0]), bits(g[0])) for f, g in zip(frames, stream()[0]))  # level 0 is the frame
    assert np.array_equal(counts_of(got), counts) and counts[:, 1].min() > 0 and counts[:, 2].min() > 0
    assert np.array_equal(records(vol), ref.public(rec))
    box = (3, 50, 7, 40, 51, 30)
    assert np.array_equal(records(vol, box), ref.public(rec)[7:31, 50:52, 3:41])
    assert np.array_equal(records(vol, (63, 51, 55, 63, 51, 55)), ref.public(rec)[55:, 51:, 63:])
    with pytest.raises(gpu.DvoAmdError) as e:
        vol.download((0, 0, 0, 64, 51, 55))
    assert e.value.status == INVALID
    n = C.c_longlong()
    assert gpu.lib().dvo_amd_volume_download(vol._h, None, None, 0, C.byref(n)) == CAPACITY and n.value == 64 * 52 * 56
    # the views
    K = resident.K
    for pose, Kv, w, h, kw in ((resident.poses[0], K, W, H, {}), (resident.poses[2], K, 1, 1, {}),
                               (resident.poses[5], (60.0, 55.0, 33.3, 2.2), 67, 5, dict(step_fraction=0.3)),
                               (resident.poses[0] @ rot_y(180.0), K, W, H, {}), (resident.poses[1], K, W, H, dict(min_weight=300, near=0.8))):
        want = ref.raycast(opt, rec, pose, Kv, w, h, **kw)
        near = kw.pop("near", None)
        got = vol.raycast(pose, Kv, w, h, near=near, options=kw)
        t = gpu.volume_timing(True)
        assert same_view(got, want), (w, h, kw, got["stats"], want["stats"])
        assert (t["launches"], t["synchronisations"]) == (1, 1)
    assert ref.raycast(opt, rec, resident.poses[0], K, W, H)["stats"]["hit"] > 2000
    assert vol.raycast(resident.poses[0] @ rot_y(180.0), K, W, H)["stats"]["missed"] == W * H
    only = vol.raycast(resident.poses[0], K, W, H, planes=("depth",))
    assert set(only) == {"depth", "stats"} and same_bits(only["depth"], ref.raycast(opt, rec, resident.poses[0], K, W, H)["depth"])
    # the surface
    xyz, rgb, cnt = ref.extract(opt, rec)
    gx, gr, gc = vol.extract()
    assert (gpu.volume_timing(True)["launches"], gpu.volume_timing(True)["synchronisations"]) == (3, 2)
    assert same_bits(gx, xyz) and np.array_equal(gr, rgb) and gc == cnt and cnt["points"] > 1000
    for mw in (2, 400):
        want = ref.extract(opt, rec, mw)
        got = vol.extract(mw)
        assert same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    with pytest.raises(gpu.DvoAmdError) as e:
        vol.extract(capacity=cnt["points"] - 1)
    assert e.value.status == CAPACITY and vol.last_extract_size == cnt["points"]
    assert vol.extract(capacity=cnt["points"])[2] == cnt
    # the model view as a pyramid: the planes of three levels equal the host constructor's on the downloaded level 0
    want = ref.raycast(opt, rec, resident.poses[0], K, W, H, fill=3.0)
    pyr = vol.raycast_pyramid(resident.poses[0], K, W, H, 3, options=dict(fill_intensity=3.0), timestamp=2.5)
    assert pyr.raycast_stats == want["stats"] and pyr.levels() == 3 and pyr.timestamp() == 2.5
    I0, Z0 = pyr.plane(0, 0), pyr.plane(0, 1)
    assert same_bits(I0, want["intensity"]) and same_bits(Z0, want["depth"])
    host = gpu.RgbdImagePyramid(I0, Z0, K, 3)
    for level in range(3):
        for plane in (0, 1):
            assert same_bits(pyr.plane(level, plane), host.plane(level, plane))
    # -1 undoes +1 exactly
    vol.integrate(resident.pyramids, resident.poses, sign=-1)
    assert not records(vol).any()


SHAPES = [dict(nx=70, ny=5, nz=3, voxel=0.05, origin=(-1.7, 0.9, 2.9), trunc=0.15, near_z=0.4, far_z=5.0),
          dict(nx=2, ny=2, nz=2, voxel=0.05, origin=(0.0, 0.0, 2.975), trunc=0.15, near_z=0.4, far_z=5.0),  # the wall z = 3 runs through its one cell
          dict(nx=12, ny=10, nz=8, voxel=0.1, origin=(-0.5, -0.4, 2.55), trunc=0.2, near_z=0.4, far_z=3.0)]


CELL_K = (400.0, 400.0, -2.3, -2.3)  # pixel (1,1) looks at (0.025, 0.025, 3): the middle of SHAPES[1]'s cell


@pytest.mark.gpu
@pytest.mark.parametrize("shape", range(len(SHAPES)))
@pytest.mark.parametrize("weight", [ref.CONSTANT, ref.SENSOR])
def test_shapes_levels_and_frames(gpu, resident, shape, weight):
    opt = ref.Options(weight=weight, **SHAPES[shape])
    away = resident.poses[1] @ rot_y(180.0)
    clip = np.array(resident.poses[2])
    clip[0, 3] += 2.6  # the frustum only clips the volume's far +x corner
    for level, items in ((0, [(resident.pyramids[0], resident.poses[0]), (resident.pyramids[4], resident.poses[4]), (resident.pyramids[1], away),
                              (resident.pyramids[2], clip)]),
                         (1, [(resident.pyramids[3], resident.poses[3]), (resident.pyramids[6], None)]),
                         (0, [(resident.other, resident.poses[3])])):
        vol = gpu.SurfaceVolume(opt.fields())
        pyramids, poses = [p for p, _ in items], [T for _, T in items]
        got = vol.integrate(pyramids, poses, level=level)
        frames = [resident.frame(p, level, T) for p, T in items]
        rec = ref.empty(opt)
        want = ref.integrate(opt, rec, frames)
        assert np.array_equal(counts_of(got), want), (level, counts_of(got), want)
        assert np.array_equal(records(vol), ref.public(rec))
        if level == 0 and len(items) == 4:
            assert want[2].tolist() == [0, 0, 0]  # the frame that looks away
            if shape == 0:
                assert 0 < want[3, 0] < want[0, 0]  # the clipped corner
        assert want[0, 0] > 0 or (shape == 0 and len(items) == 1)  # (the 32x24 frame does not see the thin volume)
        pose, K = resident.poses[0], tuple(k / 4 for k in resident.K)
        view = ref.raycast(opt, rec, pose, K, 16, 12, near=2.0)
        assert same_view(vol.raycast(pose, K, 16, 12, near=2.0), view)
        assert view["stats"]["hit"] > 0 or shape == 1 or len(items) != 4
        if shape == 1:  # a 3x3 view whose rays all pass through the volume's one cell, in steps of a tenth of trunc: the blend
            cell = dict(near=2.5, step_fraction=0.1)
            want_cell = ref.raycast(opt, rec, None, CELL_K, 3, 3, **cell)
            assert same_view(vol.raycast(None, CELL_K, 3, 3, near=2.5, options=dict(step_fraction=0.1)), want_cell)
            assert want_cell["stats"]["hit"] == 9 or len(items) != 4
        e, w = vol.extract(), ref.extract(opt, rec)
        assert same_bits(e[0], w[0]) and np.array_equal(e[1], w[1]) and e[2] == w[2]


@pytest.mark.gpu
def test_the_empty_volume(gpu, resident):
    opt = ref.Options(weight=ref.SENSOR, **SHAPES[0])
    vol = gpu.SurfaceVolume(opt.fields())
    rec = ref.empty(opt)
    assert not records(vol).any() and vol.stats() == dict(keyframes=0, updated_total=0)
    assert same_view(vol.raycast(None, resident.K, W, H), ref.raycast(opt, rec, None, resident.K, W, H))
    assert vol.raycast(None, resident.K, W, H)["stats"]["missed"] == W * H
    xyz, rgb, cnt = vol.extract()
    assert len(xyz) == 0 and len(rgb) == 0 and cnt == dict(points=0, uncoloured=0)
    assert len(vol.integrate([], [])) == 0 and len(vol.insert([], [], [])) == 0
    vol.set_poses([], [])
    vol.remove([])
    assert not records(vol).any()


@pytest.mark.gpu
def test_the_contract_on_the_device(gpu, resident):
    opt, rec8, counts8 = room_reference(8)
    ids = list(range(10, 18))
    pyr, poses = resident.pyramids, resident.poses

    def run(order, batches):
        """the keyframes inserted in `order`, split into `batches` calls: records after every stage of one history"""
        vol = gpu.SurfaceVolume(opt.fields())
        stages = []
        at = 0
        for size in batches:
            part = order[at:at + size]
            at += size
            got = vol.insert([ids[k] for k in part], [pyr[k] for k in part], [poses[k] for k in part])
            assert np.array_equal(counts_of(got), counts8[part])
            assert gpu.volume_timing(False)["launches"] == 1
        stages.append(records(vol))
        assert vol.stats() == dict(keyframes=8, updated_total=int(counts8[:, 0].sum()))
        # a move and a move back
        vol.set_poses([ids[1]], [poses[5]])
        assert (gpu.volume_timing(False)["launches"], gpu.volume_timing(False)["synchronisations"]) == (1, 1)
        stages.append(records(vol))
        vol.set_poses([ids[1]], [poses[1]])
        stages.append(records(vol))
        vol.set_poses([ids[1]], [poses[1]])  # the same floats: nothing to do, nothing launched
        assert gpu.volume_timing(False)["launches"] == 0
        # a set_poses that moves everything: every keyframe to its neighbour's pose
        vol.set_poses(ids, [poses[(k + 1) % 8] for k in range(8)])
        assert gpu.volume_timing(False)["launches"] == 1
        stages.append(records(vol))
        stats_moved = vol.stats()
        vol.remove(ids[:3])
        stages.append(records(vol))
        assert vol.stats()["keyframes"] == 5
        vol.remove(ids[3:])
        stages.append(records(vol))
        assert vol.stats() == dict(keyframes=0, updated_total=0)
        return stages, stats_moved

    a, stats_a = run(list(range(8)), [8])
    b, stats_b = run([5, 2, 7, 0, 3, 6, 1, 4], [1] * 8)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)  # two histories, the same bits at every stage
    assert stats_a == stats_b
    frames = [resident.frame(pyr[k], 0, poses[k]) for k in range(8)]
    assert np.array_equal(a[0], ref.public(rec8)) and np.array_equal(a[2], a[0])
    moved = ref.empty(opt)
    ref.integrate(opt, moved, [frames[k] if k != 1 else frames[1][:3] + (poses[5],) for k in range(8)])
    assert np.array_equal(a[1], ref.public(moved)) and not np.array_equal(a[1], a[0])
    shifted = ref.empty(opt)
    c = ref.integrate(opt, shifted, [frames[k][:3] + (poses[(k + 1) % 8],) for k in range(8)])
    assert np.array_equal(a[3], ref.public(shifted)) and stats_a["updated_total"] == int(c[:, 0].sum())
    rest = ref.empty(opt)
    ref.integrate(opt, rest, [frames[k][:3] + (poses[(k + 1) % 8],) for k in range(3, 8)])
    assert np.array_equal(a[4], ref.public(rest))
    assert not a[5].any()  # every keyframe removed: all zeros
    # the tracked form's argument errors leave the volume as it was
    vol = gpu.SurfaceVolume(opt.fields())
    vol.insert(ids[:2], pyr[:2], poses[:2])
    before = records(vol)
    bad_pose = np.array(poses[0])
    bad_pose[1, 2] = np.nan
    for call in (lambda: vol.insert([ids[0]], [pyr[3]], [poses[3]]), lambda: vol.insert([50, 50], pyr[:2], poses[:2]),
                 lambda: vol.set_poses([99], [poses[0]]), lambda: vol.remove([ids[0], ids[0]]), lambda: vol.remove([ids[5]]),
                 lambda: vol.set_poses([ids[0]], [bad_pose]), lambda: vol.insert([51], [pyr[3]], [poses[3]], level=2),
                 lambda: vol.integrate([pyr[3]], [bad_pose]), lambda: vol.integrate([pyr[3]], [poses[3]], sign=2)):
        with pytest.raises(gpu.DvoAmdError) as e:
            call()
        assert e.value.status == INVALID and "dvo_amd_volume_" in str(e.value)
    assert np.array_equal(records(vol), before) and vol.stats()["keyframes"] == 2
    vol.clear()
    assert not records(vol).any() and vol.stats()["keyframes"] == 0
