"""Loop-closure candidates: dvo_amd_covisibility and dvo_amd_find_constraint_candidates (include/dvo_amd.h).

The rule is pinned operation by operation in the header and restated in tests/covisibility_ref.py.  Every comparison in this
file is integer equality (or equality of doubles formed from integers); there is no tolerance anywhere.
CPU: the restatement against its independent pixel loop on random images and on crafted cases, each of which asserts that it
really hits its case; the radius stage and every argument check that needs no device, through the library with ctx = NULL.
GPU: the library against the restatement on the planes downloaded from the pyramids.

Sizes.  A pyramid level must be at least 4x2 with a width that is a multiple of 4 (dvo_amd_pyramid_create), so a 72x50 frame
holds two levels (3600 and 900 pixels; a request for level 2 or 3 is clamped to level 1, which the tests use), not three, and a
1x1 image cannot be a keyframe at all.  The level below four waves is therefore 80x48's level 2 (20x12 = 240 pixels; 3840 and
960 above it: none a multiple of the block's 1024-pixel chunk), the whole number of waves is 64x32 (2048 pixels, two whole
chunks; 512 and 128 below it), and the smallest image is the smallest pyramid there is, 4x2."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from covisibility_ref import COUNTS, candidates_ref, covis_brute, covis_ref, overlap, radius_ref  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTCOMES = COUNTS[1:]
BEHIND, OUTSIDE, NO_DEPTH, CONSISTENT, OCCLUDED, SEEN_THROUGH = range(1, 7)
INVALID, NO_DEVICE, CAPACITY, MISMATCH = 1, 2, 7, 8


def _both(pa, pb, Ta, Tb, opt=None, what=None):
    ref = covis_ref(pa, pb, Ta, Tb, opt, info=True)
    brute = covis_brute(pa, pb, Ta, Tb, opt)
    assert {k: ref[k] for k in COUNTS} == brute, (what, {k: ref[k] for k in COUNTS}, brute)
    assert ref["valid"] == sum(ref[k] for k in OUTCOMES) == int(np.isfinite(pa[0]).sum()), what
    return ref


def _image(rng, w, h, holes=0.15, zmin=0.5, zmax=4.0):
    Z = rng.uniform(zmin, zmax, (h, w)).astype(F)
    Z[rng.uniform(size=(h, w)) < holes] = np.nan
    return Z


def _K(rng, w, h):
    return (F(rng.uniform(0.7, 1.4) * w), F(rng.uniform(0.7, 1.4) * w), F(w / 2 + rng.uniform(-1, 1)), F(h / 2 + rng.uniform(-1, 1)))


# ---- CPU: the restatement against its pixel loop ------------------------------------------------------------------------------------

def test_restatement_matches_the_pixel_loop_on_random_images(synth):
    rng = np.random.default_rng(11)
    seen = dict.fromkeys(OUTCOMES, 0)
    sizes = [(8, 6), (9, 7), (13, 9), (16, 12), (20, 15)]
    for k in range(40):
        (wa, ha), (wb, hb) = sizes[k % 5], sizes[(k * 3 + k // 5) % 5]
        pa, pb = (_image(rng, wa, ha), _K(rng, wa, ha)), (_image(rng, wb, hb), _K(rng, wb, hb))
        scale = (0.02, 0.2, 1.0, 3.0)[k % 4]
        Ta, Tb = synth.se3_exp(rng.normal(size=6) * scale), synth.se3_exp(rng.normal(size=6) * scale)
        opt = dict(near_z=(0.1, 0.6, 1.0)[k % 3], depth_sigmas=(20.0, 1.0, 0.0, 100.0)[(k // 3) % 4])
        ref = _both(pa, pb, Ta, Tb, opt, k)
        for name in OUTCOMES:
            seen[name] += ref[name]
    assert all(v > 20 for v in seen.values()), seen


def _row(values, K=(8, 8, 2, 0)):
    """a one-row image whose pixel u comes back to column u under the identity: (Z [1, n], K)"""
    return np.asarray(values, F).reshape(1, -1), K


def test_near_plane_is_inclusive():
    near = F(0.75)
    a = _row([near, np.nextafter(near, F(0)), np.nextafter(near, F(1)), np.nan])
    b = _row([near, near, near, near])
    ref = _both(a, b, np.eye(4), np.eye(4), dict(near_z=near))
    assert ref["qz"][0, 0] == near and ref["qz"][0, 1] < near < ref["qz"][0, 2]       # exactly on it, one ulp below, one above
    assert list(ref["cls"][0]) == [CONSISTENT, BEHIND, CONSISTENT, -1]
    assert (ref["valid"], ref["behind"], ref["consistent"]) == (3, 1, 2)


def test_projection_rounds_half_up_at_both_image_edges():
    a = (np.array([[2.0]], F), (1, 1, 0, 0))                                          # one pixel on the optical axis: q = (0, 0, 2)
    Zb = np.full((2, 4), 2.0, F)
    hits = []
    for ox, want_pu, want in ((F(-0.5), 0, CONSISTENT), (np.nextafter(F(-0.5), F(-1)), -1, OUTSIDE),
                              (F(3.5), 4, OUTSIDE), (np.nextafter(F(3.5), F(0)), 3, CONSISTENT)):
        ref = _both(a, (Zb, (5, 5, ox, 0)), np.eye(4), np.eye(4))
        assert ref["proj_u"][0, 0] == ox and ref["pu"][0, 0] == want_pu and ref["cls"][0, 0] == want, ox
        hits.append(float(ref["proj_u"][0, 0]))
    assert hits[0] == -0.5 and hits[2] == 4 - 0.5                                     # exactly -0.5 and exactly w - 0.5
    for oy, want_pv, want in ((F(-0.5), 0, CONSISTENT), (np.nextafter(F(-0.5), F(-1)), -1, OUTSIDE), (F(1.5), 2, OUTSIDE)):
        ref = _both(a, (Zb, (5, 5, 0, oy)), np.eye(4), np.eye(4))
        assert ref["proj_v"][0, 0] == oy and ref["pv"][0, 0] == want_pv and ref["cls"][0, 0] == want, oy


def test_huge_and_nan_projections_are_outside():
    a, b = _row([1, 1, np.nan, 2]), _row([1, 1, 1, 1])
    far = np.eye(4)
    far[0, 3] = 1e30
    ref = _both(a, b, far, np.eye(4))
    assert np.isfinite(ref["pu"][0, [0, 1, 3]]).all() and (ref["pu"][0, [0, 1, 3]] >= 1e29).all()  # far beyond any int
    assert (ref["valid"], ref["outside"]) == (3, 3)
    # finite poses whose product is not: 1e200 * 1e200 - 1e200 * 1e200 in the translation of row 0
    A, B = np.eye(4), np.eye(4)
    A[0, 3], B[0, 0], B[0, 3] = 1e200, 1e200, 1e200
    assert np.isfinite(A).all() and np.isfinite(B).all()
    ref = _both(a, b, A, B)
    assert np.isnan(ref["T"][0, 3]) and np.isfinite(ref["T"][2]).all()
    assert np.isnan(ref["pu"][0, [0, 1, 3]]).all() and (ref["valid"], ref["outside"]) == (3, 3)


def _exact_tolerance():
    """(qz, depth_sigmas) for which tol is exactly 0.25 in float32"""
    for qz in (F(1.0), F(1.5), F(2.0), F(2.5), F(3.0)):
        s = qz - F(0.4)
        c = F(0.0012) + F(0.0019) * (s * s)
        for sig in (F(0.25) / c, np.nextafter(F(0.25) / c, F(0)), np.nextafter(F(0.25) / c, F(1e9))):
            if sig * c == F(0.25):
                return qz, sig
    raise AssertionError("no exact tolerance found")


def test_depth_tolerance_is_inclusive_on_both_sides():
    qz, sig = _exact_tolerance()
    tol = F(0.25)
    hi, lo = qz + tol, qz - tol
    assert hi - qz == tol and lo - qz == -tol                                        # exact in float32
    zb = [hi, np.nextafter(hi, F(9)), np.nextafter(hi, F(0)), lo, np.nextafter(lo, F(0)), np.nextafter(lo, F(9))]
    ref = _both(_row([qz] * 6), _row(zb), np.eye(4), np.eye(4), dict(depth_sigmas=sig))
    assert list(ref["pu"][0]) == list(range(6)) and (ref["qz"] == qz).all() and (ref["tol"] == tol).all()
    d = ref["d"][0]
    assert d[0] == tol and d[1] > tol and 0 < d[2] < tol and d[3] == -tol and d[4] < -tol and -tol < d[5] < 0
    assert list(ref["cls"][0]) == [CONSISTENT, SEEN_THROUGH, CONSISTENT, CONSISTENT, OCCLUDED, CONSISTENT]


def test_a_nan_pixel_of_b_counts_as_no_depth():
    ref = _both(_row([1, 1, 1, 1]), _row([1, np.nan, 1, np.nan]), np.eye(4), np.eye(4))
    assert list(ref["cls"][0]) == [CONSISTENT, NO_DEPTH, CONSISTENT, NO_DEPTH] and ref["no_depth"] == 2


def test_a_keyframe_sees_all_of_itself_and_nothing_behind_it(synth):
    rng = np.random.default_rng(5)
    w, h = 20, 15
    a = (_image(rng, w, h), synth.intrinsics_for(w, h))
    pose = synth.se3_exp([0.3, -0.2, 0.5, 0.2, -0.4, 0.1])
    ref = _both(a, a, pose, pose)
    assert ref["valid"] > 200 and ref["consistent"] == ref["valid"] and overlap(ref) == 1.0
    turned = pose @ synth.se3_exp([0, 0, 0, 0, np.pi, 0])                             # about its own y axis
    for x, y in ((pose, turned), (turned, pose)):
        ref = _both(a, a, x, y)
        assert ref["consistent"] == 0 and ref["behind"] == ref["valid"] > 200 and overlap(ref) == 0.0
    empty = (np.full((h, w), np.nan, F), a[1])
    ref = _both(empty, a, pose, pose)
    assert ref["valid"] == 0 and overlap(ref) == 0.0


# ---- the test scene of the GPU part; its conditions are conditions on the inputs and hold from the restatement alone -----------------

SCENES = {"72x50": (72, 50, 2), "80x48": (80, 48, 3), "64x32": (64, 32, 3)}
NEARBY, FAR, TURNED, SPARSE, DRIFTED = (0, 1, 2), 3, 4, (5, 6), 7
RADIUS = 1.5


def scene(synth, w, h):
    """8 keyframes of the synthetic room: (frames, poses).  0..2 at nearby poses, 3 translated by more than its view, 4 turned
    away, 5 and 6 with a third of their depth missing, 7 nearby but with a pose that has drifted 0.8 m along its view."""
    se = synth.se3_exp
    true = [np.eye(4), se(synth.XI_GT_PAIR * 4), se([0.05, -0.02, 0.03, 0.01, -0.02, 0.01]), se([5.0, 0, 0, 0, 0, 0]),
            se([0.1, 0, 0.05, 0, 0, 0]) @ se([0, 0, 0, 0, np.pi, 0]), se(synth.XI_GT_PAIR * -6),
            se([-0.03, 0.02, 0.04, -0.01, 0.015, 0.0]), se([0.02, 0.01, 0, 0, 0.01, 0])]
    frames = [synth.render(w, h, T, frame_id=i, nan_fraction=0.3 if i in SPARSE else 0.02) for i, T in enumerate(true)]
    poses = list(true)
    poses[DRIFTED] = true[DRIFTED] @ se([0, 0, 0.8, 0, 0, 0])
    return frames, poses


def check_scene_conditions(table, poses):
    """table[(a, b)]: the counts of the ordered pair at one level"""
    for name in OUTCOMES:
        assert any(c[name] > 0 for c in table.values()), name
    assert max(overlap(table[(a, b)]) for a in NEARBY for b in NEARBY if a != b) > 0.8
    for k in range(8):
        if k != TURNED:
            assert overlap(table[(TURNED, k)]) == 0.0 and overlap(table[(k, TURNED)]) == 0.0, k
    near = radius_ref(poses, 0, RADIUS)
    assert TURNED in near and FAR not in near and set(NEARBY) <= set(near)       # turned away, but well within the radius


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_scene_meets_its_conditions(synth, name):
    w, h, _ = SCENES[name]
    frames, poses = scene(synth, w, h)
    K = synth.intrinsics_for(w, h)
    table = {(a, b): covis_ref((frames[a][1], K), (frames[b][1], K), poses[a], poses[b]) for a in range(8) for b in range(8)}
    check_scene_conditions(table, poses)
    assert covis_brute((frames[0][1], K), (frames[DRIFTED][1], K), poses[0], poses[DRIFTED]) == table[(0, DRIFTED)]


# ---- CPU: the library's host side ------------------------------------------------------------------------------------------------------

class KF:
    def __init__(self, pose, image=None, id=0):
        self.pose, self.image, self.id = np.asarray(pose, np.float64), image, id


def _at(x, y=0.0, z=0.0):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


def test_both_entries_are_declared_and_exported(capi):
    text = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = capi.lib()
    for name in ("dvo_amd_covisibility", "dvo_amd_find_constraint_candidates", "dvo_amd_default_covisibility_options"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert hasattr(L, name), name
    assert "dvo_amd_covisibility_counts" in code and "dvo_amd_covisibility_options" in code
    assert "#define DVO_AMD_ABI_VERSION 3" in text and L.dvo_amd_abi_version() == 3
    assert C.sizeof(capi.CCovisibilityOptions) == 12 and capi.COVISIBILITY_DTYPE.itemsize == 32
    opt = capi.covisibility_options()
    assert (opt.level, opt.near_z, opt.depth_sigmas) == (3, F(0.1), F(20.0))


def test_radius_stage_needs_no_device_and_equals_its_restatement(capi, synth):
    rng = np.random.default_rng(3)
    poses = [synth.se3_exp(np.concatenate([rng.uniform(-1, 1, 3), rng.normal(size=3)])) for _ in range(40)]
    kfs = [KF(p) for p in poses]
    sizes = set()
    for q in (0, 7, 39):
        for r in (0.0, 0.4, 0.9, 1.5, 10.0):
            got, over = capi.find_constraint_candidates(None, kfs, q, r)            # ctx = NULL, min_overlap = 0
            assert got == radius_ref(poses, q, r) and q in got and got == sorted(got)
            assert len(over) == len(got) and np.isnan(over).all()
            sizes.add(len(got))
    assert 1 in sizes and 40 in sizes and len(sizes) > 4
    assert capi.find_constraint_candidates(None, kfs, 7, 0.9, min_overlap=-1.0)[0] == radius_ref(poses, 7, 0.9)


def test_radius_boundary_is_inclusive_in_float32(capi):
    # translations are cast to float first: 3.5000002 is another float than 3.5, 3.50000001 is not
    poses = [_at(1, 2, 3), _at(1 + 0.5, 2, 3), _at(1, 2 - 0.5, 3), _at(1, 2, 3 + 0.5000002), _at(1, 2, 3 + 0.50000001), _at(9, 9, 9)]
    assert F(3.5000002) > F(3.5) == F(3.50000001)
    got, _ = capi.find_constraint_candidates(None, [KF(p) for p in poses], 0, 0.5)
    assert got == radius_ref(poses, 0, 0.5) == [0, 1, 2, 4]
    # d2 == r * r exactly, and one ulp beyond
    r = F(0.7)
    on, beyond = float(r), float(np.nextafter(r, F(1)))
    poses = [_at(0, 0, 0), _at(on, 0, 0), _at(0, -beyond, 0), _at(0, 0, on)]
    d2 = F(on) * F(on)
    assert d2 == r * r and F(beyond) * F(beyond) > r * r
    got, _ = capi.find_constraint_candidates(None, [KF(p) for p in poses], 0, float(r))
    assert got == radius_ref(poses, 0, r) == [0, 1, 3]


def test_capacity_error_reports_the_size_needed(capi):
    kfs = [KF(_at(0.1 * k)) for k in range(6)]
    assert capi.find_constraint_candidates(None, kfs, 0, 0.35)[0] == [0, 1, 2, 3]
    for cap in (0, 1, 3):
        with pytest.raises(capi.DvoAmdError) as e:
            capi.find_constraint_candidates(None, kfs, 0, 0.35, capacity=cap)
        assert e.value.status == CAPACITY and e.value.needed == 4
    assert capi.find_constraint_candidates(None, kfs, 0, 0.35, capacity=4)[0] == [0, 1, 2, 3]


def _find_raw(capi, kfs, keyframe=0, r=1.0, min_overlap=0.0, opt="default", cand=True, capacity=None, n_out=True, n=None,
              null_keyframes=False):
    ckf = capi.pack_keyframes(kfs)
    capacity = len(kfs) if capacity is None else capacity
    out, over, cnt = (C.c_int * max(1, len(kfs)))(), (C.c_double * max(1, len(kfs)))(), C.c_int(-5)
    o = capi.covisibility_options() if opt == "default" else opt
    return capi.lib().dvo_amd_find_constraint_candidates(
        None, len(kfs) if n is None else n, None if null_keyframes else ckf, keyframe, r, min_overlap,
        C.byref(o) if o is not None else None, out if cand else None, over, capacity, C.byref(cnt) if n_out else None)


def test_search_rejects_bad_arguments_before_any_device(capi):
    kfs = [KF(_at(0.1 * k)) for k in range(4)]
    assert _find_raw(capi, kfs) == 0
    assert _find_raw(capi, kfs, opt=None) == 0                                    # the options are not read when min_overlap <= 0
    assert _find_raw(capi, kfs, null_keyframes=True) == INVALID
    assert _find_raw(capi, kfs, n=0) == INVALID
    assert _find_raw(capi, kfs, n_out=False) == INVALID
    assert _find_raw(capi, kfs, keyframe=-1) == INVALID and _find_raw(capi, kfs, keyframe=4) == INVALID
    assert _find_raw(capi, kfs, capacity=-1) == INVALID and _find_raw(capi, kfs, cand=False) == INVALID
    for r in (-0.5, float("nan"), float("inf")):
        assert _find_raw(capi, kfs, r=r) == INVALID, r
    assert _find_raw(capi, kfs, min_overlap=float("nan")) == INVALID
    for bad in (np.nan, np.inf):
        broken = [KF(_at(0.1 * k)) for k in range(4)]
        broken[2].pose[1, 3] = bad
        assert _find_raw(capi, broken) == INVALID
        assert b"pose" in capi.lib().dvo_amd_last_error()
    # with min_overlap > 0 the checks of dvo_amd_covisibility come first too: options, then the images
    assert _find_raw(capi, kfs, min_overlap=0.5, opt=None) == INVALID
    for field, value in (("level", -1), ("depth_sigmas", -1.0), ("depth_sigmas", float("nan")), ("depth_sigmas", float("inf")),
                         ("near_z", 0.0), ("near_z", -1.0), ("near_z", float("nan")), ("near_z", float("inf"))):
        assert _find_raw(capi, kfs, min_overlap=0.5, opt=capi.covisibility_options(**{field: value})) == INVALID, (field, value)
    assert _find_raw(capi, kfs, min_overlap=0.5) == INVALID                      # keyframes without an image
    assert b"image" in capi.lib().dvo_amd_last_error()


def _covis_raw(capi, kfs, pairs, opt="default", ctx=None, null=(), n_keyframes=None):
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
    out = np.zeros(max(1, len(pairs)), capi.COVISIBILITY_DTYPE)
    ip = C.POINTER(C.c_int)
    o = capi.covisibility_options() if opt == "default" else opt
    return capi.lib().dvo_amd_covisibility(
        ctx, len(kfs) if n_keyframes is None else n_keyframes, None if "keyframes" in null else capi.pack_keyframes(kfs),
        C.byref(o) if o is not None else None, len(pairs), None if "a" in null else pa.ctypes.data_as(ip),
        None if "b" in null else pb.ctypes.data_as(ip), None if "out" in null else out.ctypes.data_as(C.c_void_p))


class _FakeImage:
    _h = 0x1000  # never dereferenced: every call below is rejected before the image is looked at


def test_covisibility_rejects_bad_arguments_before_any_device(capi):
    kfs = [KF(_at(0.1 * k), _FakeImage()) for k in range(3)]
    pairs = [(0, 1), (2, 0)]
    for null in ("keyframes", "a", "b", "out"):
        assert _covis_raw(capi, kfs, pairs, null=(null,)) == INVALID, null
    assert _covis_raw(capi, kfs, pairs, opt=None) == INVALID
    for bad in [(0, 3)], [(-1, 0)], [(0, 1), (3, 1)]:
        assert _covis_raw(capi, kfs, bad) == INVALID, bad
    assert b"out of range" in capi.lib().dvo_amd_last_error()
    assert _covis_raw(capi, kfs, pairs, n_keyframes=2) == INVALID
    assert _covis_raw(capi, [kfs[0], KF(_at(1)), kfs[2]], [(0, 2), (2, 1)]) == INVALID   # a NULL image
    assert b"image" in capi.lib().dvo_amd_last_error()
    broken = [KF(_at(0.1 * k), _FakeImage()) for k in range(3)]
    broken[1].pose[0, 0] = np.nan
    assert _covis_raw(capi, broken, pairs) == INVALID
    for field, value in (("level", -1), ("depth_sigmas", -1.0), ("depth_sigmas", float("nan")), ("depth_sigmas", float("inf")),
                         ("near_z", 0.0), ("near_z", -1.0), ("near_z", float("nan")), ("near_z", float("inf"))):
        assert _covis_raw(capi, kfs, pairs, opt=capi.covisibility_options(**{field: value})) == INVALID, (field, value)
    assert _covis_raw(capi, kfs, pairs, n_keyframes=-1) == INVALID


def test_covisibility_fails_loudly_without_a_gpu(capi):
    if capi.lib().dvo_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    kfs = [KF(_at(0.1 * k), _FakeImage()) for k in range(3)]
    assert _covis_raw(capi, kfs, [(0, 1), (2, 0)]) == NO_DEVICE                    # valid arguments, no device: never a CPU path
    assert _covis_raw(capi, kfs, []) == NO_DEVICE
    kfs[1].pose[0, 0] = np.nan
    assert _covis_raw(capi, kfs, [(2, 0), (0, 2)]) == NO_DEVICE                    # only the keyframes the pairs name are checked
    kfs[1].pose[0, 0] = 1.0
    assert _find_raw(capi, kfs, min_overlap=0.5) == NO_DEVICE
    assert _find_raw(capi, kfs, min_overlap=0.0) == 0


def test_python_search_mirror_without_a_gpu(capi):
    from dvo_slam_amd import constraints as Cn

    kfs = [Cn.Keyframe(10 + k, None, _at(0.2 * k), None) for k in range(6)]
    s = Cn.NearestNeighborConstraintSearch(0.5)
    assert s.maxDistance() == 0.5 and s.minOverlap() == 0.0
    assert [k.id for k in s.findPossibleConstraints(kfs, kfs[2])] == [10, 11, 12, 13, 14]
    assert s.maxDistance(0.25) == 0.25
    assert [k.id for k in s.findPossibleConstraints(kfs, kfs[2])] == [11, 12, 13] and np.isnan(s.overlaps).all()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capi_gpu():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


ALL_PAIRS = [(a, b) for a in range(8) for b in range(8)]


class Scene:
    def __init__(self, capi, synth, name):
        from dvo_slam_amd import constraints as Cn

        self.w, self.h, self.levels = SCENES[name]
        frames, self.poses = scene(synth, self.w, self.h)
        K = synth.intrinsics_for(self.w, self.h)
        self.pyramids = [capi.RgbdImagePyramid(I, Z, K, self.levels) for I, Z in frames]
        self.keyframes = [Cn.Keyframe(2 * k, p, T, None) for k, (p, T) in enumerate(zip(self.pyramids, self.poses))]
        # what the library reads: the depth plane and the intrinsics of every level, downloaded
        self.planes = [[(p.plane(l, 1), tuple(p.level_info(l)[2])) for l in range(self.levels)] for p in self.pyramids]
        assert all(np.array_equal(self.planes[k][0][0], frames[k][1], equal_nan=True) for k in range(8))
        self._tables = {}

    def table(self, level, **opt):
        """the restatement's counts of all 64 ordered pairs at a level (computed once, shared)"""
        key = (level, tuple(sorted(opt.items())))
        if key not in self._tables:
            self._tables[key] = {(a, b): covis_ref(self.planes[a][level], self.planes[b][level], self.poses[a], self.poses[b], opt)
                                 for a, b in ALL_PAIRS}
        return self._tables[key]


@pytest.fixture(scope="module")
def scenes(capi_gpu, synth):
    return {name: Scene(capi_gpu, synth, name) for name in SCENES}


@pytest.fixture(scope="module")
def tracker(capi_gpu):
    return capi_gpu.DenseTracker()


def _as_dicts(counts):
    assert (counts["reserved"] == 0).all()
    return [{k: int(c[k]) for k in COUNTS} for c in counts]


def _expected(table, pairs):
    return [table[tuple(p)] for p in pairs]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_counts_equal_the_restatement_on_every_level(capi_gpu, scenes, tracker, name):
    s = scenes[name]
    check_scene_conditions(s.table(0), s.poses)
    sizes = [s.planes[0][l][0].size for l in range(s.levels)]
    assert sizes == {"72x50": [3600, 900], "80x48": [3840, 960, 240], "64x32": [2048, 512, 128]}[name]
    for level in range(s.levels):
        got = _as_dicts(capi_gpu.covisibility(tracker, s.keyframes, ALL_PAIRS, level=level))
        assert got == _expected(s.table(level), ALL_PAIRS), (name, level)
        assert all(g["valid"] == sum(g[k] for k in OUTCOMES) for g in got)
    # a level the pyramids do not have is clamped to their coarsest; the default options ask for level 3
    coarsest = _expected(s.table(s.levels - 1), ALL_PAIRS)
    assert _as_dicts(capi_gpu.covisibility(tracker, s.keyframes, ALL_PAIRS)) == coarsest
    assert _as_dicts(capi_gpu.covisibility(tracker, s.keyframes, ALL_PAIRS, level=7)) == coarsest
    # other options than the defaults
    opt = dict(level=0, near_z=2.5, depth_sigmas=0.5)
    assert _as_dicts(capi_gpu.covisibility(tracker, s.keyframes, ALL_PAIRS, **opt)) == _expected(s.table(0, near_z=2.5, depth_sigmas=0.5), ALL_PAIRS)


@pytest.mark.gpu
def test_pairs_of_keyframes_of_different_sizes(capi_gpu, scenes, tracker):
    """a from one scene, b from another: a's own rays, b's size and intrinsics; the level clamped to what both have"""
    sa, sb = scenes["80x48"], scenes["72x50"]
    kfs = sa.keyframes + sb.keyframes
    pairs = [(a, 8 + b) for a in (0, 1, 5, 7) for b in (0, 2, 4)] + [(8 + b, a) for a in (0, 1, 5, 7) for b in (0, 2, 4)]
    for level in (0, 1, 2):
        l = min(level, 1)
        want = []
        for x, y in pairs:
            px = (sa.planes[x][l], sa.poses[x]) if x < 8 else (sb.planes[x - 8][l], sb.poses[x - 8])
            py = (sa.planes[y][l], sa.poses[y]) if y < 8 else (sb.planes[y - 8][l], sb.poses[y - 8])
            want.append({k: v for k, v in covis_ref(px[0], py[0], px[1], py[1]).items()})
        assert _as_dicts(capi_gpu.covisibility(tracker, kfs, pairs, level=level)) == want, level
        assert sum(w["consistent"] for w in want) > 1000


@pytest.mark.gpu
def test_counts_do_not_depend_on_the_batch(capi_gpu, scenes, tracker):
    s = scenes["80x48"]
    for level in (0, 2):
        want = s.table(level)
        run = lambda pairs: _as_dicts(capi_gpu.covisibility(tracker, s.keyframes, pairs, level=level))  # noqa: E731
        assert run(ALL_PAIRS[::-1]) == _expected(want, ALL_PAIRS[::-1])
        for p in ALL_PAIRS[::5]:
            assert run([p]) == [want[p]], p
        repeats = [(0, 1), (0, 1), (4, 4), (0, 1), (7, 0), (4, 4), (3, 3), (0, 1)] * 3
        assert run(repeats) == _expected(want, repeats)
    assert len(capi_gpu.covisibility(tracker, s.keyframes, [])) == 0                # n_pairs == 0 is OK


@pytest.mark.gpu
def test_buffers_are_reused_and_regrown(capi_gpu, scenes):
    s, big = scenes["64x32"], scenes["80x48"]
    first, second = capi_gpu.DenseTracker(), capi_gpu.DenseTracker()
    want = _expected(s.table(0), ALL_PAIRS)
    assert _as_dicts(capi_gpu.covisibility(first, s.keyframes, ALL_PAIRS[:3], level=0)) == want[:3]   # cold, small
    assert _as_dicts(capi_gpu.covisibility(first, s.keyframes, ALL_PAIRS, level=0)) == want           # regrown
    assert _as_dicts(capi_gpu.covisibility(first, s.keyframes, ALL_PAIRS, level=0)) == want           # warm
    many = ALL_PAIRS * 40                                                                             # 2560 pairs: regrown again
    assert _as_dicts(capi_gpu.covisibility(first, big.keyframes, many, level=0)) == _expected(big.table(0), many)
    assert _as_dicts(capi_gpu.covisibility(first, s.keyframes, ALL_PAIRS[:5], level=1)) == _expected(s.table(1), ALL_PAIRS[:5])
    assert _as_dicts(capi_gpu.covisibility(second, s.keyframes, ALL_PAIRS, level=0)) == want          # another context
    assert capi_gpu.covisibility_ms(first) > 0.0


@pytest.mark.gpu
def test_smallest_image_and_an_image_without_depth(capi_gpu, synth, tracker):
    """4x2 is the smallest pyramid there is (a 1x1 image cannot be a keyframe: dvo_amd_pyramid_create needs 4x2)"""
    from dvo_slam_amd import constraints as Cn

    K = (F(3), F(3), F(1.5), F(0.5))
    Z = np.array([[1, 1.5, np.nan, 2], [2, 1, 1, 1.25]], F)
    I = np.full((2, 4), 100, F)
    tiny = capi_gpu.RgbdImagePyramid(I, Z, K, 1)
    blind = capi_gpu.RgbdImagePyramid(I, np.full((2, 4), np.nan, F), K, 1)
    T = synth.se3_exp([0.05, 0, 0, 0, 0, 0])
    kfs = [Cn.Keyframe(0, tiny, np.eye(4), None), Cn.Keyframe(2, tiny, T, None), Cn.Keyframe(4, blind, np.eye(4), None)]
    planes = [(Z, K), (Z, K), (np.full((2, 4), np.nan, F), K)]
    pairs = [(a, b) for a in range(3) for b in range(3)]
    got = capi_gpu.covisibility(tracker, kfs, pairs)
    want = [covis_ref(planes[a], planes[b], kfs[a].pose, kfs[b].pose) for a, b in pairs]
    assert _as_dicts(got) == want
    assert want[0]["valid"] == want[0]["consistent"] == 7
    over = capi_gpu.covisibility_overlap(got)
    for i, (a, b) in enumerate(pairs):
        assert over[i] == overlap(want[i])
        if a == 2:
            assert got[i]["valid"] == 0 and over[i] == 0.0                          # an all-NaN a: nothing valid, overlap 0
        if b == 2 and a != 2:
            assert got[i]["consistent"] == 0 and got[i]["no_depth"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_candidate_search_prunes_by_overlap(capi_gpu, scenes, tracker, name):
    s = scenes[name]
    table = s.table(s.levels - 1)                                                   # the default level 3, clamped

    def ov(a, b):
        return overlap(table[(a, b)])

    both = lambda c: max(ov(0, c), ov(c, 0))  # noqa: E731
    radius = radius_ref(s.poses, 0, RADIUS)
    assert TURNED in radius and both(TURNED) == 0.0
    nearby = min(both(c) for c in NEARBY)
    assert nearby > 0.5
    min_overlap = 0.5 * nearby                                                      # between the turned-away keyframe and the nearby ones
    want, want_over = candidates_ref(s.poses, 0, RADIUS, min_overlap, ov)
    got, over = capi_gpu.find_constraint_candidates(tracker, s.keyframes, 0, RADIUS, min_overlap)
    assert got == want and TURNED not in got and set(NEARBY) <= set(got) and len(got) < len(radius)
    assert over.tobytes() == np.asarray(want_over, np.float64).tobytes()            # bit for bit
    # every query keyframe, and a threshold nothing but a keyframe itself passes
    for q in range(8):
        want, want_over = candidates_ref(s.poses, q, RADIUS, min_overlap, ov)
        got, over = capi_gpu.find_constraint_candidates(tracker, s.keyframes, q, RADIUS, min_overlap)
        assert got == want and over.tobytes() == np.asarray(want_over, np.float64).tobytes(), q
    # min_overlap = 0: the reference's search, with or without a context
    for q in (0, 3, 4):
        got, over = capi_gpu.find_constraint_candidates(tracker, s.keyframes, q, RADIUS)
        assert got == radius_ref(s.poses, q, RADIUS) and np.isnan(over).all()
    assert capi_gpu.find_constraint_candidates(None, s.keyframes, 0, RADIUS)[0] == radius
    # capacity counts what is kept, not what the radius holds
    kept = len(candidates_ref(s.poses, 0, RADIUS, min_overlap, ov)[0])
    with pytest.raises(capi_gpu.DvoAmdError) as e:
        capi_gpu.find_constraint_candidates(tracker, s.keyframes, 0, RADIUS, min_overlap, capacity=kept - 1)
    assert e.value.status == CAPACITY and e.value.needed == kept


@pytest.mark.gpu
def test_search_result_feeds_the_validator(capi_gpu, synth):
    import validator_scenario as S
    from dvo_slam_amd import constraints as Cn

    key, cands = S.gpu_keyframes(capi_gpu, Cn, synth, 320, 240, 3)                  # 3 candidates and the 3 decoys
    all_kfs = [key] + cands
    search = Cn.NearestNeighborConstraintSearch(1.0, 0.5, level=3)
    found = search.findPossibleConstraints(all_kfs, key)
    ids = [k.id for k in found]
    assert key in found and 70 not in ids                                           # the decoy without depth overlaps nothing
    assert len(search.overlaps) == len(found) and (search.overlaps >= 0.5).all()
    nearby = [k for k in found if k.id in (0, 2, 4)]
    assert nearby
    plain = Cn.NearestNeighborConstraintSearch(1.0).findPossibleConstraints(all_kfs, key)
    assert [k.id for k in plain] == [k.id for k in all_kfs]                          # the reference's search keeps them all
    val = Cn.createConstraintProposalValidator(min_constraint_ratio=0.0, ratio_coarse=-1e300, ratio_fine=-1e300)
    survivors = val.validate(Cn.proposalsForCandidates(key, found))
    assert any(p.Reference is key and p.Current in nearby or p.Current is key and p.Reference in nearby for p in survivors)
    assert all(not (p.Reference is key and p.Current is key) for p in survivors)    # the odometry voter rejects the keyframe itself


@pytest.mark.gpu
def test_remaining_error_cases_on_the_device(capi_gpu, scenes, synth, tracker):
    s = scenes["64x32"]
    L = capi_gpu.lib()
    assert _covis_raw(capi_gpu, s.keyframes, [(0, 1)], ctx=None) == INVALID         # a NULL context, once a device is there
    assert _covis_raw(capi_gpu, s.keyframes, [], ctx=tracker._h) == 0
    if L.dvo_amd_device_count() >= 2:
        other = capi_gpu.DenseTracker(device=1)
        assert _covis_raw(capi_gpu, s.keyframes, [(0, 1)], ctx=other._h) == MISMATCH
        with pytest.raises(capi_gpu.DvoAmdError) as e:
            capi_gpu.find_constraint_candidates(other, s.keyframes, 0, RADIUS, 0.3)
        assert e.value.status == MISMATCH
    K4 = synth.intrinsics_for(320, 240)
    ref = capi_gpu.RgbdImagePyramid.from_raw(*synth.sensor_frame(320, 240, None, frame_id=0), K4, 4)
    nxt = capi_gpu.RgbdImagePyramid.from_raw(*synth.sensor_frame(320, 240, synth.se3_exp(synth.XI_GT_PAIR * 0.5), frame_id=1), K4, 4)
    before = _as_dicts(capi_gpu.covisibility(tracker, s.keyframes, ALL_PAIRS[:9], level=0))
    sub = tracker.submit([ref] * 4, [nxt] * 4, in_flight=4)
    try:
        assert _covis_raw(capi_gpu, s.keyframes, [(0, 1)], ctx=tracker._h) == INVALID
        assert b"in flight" in L.dvo_amd_last_error()
        with pytest.raises(capi_gpu.DvoAmdError) as e:
            capi_gpu.find_constraint_candidates(tracker, s.keyframes, 0, RADIUS, 0.3)
        assert e.value.status == INVALID
        assert capi_gpu.find_constraint_candidates(tracker, s.keyframes, 0, RADIUS)[0] == radius_ref(s.poses, 0, RADIUS)
    finally:
        tracker.wait(sub)
    assert _as_dicts(capi_gpu.covisibility(tracker, s.keyframes, ALL_PAIRS[:9], level=0)) == before == _expected(s.table(0), ALL_PAIRS[:9])
