"""The projection kernels on their one-ulp boundaries: k_covis, k_mask_warp, k_fuse_depth and the map renderer
(include/dvo_amd.h pins the rules; tests/projection_boundary_cases.py holds the cases).

The rendered rooms of the kernels' own test files essentially never put a value exactly on a boundary, so a kernel with
`qz > near_z`, `rintf(p)`, `d <= -tol`, `c > min_cos` or a z-buffer tie that goes to the higher rank would pass them.  Here every
case is a few pixels that sit on one boundary, one ulp below it and one ulp above it.
CPU: every case proves, from the restatement's own intermediate values, that it hits what its name says -- a case whose condition
does not hold fails here instead of passing vacuously on the device -- and the restatement agrees with its independent pixel loop.
GPU: the library against the restatement.  Every comparison is equality; there is no tolerance anywhere in this file."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_fusion_ref as fuse_ref  # noqa: E402
import mask_ops_ref as mask_ref  # noqa: E402
import projection_boundary_cases as cases  # noqa: E402
from covisibility_ref import COUNTS, covis_brute, covis_ref  # noqa: E402
from map_render_ref import make_view, near_limit, render_brute, render_ref  # noqa: E402
from test_map_cloud import same_bits  # noqa: E402

F = np.float32
PAIRS = {p.name: p for p in cases.pair_cases()}
FUSES = {f.name: f for f in cases.fuse_cases()}
RENDERS = {r.name: r for r in cases.render_cases()}
KEEPS = [(0, 0), (1, 1), (1, 0), (0, 1)]  # (unseen_keep, inconsistent_keep)
SAMPLE_NAMES = {fuse_ref.BILINEAR: "bilinear", fuse_ref.NEAREST: "nearest"}
PLANES = ("depth", "rgb", "intensity", "index")


def _counts_of(cls):
    """the seven counts of one pixel of class cls (-1: no depth)"""
    return {name: int(k == 0 and cls >= 0 or k == cls and k > 0) for k, name in enumerate(COUNTS)}


def _pair_info(p):
    return covis_ref(p.a, p.b, p.Ta, p.Tb, p.opt, info=True)


# ---- CPU: every case hits what its name says ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PAIRS))
def test_pair_case_sits_on_its_boundary(name):
    p = PAIRS[name]
    info = _pair_info(p)
    p.prove(info)
    n = len(p.classes)
    assert [int(c) for c in info["cls"][0, :n]] == p.classes
    assert (info["cls"][0, n:] == -1).all() and (info["cls"][1] == -1).all()        # the embedding adds no pixel
    assert {k: info[k] for k in COUNTS} == covis_brute(p.a, p.b, p.Ta, p.Tb, p.opt)
    for i, cls in enumerate(p.classes):                                                # ... and every pixel keeps its class alone
        alone = covis_ref((cases.only(p.a[0], i), p.a[1]), p.b, p.Ta, p.Tb, p.opt)
        assert alone == _counts_of(cls), (i, cls, alone)


def test_the_named_boundaries_are_all_there():
    """the list of the issue, by name: a case that is dropped or renamed shows here"""
    for name in ["near", "tolerance", "nan_in_b", "nan_transform", "special_in_a", "special_in_b"] + \
                [f"half_up_u{k}" for k in range(6)] + [f"half_up_v{k}" for k in range(7)] + [f"far_{a}" for a in ("x+", "x-", "y+", "y-", "z-")]:
        assert name in PAIRS, name
    for name in ["pair_near", "pair_tolerance", "pair_nan_in_b", "min_cos_at", "min_cos_above", "convention", "convention_inverse",
                 "corners_alone", "corners_all"] + [f"pair_half_up_u{k}" for k in range(6)] + [f"pair_half_up_v{k}" for k in range(7)] + \
                [f"window_{a}{k}" for a in "xy" for k in range(5)] + [f"corner{k}" for k in range(4)] + \
                [f"min_observations_{n}_drop{d}" for n in (3, 4) for d in (0, 1)]:
        assert name in FUSES, name
    assert sorted(RENDERS) == ["borders", "fallback", "footprints", "near", "wall"]
    assert [c[0] for c in cases.CHUNK_CASES] == ["1024_last", "1028_last", "1028_chunk_edge", "1028_first_and_last"]
    assert [np.prod(c[1]) for c in cases.CHUNK_CASES] == [1024, 1028, 1028, 1028]    # kChunk = 1024 of dvo_covisibility.cpp


@pytest.mark.parametrize("name", sorted(p.name for p in PAIRS.values() if p.single_T))
def test_warp_case_keeps_the_classes(name):
    """the whole mask: kept iff consistent under (0, 0); the other keep settings decide the pixels their names say"""
    p = PAIRS[name]
    ones = np.ones(p.b[0].shape, np.uint8)
    n = len(p.classes)
    cls = np.full(p.a[0].shape, -1)
    cls[0, :n] = p.classes
    for unseen, inconsistent in KEEPS:
        plane, counts = mask_ref.warp_ref(ones, p.a, p.b, p.Ta, dict(p.opt, unseen_keep=unseen, inconsistent_keep=inconsistent))
        want = np.where(cls == cases.CONSISTENT, 1, np.where((cls == cases.OCCLUDED) | (cls == cases.SEEN_THROUGH), inconsistent, unseen))
        assert np.array_equal(plane, want), (unseen, inconsistent)
        assert counts["dropped_by_source"] == 0 and {k: counts[k] for k in COUNTS} == {k: v for k, v in _pair_info(p).items() if k in COUNTS}


@pytest.mark.parametrize("name", sorted(FUSES))
def test_fuse_case_sits_on_its_boundary(name):
    f = FUSES[name]
    for sample in f.samples:
        info = []
        res = f.ref(sample, info)
        f.prove(sample, res, info)
        brute = fuse_ref.fuse_brute(f.key, f.frames, f.Ts, dict(f.opt, sample=sample))
        assert np.array_equal(res[0], brute[0], equal_nan=True) and np.array_equal(res[1], brute[1]), sample
        assert res[2] == brute[2] and res[3] == brute[3], sample
        plain = f.ref(sample)                                                          # info changes nothing that is returned
        assert same_bits(plain[0], res[0]) and same_bits(plain[1], res[1]) and plain[2:] == res[2:]


def _render_refs(case, xyz, rgb, view):
    label, pose, K, w, h, near = view
    v = make_view(w, h, K, cases.view_near(case, K, near))
    assert v.near_z >= near_limit(case.leaf, K)                                       # a view the entry accepts
    return render_ref(xyz, rgb, case.leaf, pose, v), render_brute(xyz, rgb, case.leaf, pose, v)


def _assert_same_render(a, b, what):
    assert a["stats"] == b["stats"], (what, a["stats"], b["stats"])
    for p in PLANES:
        assert same_bits(a[p], b[p]), (what, p)


@pytest.mark.parametrize("name", sorted(RENDERS))
def test_render_case_sits_on_its_boundary(name):
    """on the extract the voxel restatement predicts (the GPU part holds the map to it before it compares a render)"""
    case = RENDERS[name]
    xyz, rgb = case.extract()
    for view in case.views:
        ref, brute = _render_refs(case, xyz, rgb, view)
        _assert_same_render(ref, brute, (name, view[0]))
        case.prove(view[0], xyz, ref, brute)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


@pytest.fixture(scope="module")
def tracker(gpu):
    return gpu.DenseTracker()


def _pyramid(gpu, Z, K):
    """a one-level pyramid with this depth plane, and what the library reads of it, downloaded: it is the plane, bit for bit"""
    Z = np.ascontiguousarray(Z, F)
    p = gpu.RgbdImagePyramid(np.zeros(Z.shape, F), Z, K, 1)
    assert same_bits(p.plane(0, 1), Z), "the constructor changed the depth plane"
    assert same_bits(np.asarray(p.level_info(0)[2], F), np.asarray(K, F))
    return p


def _as_dicts(records):
    assert (records["reserved"] == 0).all()
    return [{k: int(r[k]) for k in COUNTS} for r in records]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PAIRS))
def test_covisibility_of_every_boundary_pixel(gpu, tracker, name):
    """the entry returns counts only, so every pixel of a is a pair of its own: the seven counts name its class"""
    from dvo_slam_amd import constraints as Cn

    p = PAIRS[name]
    n = len(p.classes)
    kfs = [Cn.Keyframe(0, _pyramid(gpu, p.b[0], p.b[1]), p.Tb, None), Cn.Keyframe(1, _pyramid(gpu, p.a[0], p.a[1]), p.Ta, None)]
    kfs += [Cn.Keyframe(2 + i, _pyramid(gpu, cases.only(p.a[0], i), p.a[1]), p.Ta, None) for i in range(n)]
    pairs = [(1 + i, 0) for i in range(n + 1)]
    got = _as_dicts(gpu.covisibility(tracker, kfs, pairs, level=0, **p.opt))
    whole = covis_ref(p.a, p.b, p.Ta, p.Tb, p.opt)
    print(name, got)
    assert got[0] == whole, (name, "the whole row")
    for i, cls in enumerate(p.classes):
        assert got[1 + i] == _counts_of(cls), (name, i, cls, got[1 + i])
    assert _as_dicts(gpu.covisibility(tracker, kfs, pairs[::-1], **p.opt)) == got[::-1]   # (the default level is clamped to 0)


@pytest.mark.gpu
def test_covisibility_at_the_chunk_edge(gpu, tracker):
    from dvo_slam_amd import constraints as Cn

    b = (cases.embed([1] * 4, 1), cases.ROW_K)
    kfs, want = [Cn.Keyframe(0, _pyramid(gpu, *b), np.eye(4), None)], []
    for _, shape, pixels in cases.CHUNK_CASES:
        Z = cases.chunk_plane(shape, pixels)
        kfs.append(Cn.Keyframe(len(kfs), _pyramid(gpu, Z, cases.CHUNK_K), np.eye(4), None))
        want.append(covis_ref((Z, cases.CHUNK_K), b, np.eye(4), np.eye(4)))
        assert want[-1]["valid"] == want[-1]["consistent"] == len(pixels)
    pairs = [(k, 0) for k in range(1, len(kfs))]
    assert _as_dicts(gpu.covisibility(tracker, kfs, pairs, level=0)) == want
    for pair, w in zip(pairs, want):                                                  # ... and each alone: its own launch geometry
        assert _as_dicts(gpu.covisibility(tracker, kfs, [pair], level=0)) == [w]


def _warp_counts(records):
    return [{k: int(r[k]) for k in mask_ref.WARP_COUNTS} for r in records]


def _warp_on_the_device(gpu, tracker, mask0, target, source, T, opt, what):
    """the warp of mask0 (on the source's pixels) under every keep setting against warp_ref: plane, counts, kept; and the counts
    against the covisibility counts of the same pair"""
    from dvo_slam_amd import constraints as Cn

    pt, ps = _pyramid(gpu, *target), _pyramid(gpu, *source)
    mask = gpu.SelectionMask.from_level0(mask0, 1)
    covis = _as_dicts(gpu.covisibility(tracker, [Cn.Keyframe(0, pt, T, None), Cn.Keyframe(1, ps, np.eye(4), None)], [(0, 1)], level=0, **opt))[0]
    planes = {}
    for unseen, inconsistent in KEEPS:
        o = dict(opt, unseen_keep=unseen, inconsistent_keep=inconsistent)
        want_plane, want_counts = mask_ref.warp_ref(mask0, target, source, T, o)
        got, counts = mask.warp(ps, pt, T, counts=True, **o)
        assert np.array_equal(got.download(0), want_plane), (what, o)
        assert _warp_counts(counts) == [want_counts], (what, o)
        assert got.info()["kept"] == [int(want_plane.sum())], (what, o)
        assert {k: want_counts[k] for k in COUNTS} == covis, (what, o)
        planes[(unseen, inconsistent)] = want_plane
    return planes


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(p.name for p in PAIRS.values() if p.single_T))
def test_warp_of_every_boundary_pixel(gpu, tracker, name):
    p = PAIRS[name]
    planes = _warp_on_the_device(gpu, tracker, np.ones(p.b[0].shape, np.uint8), p.a, p.b, p.Ta, p.opt, name)
    n = len(p.classes)
    assert list(planes[(0, 0)][0, :n]) == [int(c == cases.CONSISTENT) for c in p.classes]   # kept iff consistent


@pytest.mark.gpu
def test_warp_convention_on_the_device(gpu, tracker):
    """test_mask_ops.py: test_warp_convention_on_an_exact_case -- a shift of exactly 3 pixels, with T and with its inverse"""
    w, h = 24, 10
    K = (64.0, 64.0, 11.0, 4.0)
    Z = np.full((h, w), 2.0, F)
    T = np.eye(4)
    T[0, 3] = 3 * 2 / 64
    ms = np.zeros((h, w), np.uint8)
    ms[2:7, 9:15] = 1
    ms[8, 23] = 1
    want, back = np.zeros_like(ms), np.zeros_like(ms)
    want[:, :w - 3], back[:, 3:] = ms[:, 3:], ms[:, :w - 3]
    assert np.array_equal(_warp_on_the_device(gpu, tracker, ms, (Z, K), (Z, K), T, {}, "T")[(0, 0)], want)
    assert np.array_equal(_warp_on_the_device(gpu, tracker, ms, (Z, K), (Z, K), np.linalg.inv(T), {}, "inv(T)")[(0, 0)], back)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FUSES))
def test_fusion_on_every_boundary(gpu, name):
    f = FUSES[name]
    key = _pyramid(gpu, *f.key)
    made = {id(fr): _pyramid(gpu, *fr) for fr in {id(fr): fr for fr in f.frames}.values()}   # (a repeated frame is uploaded once)
    frames = [made[id(fr)] for fr in f.frames]
    for sample in f.samples:
        want = f.ref(sample)
        p, fc, kc, obs = key.fuse_depth(frames, f.Ts, dict(f.opt, sample=sample), counts=True, observations=True)
        fused = p.plane(0, 1)
        got_fc = [{k: int(r[k]) for k in fuse_ref.FRAME_COUNTS} for r in fc]
        got_kc = {k: int(kc[k]) for k in fuse_ref.KEYFRAME_COUNTS}
        print(name, SAMPLE_NAMES[sample], got_fc[0], got_kc)
        assert got_fc == want[2], (name, SAMPLE_NAMES[sample])
        assert got_kc == want[3], (name, SAMPLE_NAMES[sample])
        assert obs.dtype == np.uint8 and np.array_equal(obs, want[1]), (name, SAMPLE_NAMES[sample])
        assert fused.dtype == F and np.array_equal(np.isnan(fused), np.isnan(want[0])), (name, SAMPLE_NAMES[sample])
        assert np.array_equal(fused, want[0], equal_nan=True), (name, SAMPLE_NAMES[sample])


def _build_map(gpu, case, order):
    m = gpu.KeyframeMap(gpu.DenseTracker(), case.leaf)
    for k in order:
        I, Z, K, pose = case.keyframes[k]
        p = gpu.RgbdImagePyramid(I, Z, K, 1)
        assert same_bits(p.plane(0, 1), Z)
        m.insert(k, p, pose, None)
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RENDERS))
def test_render_on_every_boundary(gpu, name):
    case = RENDERS[name]
    xyz, rgb = case.extract()
    maps = [_build_map(gpu, case, order) for order in case.orders]
    for m in maps:                                                                    # the conditions hold on what the map holds
        ext = m.extract()
        assert same_bits(ext[0], xyz) and same_bits(ext[1], rgb), name
    for view in case.views:
        label, pose, K, w, h, near = view
        ref, brute = _render_refs(case, xyz, rgb, view)
        case.prove(label, xyz, ref, brute)
        for m in maps:                                                                # (in every insertion order: the same planes)
            got = m.render(pose, K, w, h, near=cases.view_near(case, K, near))
            print(name, label, got["stats"])
            _assert_same_render(got, ref, (name, label))
