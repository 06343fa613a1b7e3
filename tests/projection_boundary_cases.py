"""Crafted boundary cases of the kernels that decide a pixel by float comparisons after a rigid transform and a pinhole projection:
k_covis, k_mask_warp, k_fuse_depth and the map renderer (include/dvo_amd.h pins their rules; covisibility_ref, mask_ops_ref,
depth_fusion_ref and map_render_ref restate them).  tests/test_projection_boundaries.py proves on the CPU that every case sits on
the boundary its name says, and compares the device with the restatement on it.

Device-shaped cases.  A pyramid level is at least 4x2 and its width a multiple of 4, so a case of a few pixels is embedded: its
pixels are row 0 of a two-row plane whose width is padded to a multiple of 4.  In the image that is walked the padding and row 1
are NaN (no pixel is added); in the image that is looked up they carry a depth where the case wants a hit.

pair_cases()     one ordered pair (a, b) each: covisibility of every pixel of a on its own, the warp of a whole mask
fuse_cases()     one keyframe with its frames each
render_cases()   keyframes that build a map, and the views it is rendered into"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_fusion_ref as fuse  # noqa: E402
from map_render_ref import default_near  # noqa: E402
from test_covisibility import _exact_tolerance  # noqa: E402
from test_map_cloud import cloud_ref, voxel_ref  # noqa: E402

F = np.float32
NAN = np.nan
BEHIND, OUTSIDE, NO_DEPTH, CONSISTENT, OCCLUDED, SEEN_THROUGH = range(1, 7)
ROW_K = (8, 8, 2, 0)      # under the identity pixel u of row 0 comes back to column u of row 0
AXIS_K = (1, 1, 0, 0)     # pixel (0, 0) lies on the optical axis


def bits(x):
    return np.asarray(x, F).view(np.uint32)


def below(x):
    return np.nextafter(F(x), F(-np.inf))


def above(x):
    return np.nextafter(F(x), F(np.inf))


def embed(values, fill=NAN):
    """row 0 = values, the padding to a multiple of 4 and row 1 = fill: float32 [2, w]"""
    v = np.asarray(values, F).reshape(-1)
    Z = np.full((2, max(4, -(-len(v) // 4) * 4)), fill, F)
    Z[0, :len(v)] = v
    return Z


def only(Z, i):
    """the walked plane with pixel i of row 0 alone"""
    out = np.full(Z.shape, NAN, F)
    out[0, i] = Z[0, i]
    return out


# ---- ordered pairs: covisibility and the mask warp ------------------------------------------------------------------------------------

class Pair:
    """a, b: (Z, K), a is walked and b is looked up.  Ta, Tb: the poses (camera -> world).  opt: near_z, depth_sigmas.
    classes: the expected outcome of every pixel of a's row 0 up to the case's width (-1: no depth).  prove(info) asserts from
    covis_ref's info that the case hits its boundary.  single_T: Tb is the identity and Ta finite, so Ta is also the one
    transformation (a's camera -> b's camera) that the warp takes; identity: both are."""

    def __init__(self, name, a, b, classes, prove, Ta=None, Tb=None, opt=None):
        self.name, self.a, self.b, self.classes, self.prove = name, a, b, list(classes), prove
        self.identity = Ta is None and Tb is None
        self.single_T = Tb is None
        self.Ta, self.Tb = np.eye(4) if Ta is None else Ta, np.eye(4) if Tb is None else Tb
        self.opt = dict(opt or {})

    def __repr__(self):
        return self.name


def pair_cases():
    out = []
    # the near plane: qz exactly near_z, one ulp below, one ulp above
    near = F(0.75)

    def prove_near(i):
        assert bits(i["qz"][0, 0]) == bits(near) and i["qz"][0, 1] == below(near) and i["qz"][0, 2] == above(near)

    out.append(Pair("near", (embed([near, below(near), above(near), NAN]), ROW_K), (embed([near] * 4, near), ROW_K),
                    [CONSISTENT, BEHIND, CONSISTENT, -1], prove_near, opt=dict(near_z=near)))
    # half-up rounding: one pixel on the optical axis, q = (0, 0, 2), so the projection is b's principal point exactly
    full = np.full((2, 4), 2.0, F)
    for axis, last in (("u", 3), ("v", 1)):
        for k, (o, want_p, want) in enumerate(((F(-0.5), 0, CONSISTENT), (below(-0.5), -1, OUTSIDE),
                                               (F(last + 0.5), last + 1, OUTSIDE), (below(last + 0.5), last, CONSISTENT))):
            def prove_half(i, axis=axis, o=o, want_p=want_p):
                assert bits(i["proj_" + axis][0, 0]) == bits(o) and i["p" + axis][0, 0] == want_p
                assert i["proj_" + ("v" if axis == "u" else "u")][0, 0] == 0

            Kb = (5, 5, o, 0) if axis == "u" else (5, 5, 0, o)
            out.append(Pair(f"half_up_{axis}{k}", (embed([2.0]), AXIS_K), (full, Kb), [want], prove_half))
    # Round-half-to-even (rintf) agrees with floorf(p + 0.5f) on all eight halves above: -0.5 goes to -0, which passes >= 0, and
    # w - 0.5 goes up to the even w.  It differs where the lower neighbour is even: 0.5 -> 0 and 2.5 -> 2, not 1 and 3.  Inside the
    # image the pixel it would pick is a NaN of b; at the last row of a plane of odd height, 2.5 is outside and rintf's 2 is not.
    tall = np.full((3, 4), 2.0, F)
    for axis, k, o, Zb, hole, want_p, want in (("u", 4, F(0.5), full, (0, 0), 1, CONSISTENT), ("u", 5, F(2.5), full, (0, 2), 3, CONSISTENT),
                                                ("v", 4, F(0.5), full, (0, 0), 1, CONSISTENT), ("v", 5, F(2.5), tall, None, 3, OUTSIDE),
                                                ("v", 6, below(2.5), tall, None, 2, CONSISTENT)):
        Zb = Zb.copy()
        if hole:
            Zb[hole] = NAN

        def prove_even(i, axis=axis, o=o, want_p=want_p, Zb=Zb, hole=hole):
            assert bits(i["proj_" + axis][0, 0]) == bits(o) and i["p" + axis][0, 0] == want_p
            assert i["p" + ("v" if axis == "u" else "u")][0, 0] == 0
            if o - np.floor(o) != F(0.5):
                return                                                                        # (the neighbour one ulp below a half)
            even = int(np.rint(o))
            assert even == want_p - 1                                                         # half-to-even picks the pixel below:
            if hole:
                assert hole == ((0, even) if axis == "u" else (even, 0)) and np.isnan(Zb[hole])   # a NaN of b,
            else:
                assert even == Zb.shape[0] - 1 and want_p == Zb.shape[0]                      # or b's last row, where p is outside

        Kb = (5, 5, o, 0) if axis == "u" else (5, 5, 0, o)
        out.append(Pair(f"half_up_{axis}{k}", (embed([2.0]), AXIS_K), (Zb, Kb), [want], prove_even))
    # the depth tolerance: tol exactly 0.25, d == tol, d == -tol and their neighbours one ulp either side
    qz, sig = _exact_tolerance()
    tol = F(0.25)
    hi, lo = qz + tol, qz - tol
    zb = [hi, above(hi), below(hi), lo, below(lo), above(lo)]

    def prove_tol(i):
        d = i["d"][0]
        assert list(i["pu"][0, :6]) == list(range(6)) and (i["qz"][0, :6] == qz).all() and (i["tol"][0, :6] == tol).all()
        assert hi - qz == tol and lo - qz == -tol                                             # exact in float32
        # (the neighbours are one ulp of zb away: the nearest values of d that a depth plane can give)
        assert d[0] == tol and d[1] > tol and 0 < d[2] < tol and d[3] == -tol and d[4] < -tol and -tol < d[5] < 0

    out.append(Pair("tolerance", (embed([qz] * 6), ROW_K), (embed(zb, qz), ROW_K),
                    [CONSISTENT, SEEN_THROUGH, CONSISTENT, CONSISTENT, OCCLUDED, CONSISTENT], prove_tol, opt=dict(depth_sigmas=sig)))
    # a NaN of b under a finite pixel of a
    out.append(Pair("nan_in_b", (embed([1, 1, 1, 1]), ROW_K), (embed([1, NAN, 1, NAN], 1), ROW_K),
                    [CONSISTENT, NO_DEPTH, CONSISTENT, NO_DEPTH], lambda i: None))
    # a translation of 1e30 across the view and backwards along it
    for axis, sign in ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0), (2, -1.0)):
        far = np.eye(4)
        far[axis, 3] = sign * 1e30
        there = [0, 1, 3]

        def prove_far(i, axis=axis, sign=sign, there=there):
            if axis == 2:
                assert (i["qz"][0, there] <= -1e29).all()
            else:
                p = i["pu" if axis == 0 else "pv"][0, there]
                assert np.isfinite(p).all() and (sign * p >= 1e29).all()                      # far beyond any int

        want = BEHIND if axis == 2 else OUTSIDE
        out.append(Pair(f"far_{'xyz'[axis]}{'+' if sign > 0 else '-'}", (embed([1, 1, NAN, 2]), ROW_K), (embed([1] * 4, 1), ROW_K),
                        [want, want, -1, want], prove_far, Ta=far))
    # two finite poses whose relative transform is not: 1e200 * 1e200 - 1e200 * 1e200 in the translation of row 0
    A, B = np.eye(4), np.eye(4)
    A[0, 3], B[0, 0], B[0, 3] = 1e200, 1e200, 1e200

    def prove_nan_T(i):
        assert np.isfinite(A).all() and np.isfinite(B).all() and np.isnan(i["T"][0, 3]) and np.isfinite(i["T"][2]).all()
        assert np.isnan(i["pu"][0, [0, 1, 3]]).all() and (i["qz"][0, [0, 1, 3]] >= F(0.1)).all()

    out.append(Pair("nan_transform", (embed([1, 1, NAN, 2]), ROW_K), (embed([1] * 4, 1), ROW_K), [OUTSIDE, OUTSIDE, -1, OUTSIDE],
                    prove_nan_T, Ta=A, Tb=B))
    # depths that are no distance: in a, an infinity is no depth, zero and a negative depth are behind
    def prove_special_a(i):
        assert i["qz"][0, 2] == 0 and i["qz"][0, 3] == F(-1.5) and i["valid"] == 2

    out.append(Pair("special_in_a", (embed([np.inf, -np.inf, 0, -1.5]), ROW_K), (embed([1] * 4, 1), ROW_K), [-1, -1, BEHIND, BEHIND],
                    prove_special_a))
    # ... in b, only a NaN is no depth: every other value is classed by d
    def prove_special_b(i):
        assert list(i["d"][0]) == [np.inf, -np.inf, -1, -2.5]

    out.append(Pair("special_in_b", (embed([1] * 4), ROW_K), (embed([np.inf, -np.inf, 0, -1.5], 1), ROW_K),
                    [SEEN_THROUGH, OCCLUDED, OCCLUDED, OCCLUDED], prove_special_b))
    return out


# a of exactly one chunk of k_covis (kChunk = 1024 pixels) and of one chunk and four pixels (4 x 257): (name, (h, w), the pixels
# of a that carry a depth).  The rays of a are all but parallel (fx = fy = 1e6), so every pixel comes back to column 2 of b's row 0.
CHUNK_K = (1e6, 1e6, 0, 0)
CHUNK_CASES = [("1024_last", (4, 256), [1023]), ("1028_last", (257, 4), [1027]), ("1028_chunk_edge", (257, 4), [1023, 1024]),
               ("1028_first_and_last", (257, 4), [0, 1027])]


def chunk_plane(shape, pixels):
    Z = np.full(shape, NAN, F)
    Z.reshape(-1)[pixels] = 1.0
    return Z


# ---- depth fusion ---------------------------------------------------------------------------------------------------------------------

class Fuse:
    """key: (Z, K); frames: [(Z, K)]; Ts[k]: frame k's camera -> the keyframe's; opt: the options but the sample; samples: the
    samples the case is for.  prove(sample, out, info) asserts from fuse_ref's results that the case hits its boundary."""

    def __init__(self, name, key, frames, Ts, opt, samples, prove):
        self.name, self.key, self.frames, self.Ts, self.opt, self.samples, self.prove = name, key, frames, Ts, opt, samples, prove

    def __repr__(self):
        return self.name

    def ref(self, sample, info=None):
        return fuse.fuse_ref(self.key, self.frames, self.Ts, dict(self.opt, sample=sample), info=info)


BOTH = (fuse.BILINEAR, fuse.NEAREST)
# what the bilinear sample makes of the pairs it shares: the projections are whole numbers, a = b = 0 and the sample is z00 -- but
# all four corners must be there, and column w - 1 has no window
BILINEAR_CLASSES = {"near": [CONSISTENT, BEHIND, CONSISTENT, -1], "nan_in_b": [NO_DEPTH, NO_DEPTH, NO_DEPTH, OUTSIDE],
                    "tolerance": [CONSISTENT, SEEN_THROUGH, CONSISTENT, CONSISTENT, OCCLUDED, CONSISTENT]}


def y_rotation(deg):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    return T


def _classes(info, n):
    return [int(c) for c in info["cls"][0, :n]]


def fuse_cases():
    out = []
    # the pairs at the identity: the keyframe is walked, the frame is looked up
    for p in pair_cases():
        if not p.identity or p.name.startswith("special"):
            continue
        samples = BOTH if p.name in BILINEAR_CLASSES else (fuse.NEAREST,)

        def prove_pair(sample, res, info, p=p):
            want = p.classes if sample == fuse.NEAREST else BILINEAR_CLASSES[p.name]
            i = info[0]
            if sample == fuse.BILINEAR:
                there = np.isfinite(p.a[0][0])
                assert (i["px"][0, there] == np.floor(i["px"][0, there])).all() and (i["py"][0, there] == 0).all()
            assert _classes(i, len(want)) == want
            assert np.array_equal(res[1][0, :len(want)], [int(c == CONSISTENT) for c in want]) and res[1].sum() == want.count(CONSISTENT)

        out.append(Fuse("pair_" + p.name, p.a, [p.b], [np.eye(4)], dict(dict(depth_sigmas=20.0), **p.opt), samples, prove_pair))
    # the bilinear window of floorf(px): one pixel on the optical axis, the projection is the frame's principal point exactly
    key = (embed([2.0]), AXIS_K)
    Zf = np.full((3, 4), 2.0, F)
    tiny, small = below(0), F(-2.0 ** -126)                  # one ulp below zero (subnormal), and the largest normal below it
    for axis, last in (("x", 3), ("y", 2)):
        for k, (o, want0, want) in enumerate(((F(0), 0, CONSISTENT), (tiny, -1, OUTSIDE), (small, -1, OUTSIDE),
                                              (F(last), last, OUTSIDE), (below(last), last - 1, CONSISTENT))):
            def prove_window(sample, res, info, axis=axis, o=o, want0=want0, want=want):
                i = info[0]
                assert bits(i["p" + axis][0, 0]) == bits(o) and np.floor(i["p" + axis][0, 0]) == want0 and i["cls"][0, 0] == want
                assert res[2][0]["valid"] == 1 and res[2][0]["fused"] == int(want == CONSISTENT)

            Kf = (5, 5, o, 0.5) if axis == "x" else (5, 5, 1.5, o)
            out.append(Fuse(f"window_{axis}{k}", key, [(Zf, Kf)], [np.eye(4)], {}, (fuse.BILINEAR,), prove_window))
    # a NaN in each corner of the window in turn; and the window alone
    corners = [(0, 1), (0, 2), (1, 1), (1, 2)]               # (row, column) of z00, z10, z01, z11 for px = 1.25, py = 0.5
    planes = [(f"corner{k}", (r, c)) for k, (r, c) in enumerate(corners)] + [("corners_alone", None), ("corners_all", ())]
    for name, hole in planes:
        Z = Zf.copy()
        if hole is None:
            Z[:] = NAN
            for r, c in corners:
                Z[r, c] = 2.0
        elif hole:
            Z[hole] = NAN
        want = NO_DEPTH if hole else CONSISTENT

        def prove_corner(sample, res, info, want=want):
            i = info[0]
            assert i["px"][0, 0] == F(1.25) and i["py"][0, 0] == F(0.5) and i["cls"][0, 0] == want
            assert res[2][0]["fused"] == int(want == CONSISTENT)

        out.append(Fuse(name, key, [(Z, (5, 5, 1.25, 0.5))], [np.eye(4)], {}, (fuse.BILINEAR,), prove_corner))
    # min_cos is inclusive: a frame turned by 60 degrees about y; c of the one pixel (tx = 0.25, ty = 0) is a known float
    T = y_rotation(60.0)
    key_c = (embed([NAN, 2.0]), (4, 4, 0, 0))
    Kf = (0.5, 0.5, 1.5, 0.5)
    probe = []
    fuse.fuse_ref(key_c, [(np.full((2, 4), 1.0, F), Kf)], [T], info=probe)
    qz = probe[0]["qz"][0, 1]                               # the frame sees the point at exactly this depth: d == 0
    M = fuse.inverse_rows(T)
    c_known = F(F(F(M[2, 0] * F(0.25)) + F(M[2, 1] * F(0))) + M[2, 2])
    assert 0.7 < c_known < 0.72 and F(1.4) < qz < F(1.5)
    for name, min_cos, fused in (("min_cos_at", c_known, 1), ("min_cos_above", above(c_known), 0)):
        def prove_cos(sample, res, info, min_cos=min_cos, fused=fused):
            i = info[0]
            assert bits(i["c"][0, 1]) == bits(c_known) and i["d"][0, 1] == 0 and i["cls"][0, 1] == CONSISTENT
            assert (i["c"][0, 1] >= min_cos) == bool(fused)
            assert res[2][0]["consistent"] == 1 and res[2][0]["fused"] == fused and res[1][0, 1] == fused

        out.append(Fuse(name, key_c, [(np.full((2, 4), qz, F), Kf)], [T], dict(min_cos=min_cos), BOTH, prove_cos))
    # min_observations: n copies of one agreeing frame
    n = 3
    key_n = (embed([1, 1.5, NAN, 2, NAN]), ROW_K)
    frame = (embed([1, 1.5, 1.75, 2, 2.5], 1), ROW_K)
    for min_obs in (n, n + 1):
        for drop in (0, 1):
            def prove_obs(sample, res, info, min_obs=min_obs, drop=drop):
                has = np.isfinite(key_n[0])
                assert has.sum() == 3 and (res[1][has] == n).all() and not res[1][~has].any()
                confirmed = min_obs <= n
                assert res[3] == dict(with_depth=3, confirmed=3 * confirmed, unconfirmed_kept=3 * (not confirmed and not drop),
                                      unconfirmed_dropped=3 * (not confirmed and bool(drop)))
                assert np.array_equal(np.isfinite(res[0]), has & (confirmed or not drop))

            out.append(Fuse(f"min_observations_{min_obs}_drop{drop}", key_n, [frame] * n, [np.eye(4)] * n,
                            dict(min_observations=min_obs, drop_unconfirmed=drop), BOTH, prove_obs))
    # the convention on a case whose arithmetic is exact (test_depth_fusion.py: test_the_convention_on_an_exact_case)
    w, h = 24, 12
    K = (64.0, 64.0, 11.0, 5.0)
    Z0, Zk = np.full((h, w), 2.0, F), np.full((h, w), 1.0, F)
    T = np.eye(4)
    T[2, 3] = 1.0

    def prove_convention(sample, res, info):
        u, v = np.meshgrid(np.arange(w), np.arange(h))
        last = 1 if sample == fuse.NEAREST else 2
        inside = (2 * (u - 11) + 11 >= 0) & (2 * (u - 11) + 11 <= w - last) & (2 * (v - 5) + 5 >= 0) & (2 * (v - 5) + 5 <= h - last)
        assert np.array_equal(res[0], Z0) and np.array_equal(res[1], inside.astype(np.uint8)) and 0 < inside.sum() < w * h
        assert res[2][0]["fused"] == res[2][0]["consistent"] == int(inside.sum())

    def prove_inverse(sample, res, info):
        assert not res[1].any() and res[2][0]["consistent"] == res[2][0]["fused"] == 0 and res[2][0]["occluded"] > 0

    out.append(Fuse("convention", (Z0, K), [(Zk, K)], [T], {}, BOTH, prove_convention))
    out.append(Fuse("convention_inverse", (Z0, K), [(Zk, K)], [np.linalg.inv(T)], {}, BOTH, prove_inverse))
    return out


# ---- the renderer ---------------------------------------------------------------------------------------------------------------------

class Render:
    """keyframes: [(I, Z, K, pose)] inserted with the ids 0, 1, ...; orders: the insertion orders the map is built in (the planes
    must not depend on it); views: [(label, pose, K, width, height, near)]; prove(label, xyz, ref, brute) asserts on the extract
    and the two restatements' results of a view that the view hits its case."""

    def __init__(self, name, leaf, keyframes, views, prove, orders=None):
        self.name, self.leaf, self.keyframes, self.views, self.prove = name, leaf, keyframes, views, prove
        self.orders = orders or [list(range(len(keyframes)))]

    def __repr__(self):
        return self.name

    def extract(self):
        """what KeyframeMap.extract() returns for these keyframes (test_map_cloud.py holds the device to it)"""
        clouds = [cloud_ref(Z, I, K, pose) for I, Z, K, pose in self.keyframes]
        xyz = np.concatenate([c[0].reshape(-1, 3) for c in clouds])
        rgb = np.concatenate([c[1].reshape(-1) for c in clouds])
        return voxel_ref(xyz, rgb, self.leaf)[:2]


def _grey(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(F)


def _at(x=0.0, y=0.0, z=0.0):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def _one_voxel(z):
    return (_grey((2, 4), 1), embed([z]), AXIS_K, np.eye(4))


WALL_K = (64.0, 64.0, 8.0, 0.0)
WALL_LEAF = 1.0 / 32                                        # two pixel pitches of the wall at z = 1
WALL_HOLES = [(2, 5), (10, 13)]                             # the first column of one cell and the second of the next
WALL_PAIRS = [(3, 4), (11, 12)]                             # ... leave the two centroids on these columns, one pitch apart


def _wall_keyframes():
    """a fronto-parallel wall of 16 x 2 pixels at z = 1 seen from the identity, its pixels dealt out to three keyframes"""
    u, v = np.meshgrid(np.arange(16), np.arange(2))
    wall = np.ones((2, 16), F)
    for a, b in WALL_HOLES:
        wall[:, a] = wall[:, b] = NAN
    return [(_grey((2, 16), 10 + j), np.where((u + v) % 3 == j, wall, F(NAN)).astype(F), WALL_K, np.eye(4)) for j in range(3)]


def render_cases():
    out = []
    # ties: all voxels of the wall have cz == 1 exactly; the footprints are two pitches wide
    def prove_ties(label, xyz, ref, brute):
        assert (xyz[:, 2] == 1).all() and len(xyz) == 8
        if label != "identity":
            return
        assert brute["info"]["ties"] >= len(WALL_PAIRS)
        for a, b in WALL_PAIRS:
            left = np.flatnonzero(xyz[:, 0] == F((a - 8) / 64))
            right = np.flatnonzero(xyz[:, 0] == F((b - 8) / 64))
            assert len(left) == len(right) == 1 and left[0] < right[0]
            assert (ref["info"]["candidates"][:, [a, b]] == 2).all()                      # both footprints, nothing else
            assert (ref["index"][:, [a, b]] == left[0]).all() and (ref["depth"][:, [a, b]] == 1).all()

    far = [(f"far_{'xyz'[axis]}{'+' if sign > 0 else '-'}", _at(**{"xyz"[axis]: sign * 1e30}), WALL_K, 16, 2, None)
           for axis, sign in ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0), (2, 1.0))]
    wall = _wall_keyframes()

    def prove_wall(label, xyz, ref, brute):
        prove_ties(label, xyz, ref, brute)
        if label.startswith("far"):
            st = ref["stats"]
            assert st["drawn"] == st["covered_pixels"] == 0 and st["behind_near"] + st["outside"] == st["voxels"] == 8
            assert (st["behind_near"] if label == "far_z+" else st["outside"]) == 8
            assert (ref["index"] == -1).all() and np.isnan(ref["depth"]).all()

    out.append(Render("wall", WALL_LEAF, wall, [("identity", None, WALL_K, 16, 2, None)] + far, prove_wall,
                      orders=[[0, 1, 2], [2, 0, 1], [1, 2, 0]]))
    # the near plane: near_z equal to a voxel's z, then one ulp above it
    second = (_grey((2, 4), 20), np.full((2, 4), 1.5, F), WALL_K, _at(y=0.25))
    nears = [F(1.0), above(1.0), F(1.5), above(1.5)]

    def prove_near(label, xyz, ref, brute):
        n1, n15 = int((xyz[:, 2] == 1).sum()), int((xyz[:, 2] == F(1.5)).sum())
        assert n1 == 8 and n15 >= 1 and n1 + n15 == len(xyz)
        assert ref["stats"]["behind_near"] == {"near0": 0, "near1": n1, "near2": n1, "near3": n1 + n15}[label]
        assert ref["stats"]["drawn"] == len(xyz) - ref["stats"]["behind_near"]

    out.append(Render("near", WALL_LEAF, wall + [second], [(f"near{k}", None, WALL_K, 16, 16, near) for k, near in enumerate(nears)],
                      prove_near))
    # one voxel at (0, 0, 1), four pixels wide: cut by each border and by a corner, and wholly off each side
    K = lambda ox, oy: (40.0, 40.0, ox, oy)  # noqa: E731
    cut = {"left": K(-1.5, 8), "right": K(33.5, 8), "top": K(16, -1.5), "bottom": K(16, 17.5), "corner": K(-1, -1)}
    off = {"off_left": K(-3, 8), "off_right": K(36, 8), "off_top": K(16, -3), "off_bottom": K(16, 20)}

    def prove_border(label, xyz, ref, brute):
        assert len(xyz) == 1 and list(xyz[0]) == [0, 0, 1]
        if label in cut:
            assert ref["info"]["clamped"] == 1 and ref["stats"]["drawn"] == 1 and 0 < ref["stats"]["covered_pixels"] < 25
        else:
            assert ref["stats"]["outside"] == 1 and ref["stats"]["drawn"] == ref["stats"]["covered_pixels"] == 0

    out.append(Render("borders", 0.1, [_one_voxel(1.0)], [(label, None, Kv, 33, 17, None) for label, Kv in {**cut, **off}.items()],
                      prove_border))
    # a footprint of 0.2 pixels that contains no pixel centre: the nearest pixel
    # (at 16.5, 8.5 the nearest pixel is floorf(c + 0.5f)'s (17, 9); round-half-to-even would take (16, 8))
    def prove_fallback(label, xyz, ref, brute):
        assert len(xyz) == 1 and list(xyz[0]) == [0, 0, 2]
        at = (8, 16) if label == "fallback" else (9, 17)
        assert ref["info"]["fallback"] == 1 and ref["stats"]["covered_pixels"] == 1 and ref["index"][at] == 0

    out.append(Render("fallback", 0.01, [_one_voxel(2.0)], [("fallback", None, (40.0, 40.0, 16.3, 8.1), 33, 17, None),
                                                             ("fallback_half", None, (40.0, 40.0, 16.5, 8.5), 33, 17, None)], prove_fallback))
    # footprints of 4 (2 x 2 and 1 x 4), 5 and 6 pixels in one wave: a lane splats up to 4 pixels itself, the wave walks the rest
    spots = {"2x2": ((4.5, 2.5, 2.0), (2, 2)), "1x4": ((12.5, -2.0, 0.5), (1, 4)), "1x5": ((20.0, -2.0, 0.5), (1, 5)),
             "2x3": ((27.0, 4.5, 1.0), (2, 3))}             # (u, v, z) of the centroid in the view, (rows, columns) covered
    kfs, world = [], {}
    for name, ((u, v, z), _) in spots.items():
        world[name] = (F(u * z / 64), F(v * z / 64), F(z))
        kfs.append((_grey((2, 4), 30 + len(kfs)), embed([1.0]), AXIS_K, _at(float(world[name][0]), float(world[name][1]), z - 1.0)))

    def prove_sizes(label, xyz, ref, brute):
        assert len(xyz) == 4 and ref["stats"]["drawn"] == 4 and ref["info"]["multi"] == 0
        for name, (_, (rows, cols)) in spots.items():
            r = np.flatnonzero((xyz == np.array(world[name], F)).all(axis=1))
            assert len(r) == 1, name
            ys, xs = np.nonzero(ref["index"] == r[0])
            assert len(ys) == rows * cols and ys.max() - ys.min() + 1 == rows and xs.max() - xs.min() + 1 == cols, name

    out.append(Render("footprints", WALL_LEAF, kfs, [("sizes", None, (64.0, 64.0, 0.0, 0.0), 32, 8, None)], prove_sizes))
    return out


def view_near(case, K, near):
    return default_near(case.leaf, K) if near is None else near
