"""The keyframe map kept on the device (dvo_amd.h: dvo_amd_map_create / _insert / _set_poses / _remove / _stats / _extract).

The contract is an equality: after any sequence of operations the map equals one dvo_amd_map_cloud over the keyframes it holds,
bit for bit.  The oracle is the one of tests/test_map_cloud.py (cloud_ref, voxel_ref, voxel_brute, same_bits); there is no
tolerance anywhere in this file.
CPU: a numpy restatement of the incremental store (a dict from key to Python-int sums reduced modulo 2^64, contributions added
and subtracted keyframe by keyframe) equals voxel_ref from scratch after every operation of a random sequence, a wrapped sum
included; the box rule; without a GPU every entry fails loudly.
GPU: the library against DenseTracker.map_cloud over the current set."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_map_cloud import BIAS, FIX, random_cloud, same_bits, voxel_brute, voxel_ref  # noqa: E402

M64 = (1 << 64) - 1


# ---- the restatement of the incremental store -----------------------------------------------------------------------------------

def repose(xyz, pose):
    """cloud_ref's transform on given points: T = (float)pose, ((T0 x + T1 y) + T2 z) + T3, every operation rounded in fp32"""
    T = np.asarray(pose, dtype=np.float64).astype(np.float32)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.empty_like(xyz)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            out[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out


def _signed(v):
    return v - (1 << 64) if v >> 63 else v


class StoreRef:
    """key -> [count, sx, sy, sz, r, g, b], every entry reduced modulo 2^64 like the device's; totals as plain integers"""

    def __init__(self, leaf):
        self.leaf, self.vox = leaf, {}
        self.points_in = self.finite = self.out_of_range = 0
        self.wrapped = False  # a coordinate sum left the int64 range at some point

    def apply(self, xyz, rgb, sign):
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        rgb = np.asarray(rgb, np.uint32).reshape(-1)
        finite = np.isfinite(xyz).all(axis=1)
        inv = np.float32(1.0) / np.float32(self.leaf)
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.floor(xyz * inv)
            inr = finite & ((f >= -BIAS) & (f < BIAS)).all(axis=1)
        self.points_in += sign * len(xyz)
        self.finite += sign * int(finite.sum())
        self.out_of_range += sign * int(finite.sum() - inr.sum())
        idx = f[inr].astype(np.int64) + BIAS
        keys = ((idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]).tolist()
        q = np.rint(xyz[inr].astype(np.float64) * FIX).astype(np.int64).tolist()
        c = rgb[inr].tolist()
        for k, (qx, qy, qz), col in zip(keys, q, c):
            e = self.vox.setdefault(k, [0] * 7)
            d = [1, qx, qy, qz, (col >> 16) & 0xFF, (col >> 8) & 0xFF, col & 0xFF]
            for a in range(7):
                if 1 <= a <= 3 and not -(1 << 63) <= _signed(e[a]) + sign * d[a] < (1 << 63):
                    self.wrapped = True
                e[a] = (e[a] + sign * d[a]) & M64
            if e[0] == 0:
                assert not any(e), "a voxel without points has sums left"
                del self.vox[k]

    def extract(self, box=None):
        keys = sorted(self.vox)
        xyz = np.zeros((len(keys), 3), np.float32)
        rgb = np.zeros(len(keys), np.uint32)
        for n, k in enumerate(keys):
            e = self.vox[k]
            s = np.array([_signed(v) for v in e[1:4]], np.int64)
            xyz[n] = (s.astype(np.float64) / (np.float64(e[0]) * FIX)).astype(np.float32)
            ch = [(v + e[0] // 2) // e[0] for v in e[4:7]]
            rgb[n] = (ch[0] << 16) | (ch[1] << 8) | ch[2]
        if box is not None:
            keep = in_box(xyz, box)
            xyz, rgb = xyz[keep], rgb[keep]
        return xyz, rgb

    def stats(self):
        return {"points_in": self.points_in, "finite": self.finite, "out_of_range": self.out_of_range, "voxels": len(self.vox)}


def in_box(xyz, box):
    """the header's box rule: min <= c < max on all three axes, in fp32"""
    b = np.asarray(box, np.float32)
    return ((xyz >= b[None, :3]) & (xyz < b[None, 3:])).all(axis=1)


def _from_scratch(clouds, leaf):
    if not clouds:
        return voxel_ref(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), leaf)
    return voxel_ref(np.concatenate([c[0] for c in clouds]), np.concatenate([c[1] for c in clouds]), leaf)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------

def test_incremental_store_equals_from_scratch(synth):
    leaf = 4096.0  # large enough for a coordinate sum to pass 2^63: q = x * 2^24 with x up to 2^20 * leaf
    scale = np.float32(leaf / 0.05)
    rng = np.random.default_rng(41)
    clouds = []
    for _ in range(6):
        xyz, rgb = random_cloud(rng, 400, 0.05)
        with np.errstate(over="ignore", invalid="ignore"):
            clouds.append(((xyz * scale).astype(np.float32), rgb))
    # one voxel pushed past 2^63 by construction: 160 equal points in the middle of a voxel at x = 0.9 * 2^32 m,
    # 160 * 0.9 * 2^56 = 1.125 * 2^63
    far = np.tile(np.array([[(int(0.9 * BIAS) + 0.5) * leaf, 100.0, -300.0]], np.float32), (160, 1))
    clouds[0] = (np.concatenate([clouds[0][0], far]), np.concatenate([clouds[0][1], np.full(160, 0x102030, np.uint32)]))

    def pose():
        return synth.se3_exp(np.r_[rng.normal(scale=3000.0, size=3), rng.normal(scale=0.02, size=3)])

    store, cur = StoreRef(leaf), {}  # cur: id -> pose
    posed = lambda k: (repose(clouds[k][0], cur[k]), clouds[k][1])  # noqa: E731
    kinds = {"insert": 0, "move": 0, "remove": 0}
    for step in range(40):
        absent = [k for k in range(6) if k not in cur]
        kind = rng.choice([k for k, ok in (("insert", absent), ("move", cur), ("remove", len(cur) > 1 or step > 30)) if ok])
        if kind == "insert":
            k = int(rng.choice(absent))
            cur[k] = np.eye(4) if step == 0 else pose()
            store.apply(*posed(k), +1)
        elif kind == "move":
            k = int(rng.choice(sorted(cur)))
            store.apply(*posed(k), -1)
            cur[k] = pose()
            store.apply(*posed(k), +1)
        else:
            k = int(rng.choice(sorted(cur)))
            store.apply(*posed(k), -1)
            del cur[k]
        kinds[kind] += 1
        rx, rr, rst = _from_scratch([posed(k) for k in sorted(cur)], leaf)
        xyz, rgb = store.extract()
        assert store.stats() == rst, (step, kind)
        assert same_bits(xyz, rx) and same_bits(rgb, rr), (step, kind)
    assert all(v >= 5 for v in kinds.values()), kinds
    assert store.wrapped  # the wrap was exercised (voxel_ref's int64 sums wrap the same way)
    for k in sorted(cur):
        store.apply(*posed(k), -1)
    assert store.vox == {} and store.stats() == {"points_in": 0, "finite": 0, "out_of_range": 0, "voxels": 0}


def test_incremental_store_against_brute_force_and_box_rule():
    leaf = 0.05
    rng = np.random.default_rng(43)
    a, b = random_cloud(rng, 1500, leaf), random_cloud(rng, 1500, leaf)
    store = StoreRef(leaf)
    store.apply(*a, +1), store.apply(*b, +1), store.apply(*a, -1)
    bx, br, bst = voxel_brute(*b, leaf)
    xyz, rgb = store.extract()
    assert same_bits(xyz, bx) and same_bits(rgb, br) and {k: store.stats()[k] for k in bst} == bst
    lo, hi = np.float32(xyz[:, 0].min()), np.float32(xyz[:, 0].max())
    boxes = [(-0.1, -0.1, -0.1, 0.1, 0.1, 0.1), (-9, -9, 0.0, 9, 9, 9), (5, 5, 5, 6, 6, 6),
             (lo, -9, -9, hi, 9, 9)]  # the last: the minimum is inside (<=), the maximum is outside (<)
    counts = []
    for box in boxes:
        fx, fr = store.extract(box)
        keep = np.array([all(np.float32(box[a]) <= p[a] < np.float32(box[a + 3]) for a in range(3)) for p in xyz], bool)
        assert same_bits(fx, xyz[keep]) and same_bits(fr, rgb[keep])
        counts.append(int(keep.sum()))
    assert 0 < counts[0] < counts[1] < len(xyz) and counts[2] == 0
    assert counts[3] == len(xyz) - int((xyz[:, 0] == hi).sum()) and (xyz[:, 0] == lo).any()


def test_keyframe_map_entries_fail_loudly_without_a_gpu():
    from dvo_slam_amd import capi

    L = capi.lib()
    if L.dvo_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    h, n, st, nk = C.c_void_p(), C.c_longlong(), capi.CCloudStats(), C.c_int()
    ids = (C.c_int * 1)(0)
    pose = np.eye(4).ravel()
    pts = np.zeros((4, 4), np.float32)
    dp = pose.ctypes.data_as(C.POINTER(C.c_double))
    assert L.dvo_amd_map_create(None, 0.01, C.byref(h)) == 2 and not h.value
    assert L.dvo_amd_map_insert(None, 0, None, dp, None, 0) == 2
    assert L.dvo_amd_map_set_poses(None, 1, ids, dp) == 2
    assert L.dvo_amd_map_remove(None, 1, ids) == 2
    assert L.dvo_amd_map_stats(None, C.byref(st), C.byref(nk)) == 2
    assert L.dvo_amd_map_extract(None, None, pts.ctypes.data, 4, C.byref(n)) == 2
    d = C.c_double()
    assert L.dvo_amd_debug_keyframe_map_timing(None, C.byref(d), None, None, None, None) == 2
    L.dvo_amd_map_destroy(None)  # a null map is nothing to destroy
    with pytest.raises(capi.DvoAmdError) as e:
        capi.KeyframeMap(type("T", (), {"_h": None})())
    assert e.value.status == 2


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

LEAF = 0.02


@pytest.fixture(scope="module")
def capi_gpu():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


def _step_pose(synth, k, scale=1.0):
    return synth.se3_exp(np.array([0.02 * k, -0.01 * k, 0.015 * k, 0.01 * k, -0.02 * k, 0.005 * k]) * scale)


def _keyframe(capi, synth, w, h, k):
    """(1-level pyramid, BGR image or None) of the view from the k-th pose of a slow sweep"""
    I, Z = synth.render(w, h, _step_pose(synth, k), frame_id=k)
    bgr, raw = synth.to_raw(I, Z)
    return capi.RgbdImagePyramid.from_raw(bgr, raw, synth.intrinsics_for(w, h), 1), (bgr if k % 2 == 0 else None)


@pytest.fixture(scope="module")
def frames(capi_gpu, synth):
    """8 keyframes of 160x120 along small pose steps (the views overlap), a BGR image on every other one"""
    kfs = [_keyframe(capi_gpu, synth, 160, 120, k) for k in range(8)]
    return [p for p, _ in kfs], [_step_pose(synth, k) for k in range(8)], [b for _, b in kfs]


def _rebuild(trk, frames, cur, leaf=LEAF):
    """map_cloud over the current set: cur maps id -> (frame index, pose)"""
    pyrs, _, bgrs = frames
    ids = sorted(cur)
    return trk.map_cloud([pyrs[cur[i][0]] for i in ids], [cur[i][1] for i in ids], [bgrs[cur[i][0]] for i in ids], leaf=leaf)


def _assert_equal(m, ref, what=None):
    rx, rr, rst = ref
    xyz, rgb = m.extract()
    st = m.stats()
    st.pop("keyframes")
    assert st == rst, (what, st, rst)
    assert same_bits(xyz, rx) and same_bits(rgb, rr), what


@pytest.mark.gpu
def test_growth(capi_gpu, frames):
    pyrs, poses, bgrs = frames
    trk = capi_gpu.DenseTracker()
    m = capi_gpu.KeyframeMap(trk, LEAF)
    _assert_equal(m, _rebuild(trk, frames, {}), "empty")
    cur, singles = {}, 0
    for k in range(8):
        m.insert(k, pyrs[k], poses[k], bgrs[k])
        cur[k] = (k, poses[k])
        _assert_equal(m, _rebuild(trk, frames, cur), k)
        assert m.stats()["keyframes"] == k + 1
        singles += _rebuild(trk, frames, {k: cur[k]})[2]["voxels"]
    assert 0 < m.stats()["voxels"] < singles  # the views overlap: shared voxels were merged, not appended


@pytest.mark.gpu
def test_move(capi_gpu, synth, frames):
    pyrs, poses, bgrs = frames
    trk = capi_gpu.DenseTracker()
    m = capi_gpu.KeyframeMap(trk, LEAF)
    cur = {}
    for k in range(8):
        m.insert(k, pyrs[k], poses[k], bgrs[k])
        cur[k] = (k, poses[k])
    original = m.extract()
    other = lambda k, s: synth.se3_exp([0.01 * s, 0.02, -0.01 * k, 0.003 * k, 0.01, -0.004 * s]) @ poses[k]  # noqa: E731
    m.set_poses([3], [other(3, 1)])                                         # one keyframe
    cur[3] = (3, other(3, 1))
    assert m.timing()[2] == 2 * 160 * 120                                   # its old and its new contribution
    _assert_equal(m, _rebuild(trk, frames, cur), "one")
    m.set_poses([1, 3, 6], [other(1, 2), cur[3][1], other(6, 2)])           # three, one of them where it already is
    cur[1], cur[6] = (1, other(1, 2)), (6, other(6, 2))
    assert m.timing()[2] == 4 * 160 * 120                                   # two moved: the third costs nothing
    _assert_equal(m, _rebuild(trk, frames, cur), "three")
    m.set_poses(list(range(8)), [other(k, 3) for k in range(8)])            # all (the rebuild rule applies)
    cur = {k: (k, other(k, 3)) for k in range(8)}
    assert m.timing()[2] == 8 * 160 * 120                                   # every keyframe once: built again from scratch
    _assert_equal(m, _rebuild(trk, frames, cur), "all")
    assert not same_bits(m.extract()[0], original[0])
    m.set_poses(list(range(8))[::-1], [poses[k] for k in range(8)][::-1])   # back: the original bits
    xyz, rgb = m.extract()
    assert same_bits(xyz, original[0]) and same_bits(rgb, original[1])
    m.set_poses([2], [poses[2]])                                            # nothing moves: nothing is done
    assert same_bits(m.extract()[0], original[0])


@pytest.mark.gpu
def test_remove(capi_gpu, frames):
    pyrs, poses, bgrs = frames
    trk = capi_gpu.DenseTracker()
    m = capi_gpu.KeyframeMap(trk, LEAF)
    cur = {}
    for k in range(6):
        m.insert(k, pyrs[k], poses[k], bgrs[k])
        cur[k] = (k, poses[k])
    shared_and_deleted = 0
    for k in (2, 0, 5, 3, 1, 4):
        before = _rebuild(trk, frames, cur)[2]["voxels"]
        alone = _rebuild(trk, frames, {k: cur[k]})[2]["voxels"]
        m.remove([k])
        del cur[k]
        ref = _rebuild(trk, frames, cur)
        _assert_equal(m, ref, k)
        after = ref[2]["voxels"]
        # after < before: voxels only k saw were deleted; before - after < alone: voxels k shared stayed, with a smaller count
        shared_and_deleted += (after < before and 0 < after and before - after < alone)
    assert shared_and_deleted >= 1
    st = m.stats()
    assert st == {"points_in": 0, "finite": 0, "out_of_range": 0, "voxels": 0, "keyframes": 0}
    xyz, rgb = m.extract()
    assert xyz.shape == (0, 3) and rgb.shape == (0,)
    m.insert(2, pyrs[2], poses[2], bgrs[2])                                # a removed id again
    m.insert(7, pyrs[7], poses[7], bgrs[7])
    _assert_equal(m, _rebuild(trk, frames, {2: (2, poses[2]), 7: (7, poses[7])}), "again")
    m.remove([7, 2])
    assert m.stats()["voxels"] == 0 and m.stats()["keyframes"] == 0


@pytest.mark.gpu
def test_history_independence(capi_gpu, synth, frames):
    pyrs, poses, bgrs = frames
    capi = capi_gpu
    ids = [0, 1, 2, 3, 4]
    final = {k: synth.se3_exp([0.01, -0.02 * k, 0.01, 0.002 * k, 0.0, 0.01]) @ poses[k] for k in ids}
    detour = {k: synth.se3_exp([0.3, 0.1 * k, -0.2, 0.05, 0.02 * k, -0.03]) for k in ids}
    t1, t2 = capi.DenseTracker(), capi.DenseTracker()
    a = capi.KeyframeMap(t1, LEAF)                                           # straight: in order, at the final poses
    for k in ids:
        a.insert(k, pyrs[k], final[k], bgrs[k])
    b = capi.KeyframeMap(t2, LEAF)                                           # reversed, elsewhere first, one batched move
    for k in ids[::-1]:
        b.insert(k, pyrs[k], detour[k], bgrs[k])
    b.insert(9, pyrs[7], poses[7], bgrs[7])
    b.remove([2])
    b.set_poses([0, 1, 3, 4], [final[k] for k in (0, 1, 3, 4)])
    b.insert(2, pyrs[2], final[2], bgrs[2])
    b.remove([9])
    c = capi.KeyframeMap(t1, LEAF)                                           # shuffled, a detour, many single moves
    for k in (3, 0, 4, 1, 2):
        c.insert(k, pyrs[k], poses[k], bgrs[k])
    for k in (4, 2, 0):
        c.set_poses([k], [detour[k]])
    for k in (1, 0, 3, 2, 4):
        c.set_poses([k], [final[k]])
    ref = _rebuild(t2, frames, {k: (k, final[k]) for k in ids})
    for m in (a, b, c):
        _assert_equal(m, ref)
    xa, ra = a.extract()
    for m in (b, c):
        x, r = m.extract()
        assert same_bits(x, xa) and same_bits(r, ra) and m.stats() == a.stats()


@pytest.mark.gpu
def test_merge_edges(capi_gpu, synth, frames):
    capi = capi_gpu
    pyrs, poses, bgrs = frames
    trk = capi.DenseTracker()
    K = synth.intrinsics_for(160, 120)
    I = np.full((120, 160), 100.0, np.float32)
    one = np.full((120, 160), np.nan, np.float32)
    one[37, 91] = 1.25
    extra = [capi.RgbdImagePyramid(I, one, K, 1), capi.RgbdImagePyramid(I, np.full((120, 160), np.nan, np.float32), K, 1),
             _keyframe(capi, synth, 352, 264, 3)[0]]
    local = (pyrs + extra, None, bgrs + [None, None, None])                  # frames 8: one pixel, 9: all NaN, 10: 352x264
    far = lambda x: synth.se3_exp([x, 0, 0, 0, 0, 0])                        # noqa: E731
    m = capi.KeyframeMap(trk, LEAF)
    cur = {}

    def step(what, fn):
        fn()
        delta_voxels = m.timing()[3]  # of the update (an extract resets the probe)
        _assert_equal(m, _rebuild(trk, local, cur), what)
        return delta_voxels

    def insert(i, f, T):
        cur[i] = (f, T)
        m.insert(i, local[0][f], T, local[2][f])

    def remove(i):
        del cur[i]
        m.remove([i])

    step("empty store + delta", lambda: insert(0, 0, poses[0]))
    step("delta above the store", lambda: insert(1, 1, far(1000.0) @ poses[1]))
    step("delta below the store", lambda: insert(2, 2, far(-1000.0) @ poses[2]))
    assert step("one voxel", lambda: insert(3, 8, poses[3])) == 1
    v = m.stats()["voxels"]
    assert step("all NaN", lambda: insert(4, 9, poses[4])) == 0
    assert m.stats()["voxels"] == v and m.stats()["points_in"] == 5 * 160 * 120
    step("all NaN removed", lambda: remove(4))
    o0 = m.stats()["out_of_range"]
    step("out of range", lambda: insert(5, 5, far((1 << 20) * LEAF - 1.0) @ poses[5]))
    o1 = m.stats()["out_of_range"]
    assert o0 == 0 < o1 < m.stats()["finite"]
    step("mixed sizes", lambda: insert(6, 10, poses[3]))
    assert m.stats()["points_in"] == 5 * 160 * 120 + 352 * 264
    step("one voxel removed", lambda: remove(3))
    step("out of range removed", lambda: remove(5))
    assert m.stats()["out_of_range"] == 0
    step("far ones moved home", lambda: (m.set_poses([1, 2], [poses[1], poses[2]]),
                                        cur.update({1: (1, poses[1]), 2: (2, poses[2])})))


@pytest.mark.gpu
def test_merge_over_several_tiles(capi_gpu, synth):
    capi = capi_gpu
    trk = capi.DenseTracker()
    kfs = [_keyframe(capi, synth, 640, 480, k) for k in range(4)]
    big = ([p for p, _ in kfs], None, [b for _, b in kfs])
    poses = [_step_pose(synth, k, 0.5) for k in range(4)]
    m = capi.KeyframeMap(trk, 0.01)
    cur = {}
    for k in range(3):
        m.insert(k, big[0][k], poses[k], big[2][k])
        cur[k] = (k, poses[k])
    store = m.stats()["voxels"]
    m.insert(3, big[0][3], poses[3], big[2][3])
    cur[3] = (3, poses[3])
    _, _, points, delta, tile = m.timing()
    assert points == 640 * 480 and tile >= 256
    assert store > 2 * tile and delta > 2 * tile, (store, delta, tile)      # both span several merge tiles
    _assert_equal(m, _rebuild(trk, big, cur, 0.01))
    assert m.stats()["voxels"] < store + delta                               # keys met in the merge


@pytest.mark.gpu
def test_box(capi_gpu, frames):
    pyrs, poses, bgrs = frames
    trk = capi_gpu.DenseTracker()
    m = capi_gpu.KeyframeMap(trk, LEAF)
    for k in range(4):
        m.insert(k, pyrs[k], poses[k], bgrs[k])
    xyz, rgb = m.extract()
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    mid = (lo + hi) / 2
    c = xyz[len(xyz) // 2]                                                  # (the scene is a room's walls: its middle is empty)
    boxes = [np.r_[c - np.float32(0.15), c + np.float32(0.15)],             # inside the cloud, around one of its voxels
             np.r_[lo - 1.0, mid],                                          # straddling it
             np.r_[hi + 1.0, hi + 2.0],                                     # disjoint from it
             np.r_[lo, hi]]                                                 # min is in, max is out
    counts = []
    for box in boxes:
        bx, br = m.extract(box)
        keep = in_box(xyz, box)
        assert same_bits(bx, xyz[keep]) and same_bits(br, rgb[keep])
        counts.append(int(keep.sum()))
    assert 0 < counts[0] < len(xyz) and 0 < counts[1] < len(xyz) and counts[2] == 0 and 0 < counts[3] < len(xyz)
    for bad in ([0, 0, 0, 1, np.nan, 1], [0, 0, 0, 1, 0, 1], [0, 2, 0, 1, 1, 1], [np.nan] * 6):
        with pytest.raises(capi_gpu.DvoAmdError) as e:
            m.extract(bad)
        assert e.value.status == 1
    x2, r2 = m.extract()
    assert same_bits(x2, xyz) and same_bits(r2, rgb)


@pytest.mark.gpu
def test_ownership_and_errors(capi_gpu, synth, frames):
    capi = capi_gpu
    L = capi.lib()
    pyrs, poses, bgrs = frames
    trk = capi.DenseTracker()
    m = capi.KeyframeMap(trk, LEAF)
    # the map holds the pyramid and a copy of the image: the caller's go right after insert
    pyr, bgr = _keyframe(capi, synth, 160, 120, 0)
    bgr = bgr.copy()
    m.insert(0, pyr, poses[0], bgr)
    del pyr
    bgr[:] = 0
    del bgr
    m.insert(1, pyrs[1], poses[1], bgrs[1])
    cur = {0: (0, poses[1]), 1: (1, poses[1])}
    m.set_poses([0], [poses[1]])
    _assert_equal(m, _rebuild(trk, frames, cur), "after the caller's objects are gone")
    before = m.extract(), m.stats()

    def refused(fn, word):
        with pytest.raises(capi.DvoAmdError) as e:
            fn()
        assert e.value.status == 1 and word in str(e.value), str(e.value)
        after = m.extract(), m.stats()
        assert same_bits(after[0][0], before[0][0]) and same_bits(after[0][1], before[0][1]) and after[1] == before[1]

    bad = poses[2].copy()
    bad[1, 3] = np.inf
    refused(lambda: m.insert(1, pyrs[2], poses[2], bgrs[2]), "already")
    refused(lambda: m.insert(2, pyrs[2], bad, bgrs[2]), "non-finite")
    refused(lambda: m.set_poses([0, 5], [poses[3], poses[3]]), "not in the map")
    refused(lambda: m.set_poses([0, 1, 0], [poses[3]] * 3), "twice")
    refused(lambda: m.set_poses([1, 0], [poses[3], bad]), "non-finite")
    refused(lambda: m.remove([7]), "not in the map")
    refused(lambda: m.remove([1, 1]), "twice")
    # capacity one short: DVO_AMD_ERR_CAPACITY with the size needed, out untouched
    V = before[1]["voxels"]
    out = np.zeros((V, 4), np.float32)
    n = C.c_longlong()
    assert L.dvo_amd_map_extract(m._h, None, out.ctypes.data, V - 1, C.byref(n)) == 7 and n.value == V and not out.any()
    box = np.array([-9, -9, -9, 9, 9, 9], np.float32)
    assert L.dvo_amd_map_extract(m._h, box.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data, V - 1, C.byref(n)) == 7
    assert n.value == V and not out.any()
    assert L.dvo_amd_map_extract(m._h, None, out.ctypes.data, V, C.byref(n)) == 0 and n.value == V
    assert same_bits(out[:, :3].copy(), before[0][0])
    # refused while pairs are queued on the context
    K = synth.intrinsics_for(320, 240)
    ref = capi.RgbdImagePyramid.from_raw(*synth.sensor_frame(320, 240, None, frame_id=0), K, 4)
    nxt = capi.RgbdImagePyramid.from_raw(*synth.sensor_frame(320, 240, synth.se3_exp(synth.XI_GT_PAIR * 0.5), frame_id=1), K, 4)
    sub = trk.submit([ref] * 4, [nxt] * 4, in_flight=4)
    for call in (lambda: m.insert(3, pyrs[3], poses[3]), lambda: m.set_poses([0], [poses[3]]), lambda: m.remove([0]), m.extract):
        with pytest.raises(capi.DvoAmdError) as e:
            call()
        assert e.value.status == 1
    trk.wait(sub)
    _assert_equal(m, _rebuild(trk, frames, cur), "after the queue drained")
