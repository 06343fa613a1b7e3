"""The keyframe map's point cloud (dvo_amd.h: dvo_amd_point_cloud, dvo_amd_map_cloud, dvo_amd_voxel_downsample,
dvo_amd_write_pcd) against a numpy restatement of the semantics the header pins.

The restatement lives here, in the test: `cloud_ref` is RgbdCamera::buildPointCloud + the pinned transform order + the colour
rule, `voxel_ref` the voxel aggregate (pcl::VoxelGrid's index rule, key order, fixed-point centroid, integer colour mean).
CPU tests check the restatement against a brute-force dict of voxels and the PCD writer; GPU tests check the library against
the restatement bit for bit."""
import ctypes as C

import numpy as np
import pytest

BIAS = 1 << 20
FIX = 2.0 ** 24


# ---- the restatement ----------------------------------------------------------------------------------------------------

def rays(w, h, K):
    fx, fy, ox, oy = [np.float32(k) for k in K]
    return (np.arange(w, dtype=np.float32) - ox) / fx, (np.arange(h, dtype=np.float32) - oy) / fy


def grey_rgb(I):
    g = np.where(np.isnan(I), np.float32(0), I)
    g = np.trunc(np.clip(g, np.float32(0), np.float32(255))).astype(np.uint32)
    return (g << 16) | (g << 8) | g


def bgr_rgb(bgr):
    b = bgr.astype(np.uint32)
    return (b[..., 2] << 16) | (b[..., 1] << 8) | b[..., 0]


def cloud_ref(Z, I, K, pose=None, bgr=None):
    """organized cloud: (xyz float32 [h, w, 3], rgb uint32 [h, w])"""
    h, w = Z.shape
    tx, ty = rays(w, h, K)
    x, y, z = tx[None, :] * Z, ty[:, None] * Z, Z
    T = (np.eye(4) if pose is None else np.asarray(pose, dtype=np.float64)).astype(np.float32)
    out = np.empty((h, w, 3), np.float32)
    for r in range(3):
        out[..., r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
    return out, (grey_rgb(I) if bgr is None else bgr_rgb(bgr))


def voxel_ref(xyz, rgb, leaf):
    """(xyz float32 [V, 3], rgb uint32 [V], stats) of the voxel aggregate"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint32).reshape(-1)
    finite = np.isfinite(xyz).all(axis=1)
    inv = np.float32(1.0) / np.float32(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(xyz * inv)
        inr = finite & ((f >= -BIAS) & (f < BIAS)).all(axis=1)
    p, c = xyz[inr], rgb[inr]
    idx = f[inr].astype(np.int64) + BIAS
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    order = np.argsort(key, kind="stable")
    key, p, c = key[order], p[order], c[order]
    stats = {"points_in": len(xyz), "finite": int(finite.sum()), "out_of_range": int(finite.sum() - inr.sum())}
    if len(key) == 0:
        stats["voxels"] = 0
        return np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), stats
    heads = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    count = np.diff(np.r_[heads, len(key)]).astype(np.int64)
    q = np.rint(p.astype(np.float64) * FIX).astype(np.int64)
    s = np.add.reduceat(q, heads, axis=0)
    out = (s.astype(np.float64) / (count.astype(np.float64) * FIX)[:, None]).astype(np.float32)
    ch = np.stack([(c >> 16) & 0xFF, (c >> 8) & 0xFF, c & 0xFF], axis=1).astype(np.int64)
    cs = np.add.reduceat(ch, heads, axis=0)
    m = (cs + (count // 2)[:, None]) // count[:, None]
    stats["voxels"] = len(heads)
    return out, ((m[:, 0] << 16) | (m[:, 1] << 8) | m[:, 2]).astype(np.uint32), stats


def voxel_brute(xyz, rgb, leaf):
    """the same aggregate point by point into a dict of voxels (Python integers: no wrap, no vectorised shortcut)"""
    inv = np.float32(1.0) / np.float32(leaf)
    vox, finite, oor = {}, 0, 0
    for P, col in zip(np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(rgb, np.uint32).reshape(-1)):
        if not all(np.isfinite(P)):
            continue
        finite += 1
        with np.errstate(invalid="ignore", over="ignore"):
            ijk = [np.floor(np.float32(v) * inv) for v in P]
        if not all(-BIAS <= v < BIAS for v in ijk):
            oor += 1
            continue
        key = ((int(ijk[0]) + BIAS) << 42) | ((int(ijk[1]) + BIAS) << 21) | (int(ijk[2]) + BIAS)
        e = vox.setdefault(key, [0, 0, 0, 0, 0, 0, 0])
        e[0] += 1
        for a in range(3):
            e[1 + a] += int(np.rint(float(P[a]) * FIX))
        col = int(col)
        e[4] += (col >> 16) & 0xFF
        e[5] += (col >> 8) & 0xFF
        e[6] += col & 0xFF
    keys = sorted(vox)
    out = np.array([[np.float32(vox[k][1 + a] / (vox[k][0] * FIX)) for a in range(3)] for k in keys], np.float32).reshape(-1, 3)
    cols = []
    for k in keys:
        n = vox[k][0]
        r, g, b = [(vox[k][4 + a] + n // 2) // n for a in range(3)]
        cols.append((r << 16) | (g << 8) | b)
    return out, np.array(cols, np.uint32), {"finite": finite, "out_of_range": oor, "voxels": len(keys)}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def random_cloud(rng, n, leaf):
    xyz = rng.normal(scale=0.2, size=(n, 3)).astype(np.float32)
    xyz[rng.random(n) < 0.05, rng.integers(0, 3)] = np.nan                         # NaN points
    b = rng.random(n) < 0.1                                                          # on voxel boundaries
    xyz[b] = (np.round(xyz[b] / leaf) * leaf).astype(np.float32)
    xyz[rng.random(n) < 0.3] *= -1                                                   # negative coordinates
    o = rng.random(n) < 0.02                                                         # out of range
    xyz[o, 0] = np.float32(leaf * (BIAS + 3)) * rng.choice([-1, 1], size=o.sum())
    xyz[rng.random(n) < 0.005, 1] = np.inf
    rgb = rng.integers(0, 1 << 24, size=n, dtype=np.uint32)
    return xyz, rgb


# ---- CPU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leaf", [0.05, 0.01, 0.25])
def test_restatement_matches_brute_force(leaf):
    rng = np.random.default_rng(int(leaf * 1000))
    xyz, rgb = random_cloud(rng, 3000, leaf)
    # few voxels with many points each, too
    xyz[:500] = (xyz[:500] * np.float32(0.05)).astype(np.float32)
    a_xyz, a_rgb, a_st = voxel_ref(xyz, rgb, leaf)
    b_xyz, b_rgb, b_st = voxel_brute(xyz, rgb, leaf)
    assert a_st["out_of_range"] > 0 and a_st["finite"] < len(xyz)
    assert {k: a_st[k] for k in b_st} == b_st
    assert same_bits(a_xyz, b_xyz) and same_bits(a_rgb, b_rgb)
    # the result does not depend on the order of the points
    perm = rng.permutation(len(xyz))
    c_xyz, c_rgb, _ = voxel_ref(xyz[perm], rgb[perm], leaf)
    assert same_bits(a_xyz, c_xyz) and same_bits(a_rgb, c_rgb)


def test_restatement_colour_rules():
    I = np.array([[np.nan, -3.0, 0.0, 17.9], [254.99, 255.0, 300.0, np.inf]], np.float32)
    g = grey_rgb(I) & 0xFF
    assert g.tolist() == [[0, 0, 0, 17], [254, 255, 255, 255]]
    assert bgr_rgb(np.array([[[1, 2, 3]]], np.uint8))[0, 0] == 0x030201


def _parse_pcd(path):
    blob = open(path, "rb").read()
    at = blob.index(b"DATA binary\n") + len(b"DATA binary\n")
    head = dict(line.split(" ", 1) for line in blob[:at].decode().splitlines() if not line.startswith("#"))
    return head, blob[at:]


def test_write_pcd_round_trip(tmp_path):
    from dvo_slam_amd import tum

    rng = np.random.default_rng(5)
    xyz = rng.normal(size=(3, 4, 3)).astype(np.float32)
    xyz[1, 2] = np.nan
    rgb = rng.integers(0, 1 << 24, size=(3, 4), dtype=np.uint32)
    p = str(tmp_path / "organized.pcd")
    tum.write_pcd(p, xyz, rgb)
    head, data = _parse_pcd(p)
    assert head["VERSION"] == "0.7" and head["FIELDS"] == "x y z rgb" and head["SIZE"] == "4 4 4 4"
    assert head["TYPE"] == "F F F F" and head["COUNT"] == "1 1 1 1" and head["VIEWPOINT"] == "0 0 0 1 0 0 0"
    assert (head["WIDTH"], head["HEIGHT"], head["POINTS"]) == ("4", "3", "12")
    rec = np.frombuffer(data, np.float32).reshape(-1, 4)
    assert same_bits(rec[:, :3].reshape(3, 4, 3).copy(), xyz)
    assert same_bits(rec[:, 3].view(np.uint32).reshape(3, 4).copy(), rgb)
    q = str(tmp_path / "list.pcd")
    tum.write_pcd(q, xyz.reshape(-1, 3), rgb.reshape(-1))
    head, data2 = _parse_pcd(q)
    assert (head["WIDTH"], head["HEIGHT"], head["POINTS"]) == ("12", "1", "12") and data2 == data
    tum.write_pcd(str(tmp_path / "empty.pcd"), np.zeros((0, 3), np.float32), np.zeros(0, np.uint32))
    assert _parse_pcd(str(tmp_path / "empty.pcd"))[1] == b""


def test_map_entries_fail_loudly_without_a_gpu():
    from dvo_slam_amd import capi

    L = capi.lib()
    if L.dvo_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    pts = np.zeros((4, 4), np.float32)
    st = capi.CCloudStats()
    assert L.dvo_amd_point_cloud(None, None, 0, None, None, 0, pts.ctypes.data) == 2
    assert L.dvo_amd_map_cloud(None, 0, None, None, None, None, 0.01, pts.ctypes.data, 4, C.byref(st)) == 2
    assert L.dvo_amd_voxel_downsample(None, 4, pts.ctypes.data, 0.01, pts.ctypes.data, 4, C.byref(st)) == 2
    d = C.c_double()
    assert L.dvo_amd_debug_map_timing(None, C.byref(d), None, None) == 2


# ---- GPU ----------------------------------------------------------------------------------------------------------------

def _frame(capi, synth, w, h, pose=None, frame_id=0, channels=1, levels=4):
    img, raw = synth.sensor_frame(w, h, pose, frame_id=frame_id, channels=channels)
    K = synth.intrinsics_for(w, h)
    return capi.RgbdImagePyramid.from_raw(img, raw, K, levels), img


def _poses(synth, n, seed=11):
    rng = np.random.default_rng(seed)
    return [synth.se3_exp(np.r_[rng.normal(scale=0.3, size=3), rng.normal(scale=0.2, size=3)]) for _ in range(n)]


def _restate_level(pyr, level, pose, bgr):
    w, h, K = pyr.level_info(level)
    return cloud_ref(pyr.plane(level, 1), pyr.plane(level, 0), K, pose, bgr)


@pytest.fixture(scope="module")
def capi_gpu():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(640, 480), (1280, 960), (352, 264)])
def test_point_cloud_equals_restatement(capi_gpu, synth, size):
    capi = capi_gpu
    w, h = size
    pyr, _ = _frame(capi, synth, w, h, synth.se3_exp([0.1, -0.05, 0.02, 0.03, 0.01, -0.02]))
    rng = np.random.default_rng(w)
    poses = [None, synth.se3_exp([0.3, -0.2, 0.1, 0.2, -0.1, 0.3]), synth.se3_exp([-1.5, 2.0, 0.7, -0.9, 1.2, 0.4]),
             np.diag([1.0, -1.0, -1.0, 1.0]) @ synth.se3_exp([0.01, 0.02, 3.0, 0.0, 0.0, 1.5])]
    for level in range(4):
        lw, lh, _ = pyr.level_info(level)
        nan_ref = np.isnan(pyr.plane(level, 1))
        assert nan_ref.any() and not nan_ref.all()
        for k, pose in enumerate(poses):
            bgr = rng.integers(0, 256, size=(lh, lw, 3), dtype=np.uint8) if k % 2 else None
            xyz, rgb = pyr.point_cloud(pose=pose, bgr=bgr, level=level)
            rx, rr = _restate_level(pyr, level, pose, bgr)
            assert xyz.shape == (lh, lw, 3) and rgb.shape == (lh, lw)
            assert same_bits(xyz, rx), (size, level, k)
            assert same_bits(rgb, rr), (size, level, k)
            assert np.array_equal(np.isnan(xyz).any(axis=2), nan_ref)


@pytest.fixture(scope="module")
def keyframes(capi_gpu, synth):
    """50 keyframes of 640x480 at distinct poses, half of them with a BGR image"""
    capi = capi_gpu
    poses = [synth.se3_exp(np.array([0.02 * k, -0.01 * k, 0.015 * k, 0.01 * k, -0.02 * k, 0.005 * k]) * 0.5) for k in range(50)]
    pyrs, bgrs = [], []
    for k, T in enumerate(poses):
        I, Z = synth.render(640, 480, T, frame_id=k)
        bgr, raw = synth.to_raw(I, Z)
        pyrs.append(capi.RgbdImagePyramid.from_raw(bgr, raw, synth.intrinsics_for(640, 480), 1))
        bgrs.append(bgr if k % 2 == 0 else None)
    return pyrs, poses, bgrs


def _restate_map(keyframes, leaf):
    pyrs, poses, bgrs = keyframes
    clouds = [_restate_level(p, 0, T, b) for p, T, b in zip(pyrs, poses, bgrs)]
    return voxel_ref(np.concatenate([c[0].reshape(-1, 3) for c in clouds]), np.concatenate([c[1].reshape(-1) for c in clouds]),
                     leaf)


@pytest.mark.gpu
def test_map_cloud_equals_restatement(capi_gpu, keyframes):
    capi = capi_gpu
    pyrs, poses, bgrs = keyframes
    trk = capi.DenseTracker()
    xyz, rgb, st = trk.map_cloud(pyrs, poses, bgrs, leaf=0.01)
    rx, rr, rst = _restate_map(keyframes, 0.01)
    assert st == rst
    assert st["points_in"] == 50 * 640 * 480 and st["voxels"] > 100000
    assert same_bits(xyz, rx) and same_bits(rgb, rr)
    # determinism: shuffled keyframe order, a second run, a second context
    perm = np.random.default_rng(3).permutation(50)
    xs, rs, ss = trk.map_cloud([pyrs[i] for i in perm], [poses[i] for i in perm], [bgrs[i] for i in perm], leaf=0.01)
    assert ss == st and same_bits(xs, xyz) and same_bits(rs, rgb)
    x2, r2, s2 = trk.map_cloud(pyrs, poses, bgrs, leaf=0.01)
    assert s2 == st and same_bits(x2, xyz) and same_bits(r2, rgb)
    x3, r3, s3 = capi.DenseTracker().map_cloud(pyrs, poses, bgrs, leaf=0.01)
    assert s3 == st and same_bits(x3, xyz) and same_bits(r3, rgb)
    # = the downsampling of the concatenated organized clouds
    clouds = [p.point_cloud(pose=T, bgr=b, tracker=trk) for p, T, b in zip(pyrs, poses, bgrs)]
    xd, rd, sd = trk.voxel_downsample(np.concatenate([c[0].reshape(-1, 3) for c in clouds]),
                                      np.concatenate([c[1].reshape(-1) for c in clouds]), 0.01)
    assert sd == st and same_bits(xd, xyz) and same_bits(rd, rgb)


@pytest.mark.gpu
@pytest.mark.parametrize("leaf", [0.005, 0.05])
def test_map_cloud_leaf_sizes(capi_gpu, keyframes, leaf):
    pyrs, poses, bgrs = keyframes
    sub = (pyrs[::5], poses[::5], bgrs[::5])
    xyz, rgb, st = capi_gpu.DenseTracker().map_cloud(*sub, leaf=leaf)
    rx, rr, rst = _restate_map(sub, leaf)
    assert st == rst and same_bits(xyz, rx) and same_bits(rgb, rr)


@pytest.mark.gpu
def test_voxel_downsample_random_points(capi_gpu):
    rng = np.random.default_rng(9)
    trk = capi_gpu.DenseTracker()
    for leaf in (0.01, 0.05):
        xyz, rgb = random_cloud(rng, 200000, leaf)
        a = trk.voxel_downsample(xyz, rgb, leaf)
        r = voxel_ref(xyz, rgb, leaf)
        assert a[2] == r[2] and same_bits(a[0], r[0]) and same_bits(a[1], r[1])
        perm = rng.permutation(len(xyz))
        b = trk.voxel_downsample(xyz[perm], rgb[perm], leaf)
        assert b[2] == a[2] and same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    # one voxel holding every point
    xyz = np.full((100000, 3), 0.123, np.float32)
    rgb = np.arange(100000, dtype=np.uint32)
    a = trk.voxel_downsample(xyz, rgb, 1.0)
    r = voxel_ref(xyz, rgb, 1.0)
    assert a[2] == r[2] and a[2]["voxels"] == 1 and same_bits(a[0], r[0]) and same_bits(a[1], r[1])


@pytest.mark.gpu
def test_map_cloud_edge_cases(capi_gpu, synth, keyframes):
    capi = capi_gpu
    L = capi.lib()
    trk = capi.DenseTracker()
    xyz, rgb, st = trk.map_cloud([], [], leaf=0.01)
    assert xyz.shape == (0, 3) and rgb.shape == (0,) and st == {"points_in": 0, "finite": 0, "out_of_range": 0, "voxels": 0}
    I = np.full((120, 160), 100.0, np.float32)
    nan_pyr = capi.RgbdImagePyramid(I, np.full((120, 160), np.nan, np.float32), synth.intrinsics_for(160, 120), 1)
    xyz, rgb, st = trk.map_cloud([nan_pyr], [np.eye(4)], leaf=0.01)
    assert len(xyz) == 0 and st == {"points_in": 160 * 120, "finite": 0, "out_of_range": 0, "voxels": 0}
    # capacity one short: DVO_AMD_ERR_CAPACITY with the count needed
    pyrs, poses, bgrs = keyframes
    _, _, full = trk.map_cloud(pyrs[:3], poses[:3], leaf=0.01)
    V = full["voxels"]
    hs = (C.c_void_p * 3)(*[p._h for p in pyrs[:3]])
    T = np.ascontiguousarray(np.stack([np.asarray(P, np.float64).T for P in poses[:3]]))
    out = np.zeros((V, 4), np.float32)
    stats = capi.CCloudStats()
    rc = L.dvo_amd_map_cloud(trk._h, 3, hs, T.ctypes.data_as(C.POINTER(C.c_double)), None, None, 0.01, out.ctypes.data, V - 1,
                             C.byref(stats))
    assert rc == 7 and stats.voxels == V and not out.any()
    rc = L.dvo_amd_map_cloud(trk._h, 3, hs, T.ctypes.data_as(C.POINTER(C.c_double)), None, None, 0.01, out.ctypes.data, V,
                             C.byref(stats))
    assert rc == 0 and stats.voxels == V
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        assert L.dvo_amd_map_cloud(trk._h, 3, hs, T.ctypes.data_as(C.POINTER(C.c_double)), None, None, bad, out.ctypes.data,
                                   V, C.byref(stats)) == 1
    # refused while pairs are queued
    ref, _ = _frame(capi, synth, 320, 240)
    cur, _ = _frame(capi, synth, 320, 240, synth.se3_exp(synth.XI_GT_PAIR * 0.5), frame_id=1)
    sub = trk.submit([ref] * 4, [cur] * 4, in_flight=4)
    with pytest.raises(capi.DvoAmdError) as e:
        trk.map_cloud(pyrs[:2], poses[:2], leaf=0.01)
    assert e.value.status == 1
    with pytest.raises(capi.DvoAmdError) as e:
        pyrs[0].point_cloud(tracker=trk)
    assert e.value.status == 1
    with pytest.raises(capi.DvoAmdError) as e:
        trk.voxel_downsample(np.zeros((4, 3), np.float32), np.zeros(4, np.uint32), 0.01)
    assert e.value.status == 1
    trk.wait(sub)
    assert trk.map_cloud(pyrs[:2], poses[:2], leaf=0.01)[2]["points_in"] == 2 * 640 * 480
