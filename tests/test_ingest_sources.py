"""Every source of level 0 gives the same pyramid, bit for bit, on every plane of every level.

The expected base planes are the numpy restatement of the raw ingest -- grey = (B*1868 + G*9617 + R*4899 + 8192) >> 14 or the byte
itself, depth = NaN for 0 and float32(raw) * float32(scale) otherwise -- and the expected pyramid is the contiguous host constructor
on them.  Against it: float planes from a strided host array, from device memory (contiguous: two copies; strided from an
unaligned base: k_copy_strided), and the raw frame from host and device memory, contiguous and strided (device: from unaligned
bases, both unaligned branches of k_ingest), with 1 and 3 channels.  The float planes already hold NaN depth.

Shapes: 4x2 one lane; 8x4 whose level 1 is the 4x2 minimum; 260x3 65 lanes, a second block holding one; 72x50 two levels.

One thread test: the plain raw, the remapped and the registered ingest from four threads at once, each thread with a frame of its
own, against the same builds made serially -- the mutex and staging discipline of the one driver behind them."""
import ctypes as C
import os
import sys
import threading
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rectify_ref import grey_plane, same_planes  # noqa: E402

F = np.float32
SCALE = 1.0 / 5000.0
SHAPES = [((4, 2), 1), ((8, 4), 2), ((260, 3), 1), ((72, 50), 2)]
PLANE_KINDS = ["planes_host_strided", "planes_device", "planes_device_offset_strided"]
RAW_KINDS = ["raw_host", "raw_host_strided", "raw_device", "raw_device_offset_strided"]


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


def _gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")


def _frame(rng, w, h, channels):
    image = rng.integers(0, 256, (h, w) if channels == 1 else (h, w, 3)).astype(np.uint8)
    depth = rng.integers(1, 65536, (h, w)).astype(np.uint16)
    depth[rng.uniform(size=(h, w)) < 0.2] = 0
    depth[0, :3] = [0, 1, 65535]                                            # no measurement, the smallest and the largest raw value
    return image, depth


def _expected(image, depth, scale=SCALE):
    I = grey_plane(image).astype(F)
    Z = np.where(depth == 0, F(np.nan), depth.astype(F) * F(scale)).astype(F)
    return I, Z


@pytest.fixture(scope="module")
def cases():
    """per shape and channel count: the raw frame and the restatement's planes -- computed once, never written to"""
    rng = np.random.default_rng(51)
    out = {}
    for (w, h), levels in SHAPES:
        for channels in (1, 3):
            image, depth = _frame(rng, w, h, channels)
            I, Z = _expected(image, depth)
            assert np.isnan(Z[0, 0]) and Z[0, 1] == F(1) * F(SCALE) and Z[0, 2] == F(65535) * F(SCALE) and np.isnan(Z).sum() >= 1
            for a in (image, depth, I, Z):
                a.setflags(write=False)
            out[(w, h), channels] = dict(size=(w, h), levels=levels, image=image, depth=depth, I=I, Z=Z,
                                         K=(F(0.9 * w), F(0.95 * w), F(w / 2 - 0.3), F(h / 2 + 0.2)))
    return out


@pytest.fixture(scope="module")
def references(capi, cases):
    """the contiguous host constructor's pyramid of a case, built on first use and shared"""
    built = {}

    def get(key):
        if key not in built:
            c = cases[key]
            built[key] = capi.RgbdImagePyramid(c["I"], c["Z"], c["K"], c["levels"])
        return built[key]

    return get


def _all_planes_equal(p, q, levels, what):
    assert p.levels() == q.levels() == levels
    for level in range(levels):
        assert p.level_info(level)[:2] == q.level_info(level)[:2] and np.array_equal(p.level_info(level)[2], q.level_info(level)[2])
        for plane in range(6):
            assert same_planes(p.plane(level, plane), q.plane(level, plane)), (what, level, plane)


def _wide(a, width, extra, fill):
    """the rows of `a` (h x width elements) at the start of rows `extra` elements longer, the rest holding `fill`"""
    h = a.shape[0]
    out = np.full((h, width + extra), fill, a.dtype)
    out[:, :width] = a.reshape(h, width)
    return out


def _offset_on_device(torch, wide, view=None):
    """`wide` in device memory one element past an aligned address: (the tensor that owns it, the pointer)"""
    flat = wide.reshape(-1) if view is None else wide.view(view).reshape(-1)
    buf = torch.zeros(flat.size + 1, dtype=torch.from_numpy(flat[:1]).dtype, device="cuda")
    buf[1:] = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + flat.itemsize


def _from_planes(capi, c, kind):
    w, h = c["size"]
    fx, fy, ox, oy = [float(k) for k in c["K"]]
    if kind == "planes_host_strided":
        wide_i, wide_z = _wide(c["I"], w, 3, F(7)), _wide(c["Z"], w, 3, F(7))
        p = capi.RgbdImagePyramid.__new__(capi.RgbdImagePyramid)
        p._h, p.device = C.c_void_p(), 0
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        rc = capi.lib().dvo_amd_pyramid_create(0, fp(wide_i), fp(wide_z), w, h, w + 3, fx, fy, ox, oy, c["levels"], 0.0, C.byref(p._h))
        assert rc == 0, rc
        return p
    import torch

    if kind == "planes_device":
        d_i, d_z = torch.from_numpy(c["I"].copy()).cuda(), torch.from_numpy(c["Z"].copy()).cuda()
        torch.cuda.synchronize()
        return capi.RgbdImagePyramid.from_device(d_i.data_ptr(), d_z.data_ptr(), w, h, c["K"], c["levels"])
    keep_i, p_i = _offset_on_device(torch, _wide(c["I"], w, 3, F(7)))
    keep_z, p_z = _offset_on_device(torch, _wide(c["Z"], w, 3, F(7)))
    assert p_i % 16 == 4 and p_z % 16 == 4
    return capi.RgbdImagePyramid.from_device(p_i, p_z, w, h, c["K"], c["levels"], stride=w + 3)


def _from_raw(capi, c, kind):
    image, depth = c["image"], c["depth"]
    w, h = c["size"]
    channels = 1 if image.ndim == 2 else 3
    row = w * channels
    if kind == "raw_host":
        return capi.RgbdImagePyramid.from_raw(image, depth, c["K"], c["levels"], depth_scale=SCALE)
    istride, zstride = row + 5, w + 3                                       # rows that break the 4- and 8-byte alignment
    wide_i, wide_z = _wide(image, row, 5, 0xAB), _wide(depth, w, 3, 0x1234)
    if kind == "raw_host_strided":
        return capi.RgbdImagePyramid._raw(wide_i.ctypes.data, channels, istride, wide_z.ctypes.data, zstride, SCALE, 0, w, h, c["K"],
                                          c["levels"], 0, 0.0)
    import torch

    if kind == "raw_device":
        d_i, d_z = torch.from_numpy(image.copy()).cuda(), torch.from_numpy(depth.view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        return capi.RgbdImagePyramid.from_raw_device(d_i.data_ptr(), channels, d_z.data_ptr(), w, h, c["K"], c["levels"], depth_scale=SCALE)
    keep_i, p_i = _offset_on_device(torch, wide_i)
    keep_z, p_z = _offset_on_device(torch, wide_z, np.int16)
    assert p_i % 4 == 1 and p_z % 8 == 2
    return capi.RgbdImagePyramid.from_raw_device(p_i, channels, p_z, w, h, c["K"], c["levels"], depth_scale=SCALE,
                                                 image_stride_bytes=istride, depth_stride=zstride)


def _check_source(capi, cases, references, shape, channels, kind, build):
    _gpu(capi)
    if "device" in kind:
        pytest.importorskip("torch")
    c = cases[shape, channels]
    p = build(capi, c, kind)
    _all_planes_equal(p, references((shape, channels)), c["levels"], (shape, channels, kind))
    assert same_planes(p.plane(0, 0), c["I"]) and same_planes(p.plane(0, 1), c["Z"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", PLANE_KINDS)
@pytest.mark.parametrize("shape", [s[0] for s in SHAPES], ids=lambda s: "%dx%d" % s)
def test_float_plane_sources_give_the_host_constructors_pyramid(capi, cases, references, shape, kind):
    _check_source(capi, cases, references, shape, 3, kind, _from_planes)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", RAW_KINDS)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", [s[0] for s in SHAPES], ids=lambda s: "%dx%d" % s)
def test_raw_sources_give_the_host_constructors_pyramid(capi, cases, references, shape, channels, kind):
    _check_source(capi, cases, references, shape, channels, kind, _from_raw)


# ---- threads ----------------------------------------------------------------------------------------------------------------------------

THREADS, ROUNDS, JOIN_SECONDS = 4, 4, 60.0


def _three_builds(capi, job):
    """the plain raw, the remapped and the registered pyramid of a thread's frames, each as (its 12 planes, its statistics)"""
    K, levels = job["K"], 2
    built = [capi.RgbdImagePyramid.from_raw(job["image"], job["depth"], K, levels, depth_scale=SCALE),
             capi.RgbdImagePyramid.from_raw(job["src_image"], job["src_depth"], K, levels, depth_scale=SCALE, remap=job["remap"]),
             capi.RgbdImagePyramid.from_raw(job["image"], job["reg_depth"], K, levels, depth_scale=SCALE, registration=job["registration"])]
    return [([p.plane(level, plane) for level in range(levels) for plane in range(6)], p.registration_stats) for p in built]


def _same_builds(a, b):
    return len(a) == len(b) and all(sa == sb and len(pa) == len(pb) and all(same_planes(x, y) for x, y in zip(pa, pb))
                                    for (pa, sa), (pb, sb) in zip(a, b))


@pytest.mark.gpu
def test_threads_sharing_a_device_build_what_a_single_thread_builds(capi):
    _gpu(capi)
    rng = np.random.default_rng(52)
    w, h, sw, sh, dw, dh = 72, 50, 80, 60, 64, 48
    K = (F(0.9 * w), F(0.95 * w), F(w / 2 - 0.3), F(h / 2 + 0.2))
    mx, my = rng.uniform(-0.1 * sw, 1.1 * sw, (h, w)).astype(F), rng.uniform(-0.1 * sh, 1.1 * sh, (h, w)).astype(F)
    remap = capi.Remap.from_maps(mx, my, (sw, sh))                          # one map shared by all threads
    assert 0 < remap.info()["n_inside"] < w * h
    T = np.eye(4)
    T[:3, 3] = (0.02, -0.01, 0.005)
    registration = capi.Registration(K_depth=(0.9 * dw, 0.95 * dw, dw / 2 - 0.2, dh / 2 + 0.1), T=T, min_z=0.0, fill=True)
    jobs = []
    for t in range(THREADS):                                                # a frame of its own per thread: a mixed-up staging area shows
        image, depth = _frame(rng, w, h, (1, 3)[t % 2])
        src_image, src_depth = _frame(rng, sw, sh, (1, 3)[t % 2])
        jobs.append(dict(K=K, image=image, depth=depth, src_image=src_image, src_depth=src_depth, reg_depth=_frame(rng, dw, dh, 1)[1],
                         remap=remap, registration=registration))
    want = [_three_builds(capi, job) for job in jobs]
    for a in range(THREADS):
        assert want[a][2][1]["drawn"] > 0
        for b in range(a):
            assert not _same_builds(want[a], want[b])                       # (the frames differ: so do the pyramids)
    verdicts, errors = [[] for _ in jobs], []

    def work(t):
        try:
            for _ in range(ROUNDS):
                verdicts[t].append(_same_builds(_three_builds(capi, jobs[t]), want[t]))
        except Exception as e:                                              # noqa: BLE001  (reported by the test below)
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(THREADS)]
    for th in threads:
        th.start()
    deadline = time.monotonic() + JOIN_SECONDS
    for th in threads:
        th.join(max(0.0, deadline - time.monotonic()))
    if any(th.is_alive() for th in threads):
        pytest.fail("a thread did not finish within %g s" % JOIN_SECONDS)
    assert not errors, errors
    assert verdicts == [[True] * ROUNDS] * THREADS, verdicts
