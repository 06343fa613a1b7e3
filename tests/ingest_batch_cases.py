"""What tests/test_ingest_batch_entries.py (any host) and tests/test_ingest_batch.py (GPU) share: the frames of a batch, the raw
call of dvo_amd_pyramid_create_raw_batch with strides, and the compile lines of the two examples."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCKS = os.path.join(ROOT, "tests", "mock_include")  # TEST-ONLY stand-ins for <Eigen/Geometry> and <opencv2/core/core.hpp>
SCALE = 1.0 / 5000.0
# (width, height) -> levels: the smallest pyramid check_levels allows; rows longer than one 256-pixel block; a level 0 whose
# 21 120 pixels cross one 16 384-pixel pad unit, every level's width (528, 264, 132) a multiple of 4
SHAPES = {(8, 4): 2, (320, 24): 3, (528, 40): 3}
MAX_FRAMES = 5
XI_STEP = np.array([0.004, -0.002, 0.003, 0.002, -0.003, 0.001])  # camera motion from one frame of a batch to the next


@functools.lru_cache(maxsize=None)
def frames(shape, channels):
    """MAX_FRAMES different sensor frames (uint8 grey or BGR, uint16 depth) of one camera moving through the synthetic scene, and
    the camera: ([(image, depth)], K).  Read-only: the tests share them."""
    from dvo_slam_amd import synth

    w, h = shape
    out = []
    for f in range(MAX_FRAMES):
        image, depth = synth.sensor_frame(w, h, synth.se3_exp(XI_STEP * f), frame_id=f, channels=channels)
        image, depth = np.ascontiguousarray(image, np.uint8), np.ascontiguousarray(depth, np.uint16)
        image.setflags(write=False), depth.setflags(write=False)
        out.append((image, depth))
    return out, tuple(float(k) for k in synth.intrinsics_for(w, h))


def wide(a, pad, fill):
    """the rows of `a` (HxW or HxWxC) with `pad` more elements behind each, holding `fill`: (the 2-D array, its row length)"""
    flat = a.reshape(a.shape[0], -1)
    out = np.full((flat.shape[0], flat.shape[1] + pad), fill, flat.dtype)
    out[:, :flat.shape[1]] = flat
    return out, out.shape[1]


def create_raw_batch(capi, image_ptrs, depth_ptrs, channels, istride, zstride, on_device, shape, K, levels, selection=None, timestamps=None,
                     device=0):
    """dvo_amd_pyramid_create_raw_batch on raw pointers with explicit strides: (status, [RgbdImagePyramid] or None)"""
    n = len(image_ptrs)
    b = capi.CRawBatch()
    b.count = n
    b.images, b.depths = (C.c_void_p * n)(*image_ptrs), (C.c_void_p * n)(*depth_ptrs)
    b.timestamps = None if timestamps is None else (C.c_double * n)(*timestamps)
    b.channels, b.image_stride_bytes, b.depth_stride, b.depth_scale, b.on_device = channels, istride, zstride, SCALE, int(on_device)
    b.width, b.height = shape
    b.fx, b.fy, b.ox, b.oy = K
    b.levels, b.build_selection = levels, int(selection is not None)
    if selection is not None:
        b.intensity_threshold, b.depth_threshold = selection
    out = (C.c_void_p * n)()
    rc = capi.lib().dvo_amd_pyramid_create_raw_batch(device, C.byref(b), out)
    if rc != 0:
        assert not any(out[f] for f in range(n))
        return rc, None
    pyramids = []
    for f in range(n):
        p = capi.RgbdImagePyramid.__new__(capi.RgbdImagePyramid)
        p._h, p.device, p.registration_stats = C.c_void_p(out[f]), device, None
        pyramids.append(p)
    return rc, pyramids


def compile_example(kind):
    """examples/batch_ingest_example.c ("c") or examples/batch_ingest_adaptor_example.cpp as plain C++11 ("cpp") and against the Eigen /
    OpenCV mocks ("mock"); returns the executable"""
    from dvo_slam_amd import _build

    _build.build()
    exe = os.path.join(ROOT, "examples", "_build", "batch_ingest_example_" + kind)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.join(ROOT, "dvo_slam_amd")
    link = ["-o", exe, "-L" + libdir, "-ldvo_amd", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    if kind == "c":
        cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "batch_ingest_example.c")] + link
    else:
        cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if kind == "mock" else []) + [
               "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "batch_ingest_adaptor_example.cpp")] + link
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe
