"""Rectification at ingest above the C ABI: dvo::core::Rectification (include/dvo_amd/rectification.hpp) in
examples/rectified_ingest_adaptor_example.cpp and the C99 example examples/rectified_ingest_example.c.
CPU: both compile against the headers with -Werror (the C++ one as plain C++11 and against the Eigen / OpenCV mocks).
GPU: both run; the n_inside and the plane checksums they print are those of the Python binding on the same frame and camera."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCKS = os.path.join(ROOT, "tests", "mock_include")  # TEST-ONLY stand-ins for <Eigen/Geometry> and <opencv2/core/core.hpp>


def _compile(kind):
    from dvo_slam_amd import _build

    _build.build()
    exe = os.path.join(ROOT, "examples", "_build", "rectified_ingest_example_" + kind)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.join(ROOT, "dvo_slam_amd")
    link = ["-o", exe, "-L" + libdir, "-ldvo_amd", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    if kind == "c":
        cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "rectified_ingest_example.c")] + link
    else:
        cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if kind == "mock" else []) + [
               "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "rectified_ingest_adaptor_example.cpp")] + link
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


@pytest.mark.parametrize("kind", ["c", "cpp", "mock"])
def test_rectified_ingest_examples_compile(kind):
    assert os.path.exists(_compile(kind))


def _checksum(plane):
    words = np.ascontiguousarray(plane, np.float32).view(np.uint32).copy()
    words[np.isnan(plane)] = 0x7FC00000
    h = 0
    for word in words.reshape(-1).tolist():
        h = (h * 31 + word) & 0xFFFFFFFF
    return h


@pytest.fixture(scope="module")
def expected_lines():
    """the lines both examples print, from the Python binding on the same synthetic frame"""
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    sw, sh, w, h, levels = 80, 60, 72, 50, 2
    u, v = np.meshgrid(np.arange(sw), np.arange(sh))
    bgr = np.stack([(3 * u + 5 * v) % 256, (7 * u + v) % 256, (u + 11 * v) % 256], -1).astype(np.uint8)
    depth = np.where((u + 2 * v) % 9 == 0, 0, 5000 + 13 * u + 7 * v).astype(np.uint16)
    k_out, k_src, dist = (60.0, 60.0, 35.5, 24.5), (64.0, 64.0, 39.5, 29.5), (0.1, -0.05, 0.002, -0.001, 0.01)
    remap = capi.Remap.undistort((w, h), k_out, (sw, sh), k_src, dist)
    i = remap.info()
    assert 0.5 * w * h < i["n_inside"] < w * h                             # the example's table has both kinds of pixel
    lines = ["remap: %d x %d from %d x %d, %d inside" % (i["width"], i["height"], i["src_width"], i["src_height"], i["n_inside"])]
    p = capi.RgbdImagePyramid.from_raw(bgr, depth, k_out, levels, depth_scale=1.0 / 5000.0, remap=remap)
    for l in range(levels):
        lw, lh, _ = p.level_info(l)
        lines.append("level %d: %d x %d intensity %08x depth %08x" % (l, lw, lh, _checksum(p.plane(l, 0)), _checksum(p.plane(l, 1))))
    return lines


@pytest.mark.gpu
def test_c_example_prints_the_bindings_checksums(expected_lines):
    res = subprocess.run([_compile("c")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.splitlines() == expected_lines


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cpp", "mock"])
def test_cpp_wrapper_prints_the_bindings_checksums(expected_lines, kind):
    res = subprocess.run([_compile(kind)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.splitlines() == expected_lines + ["fromMaps gives the same pyramid: 1"]
