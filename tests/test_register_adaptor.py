"""Registered ingest above the C ABI: dvo::core::DepthRegistration (include/dvo_amd/depth_registration.hpp) in
examples/registered_ingest_adaptor_example.cpp and the C99 example examples/registered_ingest_example.c.
CPU: both compile against the headers with -Werror (the C++ one as plain C++11 and against the Eigen / OpenCV mocks).
GPU: both run; the counters and the plane checksums they print are those of the Python binding on the same frames and cameras."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCKS = os.path.join(ROOT, "tests", "mock_include")  # TEST-ONLY stand-ins for <Eigen/Geometry> and <opencv2/core/core.hpp>


def _compile(kind):
    from dvo_slam_amd import _build

    _build.build()
    exe = os.path.join(ROOT, "examples", "_build", "registered_ingest_example_" + kind)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.join(ROOT, "dvo_slam_amd")
    link = ["-o", exe, "-L" + libdir, "-ldvo_amd", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    if kind == "c":
        cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "registered_ingest_example.c")] + link
    else:
        cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if kind == "mock" else []) + [
               "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "registered_ingest_adaptor_example.cpp")] + link
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


@pytest.mark.parametrize("kind", ["c", "cpp", "mock"])
def test_registered_ingest_examples_compile(kind):
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
    """the lines both examples print, from the Python binding on the same synthetic frames"""
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    sw, sh, w, h, dw, dh, levels = 80, 60, 72, 50, 40, 30, 2
    u, v = np.meshgrid(np.arange(sw), np.arange(sh))
    bgr = np.stack([(3 * u + 5 * v) % 256, (7 * u + v) % 256, (u + 11 * v) % 256], -1).astype(np.uint8)
    u, v = np.meshgrid(np.arange(dw), np.arange(dh))
    depth = np.where((u + 2 * v) % 9 == 0, 0, np.where((u + v) % 17 == 0, 1000, 5000 + 130 * u + 70 * v)).astype(np.uint16)
    k_colour, k_src, dist = (60.0, 60.0, 35.5, 24.5), (64.0, 64.0, 39.5, 29.5), (0.1, -0.05, 0.002, -0.001, 0.01)
    T = np.array([[0.9998, 0, 0.02, 0.025], [0, 1, 0, 0.001], [-0.02, 0, 0.9998, -0.004], [0, 0, 0, 1]])
    reg = capi.Registration(K_depth=(26.0, 26.0, 19.5, 14.5), T=T, min_z=0.3, fill=True)
    remap = capi.Remap.undistort((w, h), k_colour, (sw, sh), k_src, dist)
    lines = []
    for what, image, rm, fill in (("registered", bgr[:h, :w], None, True), ("registered and rectified", bgr, remap, False)):
        reg.fill = fill
        p = capi.RgbdImagePyramid.from_raw(image, depth, k_colour, levels, depth_scale=1.0 / 5000.0, remap=rm, registration=reg)
        st = p.registration_stats
        assert st["behind"] > 0 and st["outside"] > 0 and st["drawn"] > 0      # the example's frame takes every path of the rule
        lines.append("%s: %d measurements, %d behind, %d outside, %d drawn, %d covered" % (
            what, st["measurements"], st["behind"], st["outside"], st["drawn"], st["covered_pixels"]))
        for l in range(levels):
            lw, lh, _ = p.level_info(l)
            lines.append("level %d: %d x %d intensity %08x depth %08x" % (l, lw, lh, _checksum(p.plane(l, 0)), _checksum(p.plane(l, 1))))
    return lines


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["c", "cpp", "mock"])
def test_example_prints_the_bindings_counters_and_checksums(expected_lines, kind):
    res = subprocess.run([_compile(kind)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.splitlines() == expected_lines
