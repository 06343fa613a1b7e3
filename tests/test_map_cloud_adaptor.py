"""The C++ adaptor of the keyframe map (include/dvo_amd/point_cloud.hpp, RgbdImage::rgb / RgbdImage::pointcloud of
include/dvo_amd/dense_tracking.hpp).  examples/map_cloud_example.cpp is written like graph_visualizer.cpp:255 and
point_cloud_aggregator.cpp:74-109 use these classes.
CPU: it compiles as plain C++11 and against the Eigen / OpenCV mocks with -Werror.
GPU: its map of 120 named keyframes equals the Python binding's map_cloud of the 60 the reference's rule picks (std::map name
order, every max(n / 50, 1)-th), and RgbdImage::pointcloud equals point_cloud at the identity pose."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCKS = os.path.join(ROOT, "tests", "mock_include")  # TEST-ONLY stand-ins for <Eigen/Geometry> and <opencv2/core/core.hpp>


def _compile(mocks):
    from dvo_slam_amd import _build

    _build.build()
    exe = os.path.join(ROOT, "examples", "_build", "map_cloud_example" + ("_mock" if mocks else ""))
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.join(ROOT, "dvo_slam_amd")
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
           "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "map_cloud_example.cpp"), "-o", exe, "-L" + libdir, "-ldvo_amd",
           "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


@pytest.mark.parametrize("mocks", [False, True])
def test_map_cloud_example_compiles(mocks):
    assert os.path.exists(_compile(mocks))


def _to8(bgr):
    """dvo_amd.h's colour rule on float BGR: clamped to [0, 255], truncated, NaN -> 0"""
    g = np.where(np.isnan(bgr), np.float32(0), bgr)
    return np.trunc(np.clip(g, 0, 255)).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("mocks", [False, True])
def test_aggregator_and_pointcloud_match_python_binding(tmp_path, synth, mocks):
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    exe = _compile(mocks)
    w, h, n = 160, 120, 120
    K = synth.intrinsics_for(w, h)
    rng = np.random.default_rng(17)
    I, Z, P, B = [], [], [], []
    for k in range(n):
        T = synth.se3_exp(np.r_[rng.normal(scale=0.2, size=3), rng.normal(scale=0.1, size=3)])
        i, z = synth.render(w, h, T, frame_id=k)
        I.append(i), Z.append(z), P.append(T)
        b = rng.uniform(-20.0, 280.0, size=(h, w, 3)).astype(np.float32)  # out of range on purpose: the clamp is exercised
        b[rng.random((h, w)) < 0.01] = np.nan
        B.append(b)
    frames = tmp_path / "frames.bin"
    with open(frames, "wb") as fh:
        np.ascontiguousarray(np.stack(I), np.float32).tofile(fh)
        np.ascontiguousarray(np.stack(Z), np.float32).tofile(fh)
        np.ascontiguousarray(np.stack([T.T for T in P]), np.float64).tofile(fh)  # column-major
        np.ascontiguousarray(np.stack(B), np.float32).tofile(fh)
    out = tmp_path / "out.bin"
    res = subprocess.run([exe, str(w), str(h)] + [repr(float(k)) for k in K] + [str(n), str(frames), str(out)],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert res.stdout.split()[-1] == "1"  # an empty aggregator returns the reference's single default point
    blob = open(out, "rb").read()
    V = int(np.frombuffer(blob[:8], np.uint64)[0])
    rec = np.frombuffer(blob[8:8 + 16 * V], np.uint8).reshape(V, 16)
    xyz = rec[:, :12].copy().view(np.float32).reshape(V, 3)
    rgb = (rec[:, 12].astype(np.uint32) << 16) | (rec[:, 13].astype(np.uint32) << 8) | rec[:, 14].astype(np.uint32)
    at = 8 + 16 * V
    cols = int(np.frombuffer(blob[at:at + 8], np.uint64)[0])
    pc = np.frombuffer(blob[at + 8:], np.float32).reshape(cols, 4)

    # the reference's pick: names in std::map order, every max(n / 50, 1)-th
    names = sorted(str(k) for k in range(n))
    picked = [int(s) for s in names[::max(n // 50, 1)]]
    assert len(picked) == 60
    pyrs = {k: capi.RgbdImagePyramid(I[k], Z[k], K, 1) for k in picked + [0]}
    trk = capi.DenseTracker()
    rx, rr, st = trk.map_cloud([pyrs[k] for k in picked], [P[k] for k in picked],
                               [_to8(B[k]) if k % 2 == 0 else None for k in picked], leaf=0.01)
    assert V == st["voxels"] > 1000
    assert rx.tobytes() == xyz.tobytes() and rr.tobytes() == rgb.tobytes()

    # RgbdImage::pointcloud: (x, y, z, 1) of point_cloud at the identity pose
    ex, _ = pyrs[0].point_cloud(tracker=trk)
    assert cols == w * h
    assert pc[:, :3].tobytes() == ex.reshape(-1, 3).tobytes()
    assert np.all(pc[:, 3] == 1.0)
