"""Depth fusion through the C++ adaptor and from C: examples/depth_fusion_adaptor_example.cpp
(dvo::core::RgbdImagePyramid::fuseDepth) and examples/depth_fusion_example.c (the C ABI, C99).  Each runs the whole chain once:
three frames tracked against a keyframe, fused into it, a fourth frame tracked against the fused keyframe.  CPU: both compile with
-Werror.  GPU: both print what the Python binding computes for the same chain."""
import os
import subprocess

import numpy as np
import pytest

import selection_mask_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCKS = os.path.join(ROOT, "tests", "mock_include")
LIBDIR = os.path.join(ROOT, "dvo_slam_amd")
LINK = ["-L" + LIBDIR, "-ldvo_amd", "-Wl,-rpath," + LIBDIR, "-Wl,--allow-shlib-undefined"]
W, H, LEVELS = 160, 120, 4


def _out(name):
    from dvo_slam_amd import _build

    _build.build()
    os.makedirs(os.path.join(ROOT, "examples", "_build"), exist_ok=True)
    return os.path.join(ROOT, "examples", "_build", name)


def _compile_cpp(mocks=False):
    exe = _out("depth_fusion_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "depth_fusion_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("depth_fusion_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "depth_fusion_example.c"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_the_c_example_is_plain_c99():
    assert os.path.exists(_compile_c())


@pytest.mark.parametrize("mocks", [False, True])
def test_the_adaptor_example_compiles_as_cxx11_plain_and_against_the_eigen_and_opencv_mocks(mocks):
    assert os.path.exists(_compile_cpp(mocks))


def _lines(stdout):
    """{"counts": [4 ints], "fused": float, "track": float, "isnan": int} of the lines an example printed"""
    out = {}
    for ln in stdout.strip().splitlines():
        t = ln.split()
        if t[:2] == ["fused", "counts"]:
            out["counts"] = [int(v) for v in t[2:]]
        elif t[:2] == ["fused", "checksum"]:
            out["fused"] = float(t[2])
        elif t[:2] == ["track", "checksum"]:
            out["track"], out["isnan"] = float(t[2]), int(t[4])
    return out


@pytest.mark.gpu
def test_the_examples_print_what_the_python_binding_computes(tmp_path, synth):
    from dvo_slam_amd import capi

    K = synth.intrinsics_for(W, H)
    frames = []
    for k in range(5):
        grey, raw = synth.sensor_frame(W, H, synth.se3_exp(k * synth.XI_STEP_STREAM), frame_id=k)
        frames.append(synth.raw_to_float(grey, raw))
    paths = []
    for k, (I, Z) in enumerate(frames):
        for name, arr in (("i", I), ("z", Z)):
            p = tmp_path / f"f{k}{name}.f32"
            np.ascontiguousarray(arr, dtype=np.float32).tofile(p)
            paths.append(str(p))
    args = [str(W), str(H)] + [repr(float(k)) for k in K] + paths
    cpp = subprocess.run([_compile_cpp()] + args, capture_output=True, text=True)
    assert cpp.returncode == 0, cpp.stderr
    c = subprocess.run([_compile_c()] + args, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr

    cfg = capi.Config()
    assert cfg.FirstLevel == LEVELS - 1
    trk = capi.DenseTracker(cfg)
    kf, f1, f2, f3, f4 = [capi.RgbdImagePyramid(I, Z, K, LEVELS) for I, Z in frames]
    Ts = [trk.match(kf, f).Transformation for f in (f1, f2, f3)]
    fused, _, counts = kf.fuse_depth([f1, f2, f3], Ts, counts=True)
    result = trk.match(fused, f4)

    from_c, from_cpp = _lines(c.stdout), _lines(cpp.stdout)
    assert from_c == from_cpp  # same library, same doubles handed over: the same bits (%.17g)
    assert sorted(from_c) == ["counts", "fused", "isnan", "track"]
    assert from_c["counts"] == [int(counts[k]) for k in capi.FUSE_KEYFRAME_COUNTS]
    assert from_c["counts"][0] == from_c["counts"][1] == int(np.isfinite(frames[0][1]).sum())
    depth = fused.plane(0, 1)
    total = 0.0
    for v in depth[np.isfinite(depth)]:  # scan order, as the examples add
        total += float(v)
    assert from_c["fused"] == total
    assert from_c["isnan"] == 0 and not result.isNaN()
    assert from_c["track"] == cases.pose_checksum(result.Transformation)
    assert from_c["track"] != cases.pose_checksum(trk.match(kf, f4).Transformation)
