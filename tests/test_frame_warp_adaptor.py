"""Frame warps through the C++ adaptor and from C: examples/frame_warp_adaptor_example.cpp
(dvo::core::RgbdImagePyramid::warpInverse, ::warpForward) and examples/frame_warp_example.c (the C ABI, C99).  Each runs the chain
once: a frame tracked against another, warped onto its pixels in both directions, the warped pyramid tracked again.  CPU: both
compile with -Werror.  GPU: both print what the Python binding computes for the same chain."""
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
    exe = _out("frame_warp_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "frame_warp_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("frame_warp_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "frame_warp_example.c"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_the_c_example_is_plain_c99():
    assert os.path.exists(_compile_c())


@pytest.mark.parametrize("mocks", [False, True])
def test_the_adaptor_example_compiles_as_cxx11_plain_and_against_the_eigen_and_opencv_mocks(mocks):
    assert os.path.exists(_compile_cpp(mocks))


def _lines(stdout):
    """what an example printed: the counts as ints, the checksums as floats"""
    out = {}
    for ln in stdout.strip().splitlines():
        t = ln.split()
        if t[1] == "counts":
            out[t[0] + "_counts"] = [int(v) for v in t[2:]]
        elif t[:2] == ["inverse", "checksum"]:
            out["inverse"] = float(t[2])
        elif t[:2] == ["forward", "checksum"]:
            out["forward"], out["index"] = float(t[2]), int(t[3])
        elif t[:2] == ["track", "checksum"]:
            out["track"], out["isnan"] = float(t[2]), int(t[4])
    return out


def _scan_sum(values):
    total = 0.0
    for v in values:  # scan order, as the examples add
        total += float(v)
    return total


@pytest.mark.gpu
def test_the_examples_print_what_the_python_binding_computes(tmp_path, synth):
    from dvo_slam_amd import capi

    K = synth.intrinsics_for(W, H)
    frames = []
    for k in range(2):
        grey, raw = synth.sensor_frame(W, H, synth.se3_exp(3 * k * synth.XI_STEP_STREAM), frame_id=k)
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
    fixed, moving = [capi.RgbdImagePyramid(I, Z, K, LEVELS) for I, Z in frames]
    T = trk.match(fixed, moving).Transformation
    I, Z, ic = moving.warp_inverse(fixed, T, 0)
    d, i, x, fc = moving.warp_forward(T, None, 0, dict(splat=capi.WARP_SPLAT_FOOTPRINT))
    warped, _ = moving.warp_inverse(fixed, T, options=dict(depth=capi.WARP_DEPTH_FIXED))
    result = trk.match(fixed, warped)

    from_c, from_cpp = _lines(c.stdout), _lines(cpp.stdout)
    assert from_c == from_cpp  # same library, same doubles handed over: the same bits (%.17g)
    assert sorted(from_c) == ["forward", "forward_counts", "index", "inverse", "inverse_counts", "isnan", "track"]
    assert from_c["inverse_counts"] == [int(ic[k]) for k in capi.WARP_INVERSE_COUNTS]
    assert from_c["forward_counts"] == [int(fc[k]) for k in capi.WARP_FORWARD_COUNTS]
    assert from_c["inverse_counts"][5] > 0.8 * W * H and from_c["forward_counts"][5] > 0.8 * W * H
    assert from_c["inverse"] == _scan_sum(I[~np.isnan(I)])
    assert from_c["forward"] == _scan_sum(d[x >= 0]) and from_c["index"] == int(x[x >= 0].astype(np.int64).sum())
    assert from_c["isnan"] == 0 and not result.isNaN()
    assert from_c["track"] == cases.pose_checksum(result.Transformation)
    # The warped pyramid holds the moving frame's grey values on the fixed frame's pixels and, with WARP_DEPTH_FIXED, the fixed
    # frame's own depth there: against the fixed frame its depth residual is zero and its grey residual is the sensor's noise, so
    # what is left of the motion is smaller than the motion
    assert synth.pose_error(np.eye(4), result.Transformation) < synth.pose_error(np.eye(4), T)
