"""Depth filtering through the C++ adaptor and from C: examples/depth_filter_adaptor_example.cpp
(dvo::core::RgbdImagePyramid::filterDepth) and examples/depth_filter_example.c (the C ABI, C99; both frames in one call).  Each runs
the whole chain once: two frames filtered, the second tracked against the first.  CPU: both compile with -Werror, the adaptor as
plain C++11 and against the Eigen / OpenCV mocks, and where there is no device both run up to the first call that needs one and say
so.  GPU: both print and write what the Python binding computes for the same chain, bit for bit."""
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
OPTIONS = dict(min_support=4, fill_radius=1)  # what both examples set on top of the defaults


def _out(name):
    from dvo_slam_amd import _build

    _build.build()
    os.makedirs(os.path.join(ROOT, "examples", "_build"), exist_ok=True)
    return os.path.join(ROOT, "examples", "_build", name)


def _compile_cpp(mocks=False):
    exe = _out("depth_filter_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "depth_filter_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("depth_filter_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "depth_filter_example.c"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _arguments(tmp_path, synth):
    K = synth.intrinsics_for(W, H)
    frames = [synth.raw_to_float(*synth.sensor_frame(W, H, synth.se3_exp(k * synth.XI_STEP_STREAM), frame_id=k)) for k in range(2)]
    paths = []
    for k, (I, Z) in enumerate(frames):
        for name, arr in (("i", I), ("z", Z)):
            p = tmp_path / f"f{k}{name}.f32"
            np.ascontiguousarray(arr, dtype=np.float32).tofile(p)
            paths.append(str(p))
    return K, frames, [str(W), str(H)] + [repr(float(k)) for k in K] + paths


def test_the_c_example_is_plain_c99():
    assert os.path.exists(_compile_c())


@pytest.mark.parametrize("mocks", [False, True])
def test_the_adaptor_example_compiles_and_runs_as_cxx11_plain_and_against_the_eigen_and_opencv_mocks(tmp_path, synth, mocks):
    """compiled here, and run here as far as a machine without a device lets it: the adaptor turns the library's refusal into a
    DvoAmdError that names the status, and the example ends with it instead of a result"""
    from dvo_slam_amd import capi

    exe = _compile_cpp(mocks)
    assert os.path.exists(exe)
    usage = subprocess.run([exe], capture_output=True, text=True)
    assert usage.returncode == 2 and "usage" in usage.stderr
    if capi.lib().dvo_amd_device_count() == 0:
        _, _, args = _arguments(tmp_path, synth)
        for program in (exe, _compile_c()):
            res = subprocess.run([program] + args + [str(tmp_path / "out.bin")], capture_output=True, text=True)
            assert res.returncode == 1 and "no usable HIP device" in res.stderr, (program, res.returncode, res.stderr)
            assert res.stdout == "" and not os.path.exists(tmp_path / "out.bin")


def _lines(stdout):
    out = {"counts": []}
    for ln in stdout.strip().splitlines():
        t = ln.split()
        if t[:2] == ["filter", "counts"]:
            out["counts"].append([int(v) for v in t[3:]])
        elif t[:2] == ["filtered", "checksum"]:
            out["filtered"] = float(t[2])
        elif t[:2] == ["track", "checksum"]:
            out["track"], out["isnan"] = float(t[2]), int(t[4])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mocks", [False, True])
def test_the_examples_print_and_write_what_the_python_binding_computes(tmp_path, synth, mocks):
    from dvo_slam_amd import capi

    K, frames, args = _arguments(tmp_path, synth)
    cpp_out, c_out = str(tmp_path / "cpp.bin"), str(tmp_path / "c.bin")
    cpp = subprocess.run([_compile_cpp(mocks)] + args + [cpp_out], capture_output=True, text=True)
    assert cpp.returncode == 0, cpp.stderr
    c = subprocess.run([_compile_c()] + args + [c_out], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr

    cfg = capi.Config()
    assert cfg.FirstLevel == LEVELS - 1
    trk = capi.DenseTracker(cfg)
    kf, f1 = [capi.RgbdImagePyramid(I, Z, K, LEVELS) for I, Z in frames]
    (fk, f1f), counts, (support, _) = capi.filter_depth_many([kf, f1], OPTIONS, counts=True, support=True)
    result = trk.match(fk, f1f)

    from_c, from_cpp = _lines(c.stdout), _lines(cpp.stdout)
    assert from_c == from_cpp  # one call for both frames (C) and a call per frame (C++): the same bits
    assert sorted(from_c) == ["counts", "filtered", "isnan", "track"]
    assert from_c["counts"] == [[int(rec[k]) for k in capi.DEPTH_FILTER_COUNTS] for rec in counts]
    assert all(v > 0 for v in from_c["counts"][0])  # kept, dropped and filled pixels: every rule of the filter took part
    depth = fk.plane(0, 1)
    total = 0.0
    for v in depth[np.isfinite(depth)]:  # scan order, as the examples add
        total += float(v)
    assert from_c["filtered"] == total
    assert from_c["isnan"] == 0 and not result.isNaN()
    assert from_c["track"] == cases.pose_checksum(result.Transformation)
    assert from_c["track"] != cases.pose_checksum(trk.match(kf, f1).Transformation)
    blob = depth.tobytes() + support.tobytes()
    assert open(c_out, "rb").read() == blob and open(cpp_out, "rb").read() == blob
