"""Exposure compensation through the C++ adaptor and from C: examples/exposure_adaptor_example.cpp (dvo::core::RgbdImagePyramid::
estimateExposure, ::adjustIntensity, dvo::DenseTracker::matchCompensated) and examples/exposure_example.c (the C ABI, C99).  Each
aligns a current frame whose exposure changed, plain and behind the compensation.  CPU: both compile with -Werror.  GPU: both print
what the Python binding computes for the same chain, and the estimate is the restatement's (tests/exposure_ref.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exposure_ref as er  # noqa: E402
import selection_mask_cases as cases  # noqa: E402

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
    exe = _out("exposure_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "exposure_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("exposure_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "exposure_example.c"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_the_c_example_is_plain_c99():
    assert os.path.exists(_compile_c())


@pytest.mark.parametrize("mocks", [False, True])
def test_the_adaptor_example_compiles_as_cxx11_plain_and_against_the_eigen_and_opencv_mocks(mocks):
    assert os.path.exists(_compile_cpp(mocks))


def _lines(stdout):
    """{first word: {name: value}} of the lines the examples print"""
    out = {}
    for ln in stdout.strip().splitlines():
        t = ln.split()
        out[t[0]] = {t[k]: (float(t[k + 1]) if "." in t[k + 1] or "e" in t[k + 1] or "n" in t[k + 1] else int(t[k + 1])) for k in range(1, len(t), 2)}
    return out


@pytest.mark.gpu
def test_the_examples_print_what_the_python_binding_computes(tmp_path, synth):
    from dvo_slam_amd import capi

    ref, cur, T_gt, K = er.exposure_pair(synth, 0.7, 20.0)
    paths = []
    for tag, arr in (("ri", ref[0]), ("rz", ref[1]), ("ci", cur[0]), ("cz", cur[1])):
        p = tmp_path / f"{tag}.f32"
        np.ascontiguousarray(arr, dtype=np.float32).tofile(p)
        paths.append(str(p))
    args = [str(W), str(H)] + [repr(float(k)) for k in K] + paths
    cpp = subprocess.run([_compile_cpp()] + args, capture_output=True, text=True)
    assert cpp.returncode == 0, cpp.stderr
    c = subprocess.run([_compile_c()] + args, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr

    trk = capi.DenseTracker(capi.Config())
    reference, current = capi.RgbdImagePyramid(ref[0], ref[1], K, LEVELS), capi.RgbdImagePyramid(cur[0], cur[1], K, LEVELS)
    plain = trk.match(reference, current)
    result, estimates, _ = trk.match_compensated(reference, current)
    e = estimates[0].as_dict()
    assert e == er.estimate_ref((ref[0], ref[1], K), (cur[0], cur[1], K))

    from_c, from_cpp = _lines(c.stdout), _lines(cpp.stdout)
    assert from_c == from_cpp  # same library, same doubles handed over: the same integers, the same bits (%.17g)
    assert from_c["plain"] == {"checksum": cases.pose_checksum(plain.Transformation), "isnan": 0}
    assert from_c["estimate"] == {k: e[k] for k in ("gain", "bias", "r2", "passes", "degenerate")}
    assert from_c["counts"] == {k: e[k] for k in ("valid", "consistent", "masked", "saturated", "candidates", "used", "trimmed")}
    assert from_c["sums"] == {k: e[k] for k in er.SUMS}
    assert from_c["compensated"] == {"checksum": cases.pose_checksum(result.Transformation), "isnan": 0}
    assert synth.pose_error(T_gt, result.Transformation) <= 0.5 * synth.pose_error(T_gt, plain.Transformation)
