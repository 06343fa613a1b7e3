"""The place index through the C++ adaptor and from C: examples/place_index_adaptor_example.cpp
(dvo_slam::AppearanceConstraintSearch, include/dvo_amd/constraints.hpp) and examples/place_index_example.c (the C ABI, C99).  Each
builds an index of six keyframes, asks for the keyframes that look like keyframe 0 and like a frame that is no keyframe, and prints
ids, scores and dots.  CPU: both compile with -Werror.  GPU: both print what the Python binding computes for the same inputs."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCKS = os.path.join(ROOT, "tests", "mock_include")
LIBDIR = os.path.join(ROOT, "dvo_slam_amd")
LINK = ["-L" + LIBDIR, "-ldvo_amd", "-Wl,-rpath," + LIBDIR, "-Wl,--allow-shlib-undefined"]
W, H, LEVELS, KEYFRAMES = 160, 120, 4, 6


def _out(name):
    from dvo_slam_amd import _build

    _build.build()
    os.makedirs(os.path.join(ROOT, "examples", "_build"), exist_ok=True)
    return os.path.join(ROOT, "examples", "_build", name)


def _compile_cpp(mocks=False):
    exe = _out("place_index_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "place_index_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("place_index_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "place_index_example.c"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_the_c_example_is_plain_c99():
    assert os.path.exists(_compile_c())


@pytest.mark.parametrize("mocks", [False, True])
def test_the_adaptor_example_compiles_as_cxx11_plain_and_against_the_eigen_and_opencv_mocks(mocks):
    assert os.path.exists(_compile_cpp(mocks))


def _found(line):
    """[(id, score)] of a line `what: id:score id:score ...`"""
    return [(int(t.split(":")[0]), float(t.split(":")[1])) for t in line.split(": ", 1)[1].split()] if ": " in line else []


@pytest.mark.gpu
def test_the_examples_print_what_the_python_binding_computes(tmp_path, synth):
    from dvo_slam_amd import capi

    K = synth.intrinsics_for(W, H)
    poses = synth.stream_poses(KEYFRAMES)
    frames = []
    for k in range(KEYFRAMES):
        grey, raw = synth.sensor_frame(W, H, poses[k], frame_id=k)
        frames.append(synth.raw_to_float(grey, raw))
    grey, raw = synth.sensor_frame(W, H, poses[2] @ synth.se3_exp(0.3 * synth.XI_STEP_STREAM), frame_id=50)
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
    assert c.stdout == cpp.stdout  # same library, same inputs: the same ids, dots and doubles (%.17g)

    pyramids = [capi.RgbdImagePyramid(I, Z, K, LEVELS) for I, Z in frames]
    index = capi.PlaceIndex()
    assert index.add(pyramids[:KEYFRAMES]) == range(0, KEYFRAMES)
    info = index.info()
    lines = c.stdout.strip().splitlines()
    assert lines[0] == f"index size {KEYFRAMES} dim {info['dim']} first 0" and info["dim"] == 320
    cand, score, counts = index.query([0], k=3)
    assert counts[0] == 3 and _found(lines[1]) == list(zip(cand[0].tolist(), score[0].tolist())) and lines[1].startswith("keyframe 0: ")
    cand, score, counts = index.query_frames([pyramids[KEYFRAMES]], k=3)
    assert counts[0] == 3 and _found(lines[2]) == list(zip(cand[0].tolist(), score[0].tolist())) and lines[2].startswith("frame: ")
    assert cand[0, 0] == 2  # the frame was taken next to keyframe 2
    assert lines[3] == "dots: " + " ".join(str(v) for v in index.scores([0])[0].tolist())
    assert len(lines) == 4
