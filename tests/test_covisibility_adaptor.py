"""The candidate search above the C ABI: dvo_slam::NearestNeighborConstraintSearch (include/dvo_amd/constraints.hpp) in
examples/constraint_search_adaptor_example.cpp and the C99 example examples/constraint_search_example.c.
CPU: both compile against the headers with -Werror (the C++ one as plain C++11 and against the Eigen / OpenCV mocks); the C++
example's radius search runs without a GPU.
GPU: the C++ example prunes by overlap; the C example goes from the search through the proposals to validated constraints."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCKS = os.path.join(ROOT, "tests", "mock_include")  # TEST-ONLY stand-ins for <Eigen/Geometry> and <opencv2/core/core.hpp>


def _compile(kind):
    from dvo_slam_amd import _build

    _build.build()
    exe = os.path.join(ROOT, "examples", "_build", "constraint_search_example_" + kind)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.join(ROOT, "dvo_slam_amd")
    link = ["-o", exe, "-L" + libdir, "-ldvo_amd", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    if kind == "c":
        cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "constraint_search_example.c")] + link
    else:
        cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if kind == "mock" else []) + [
               "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "constraint_search_adaptor_example.cpp")] + link
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


@pytest.mark.parametrize("kind", ["c", "cpp", "mock"])
def test_constraint_search_examples_compile(kind):
    assert os.path.exists(_compile(kind))


@pytest.mark.parametrize("kind", ["cpp", "mock"])
def test_cpp_radius_search_runs_without_a_gpu(kind):
    res = subprocess.run([_compile(kind)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.splitlines() == ["within 1 m: 0 2 4 6 8", "maxDistance 0.05, minOverlap 0.00",
                                       "within 0.05 m of keyframe 4: 2 4 6 8"]


def _gpu():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")


@pytest.mark.gpu
def test_cpp_search_prunes_by_overlap():
    _gpu()
    res = subprocess.run([_compile("cpp"), "overlap"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert lines[:3] == ["within 1 m: 0 2 4 6 8", "maxDistance 0.05, minOverlap 0.00", "within 0.05 m of keyframe 4: 2 4 6 8"]
    assert lines[3] == "within 1 m and overlapping: 0 2 4 6"                 # 8 looks the other way
    overlaps = [float(re.fullmatch(r"  \d+: ([0-9.]+)", l).group(1)) for l in lines[4:]]
    assert len(overlaps) == 4 and overlaps[0] == 1.0 and all(o >= 0.3 for o in overlaps)


@pytest.mark.gpu
def test_c_example_goes_from_the_search_to_validated_constraints():
    _gpu()
    res = subprocess.run([_compile("c")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert lines[0] == "within 1 m of keyframe 0: 0 2 4 6 8"
    assert re.fullmatch(r"\.\.\. of which overlap its view by 0\.3 or more: 0 \(1\.000\) 2 \(\S+\) 4 \(\S+\) 6 \(\S+\)", lines[1]), lines[1]
    n_valid, n_proposals = [int(v) for v in re.fullmatch(r"validated: (\d+) constraints from (\d+) proposals", lines[2]).groups()]
    assert n_proposals == 8 and 1 <= n_valid <= 8 and len(lines) == 3 + n_valid
    assert not any(l.startswith("  0 -> 0:") for l in lines[3:])             # the odometry voter rejects the keyframe itself
