"""The keyframe map above the C ABI: dvo::visualization::KeyframeMap (include/dvo_amd/point_cloud.hpp) in
examples/keyframe_map_adaptor_example.cpp and the C99 example examples/keyframe_map_example.c.
CPU: both compile against the headers with -Werror (the C++ one as plain C++11 and against the Eigen / OpenCV mocks).
GPU: the C example inserts three keyframes, moves one, removes one, compares the map with the rebuild after every event itself
and writes a PCD; the C++ example runs the same verbs through the wrapper."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCKS = os.path.join(ROOT, "tests", "mock_include")  # TEST-ONLY stand-ins for <Eigen/Geometry> and <opencv2/core/core.hpp>


def _compile(kind):
    from dvo_slam_amd import _build

    _build.build()
    exe = os.path.join(ROOT, "examples", "_build", "keyframe_map_example_" + kind)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.join(ROOT, "dvo_slam_amd")
    link = ["-o", exe, "-L" + libdir, "-ldvo_amd", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    if kind == "c":
        cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "keyframe_map_example.c")] + link
    else:
        cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if kind == "mock" else []) + [
               "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "keyframe_map_adaptor_example.cpp")] + link
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


@pytest.mark.parametrize("kind", ["c", "cpp", "mock"])
def test_keyframe_map_examples_compile(kind):
    assert os.path.exists(_compile(kind))


def _gpu():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")


@pytest.mark.gpu
def test_c_example_keeps_the_map_equal_to_the_rebuild(tmp_path):
    _gpu()
    pcd = tmp_path / "map.pcd"
    res = subprocess.run([_compile("c"), str(pcd)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    counts = [int(re.search(r": (\d+) voxels", ln).group(1)) for ln in lines[:6]]
    assert [ln.split()[0].rstrip(":") for ln in lines[:6]] == ["insert", "insert", "insert", "move", "remove", "box"]
    assert 0 < counts[0] < counts[1] < counts[2] and 0 < counts[4] < counts[3] and 0 < counts[5] < counts[4]
    assert lines[-1].endswith("equal to the rebuild after every event: 1")
    blob = open(pcd, "rb").read()
    at = blob.index(b"DATA binary\n") + len(b"DATA binary\n")
    assert ("POINTS %d\n" % counts[4]).encode() in blob[:at] and len(blob) - at == 16 * counts[4]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cpp", "mock"])
def test_cpp_wrapper_runs_the_same_verbs(kind):
    _gpu()
    res = subprocess.run([_compile(kind)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    n = [int(v) for v in re.findall(r"(\d+) (?:points|in the box|voxels)", res.stdout)]
    assert len(n) == 7, res.stdout
    ins0, ins1, ins2, move, rem, box, vox = n
    assert 0 < ins0 < ins1 < ins2 and move > 0 and 0 < box < rem < move and vox == rem
