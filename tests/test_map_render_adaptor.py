"""The map render above the C ABI: dvo::visualization::KeyframeMap::render / renderPyramid (include/dvo_amd/point_cloud.hpp) in
examples/map_render_adaptor_example.cpp and the C99 example examples/map_render_example.c.
CPU: both compile against the headers with -Werror (the C++ one as plain C++11 and against the Eigen / OpenCV mocks).
GPU: the C++ example compares the wrapper's planes and pyramid with the C ABI's output for one view itself; the C example renders
a view between keyframes, builds its pyramid and aligns a live frame to it."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCKS = os.path.join(ROOT, "tests", "mock_include")  # TEST-ONLY stand-ins for <Eigen/Geometry> and <opencv2/core/core.hpp>


def _compile(kind):
    from dvo_slam_amd import _build

    _build.build()
    exe = os.path.join(ROOT, "examples", "_build", "map_render_example_" + kind)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir = os.path.join(ROOT, "dvo_slam_amd")
    link = ["-o", exe, "-L" + libdir, "-ldvo_amd", "-Wl,-rpath," + libdir, "-Wl,--allow-shlib-undefined"]
    if kind == "c":
        cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "map_render_example.c")] + link
    else:
        cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if kind == "mock" else []) + [
               "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
               os.path.join(ROOT, "examples", "map_render_adaptor_example.cpp")] + link
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


@pytest.mark.parametrize("kind", ["c", "cpp", "mock"])
def test_map_render_examples_compile(kind):
    assert os.path.exists(_compile(kind))


def _gpu():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cpp", "mock"])
def test_cpp_wrapper_renders_what_the_c_abi_renders(kind):
    _gpu()
    res = subprocess.run([_compile(kind)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    voxels, drawn, covered = [int(v) for v in re.search(r"render: (\d+) voxels, (\d+) drawn, (\d+) pixels covered", res.stdout).groups()]
    assert 0 < drawn <= voxels and 0.5 * 160 * 120 < covered <= 160 * 120
    assert "pyramid: 3 levels, level 2 is 40 x 30, timestamp 2.5" in res.stdout
    assert res.stdout.splitlines()[-1] == "equal to the C ABI: 1"


@pytest.mark.gpu
def test_c_example_tracks_a_live_frame_against_the_model_view():
    _gpu()
    res = subprocess.run([_compile("c")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    voxels, behind, outside, drawn, covered = [int(v) for v in re.findall(r"(\d+) (?:voxels|behind|outside|drawn|of)", lines[0])]
    assert voxels == behind + outside + drawn and drawn > 0 and covered > 0.5 * 160 * 120
    assert lines[1].startswith("model view") and lines[2].startswith("live frame relative to the model view")
