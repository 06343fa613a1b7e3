"""Point-budget masks through the C++ adaptor and from C: examples/budget_selection_adaptor_example.cpp
(dvo::core::SelectionMask::topK / ::grid behind a MaskedGradientThresholdPredicate) and examples/budget_selection_example.c
(the C ABI, C99).  CPU: both compile with -Werror.  GPU: both print what the Python binding computes for the same budgets."""
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
K0, CELL = 6000, 3


def _out(name):
    from dvo_slam_amd import _build

    _build.build()
    os.makedirs(os.path.join(ROOT, "examples", "_build"), exist_ok=True)
    return os.path.join(ROOT, "examples", "_build", name)


def _compile_cpp(mocks=False):
    exe = _out("budget_selection_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "budget_selection_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("budget_selection_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "budget_selection_example.c"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_the_c_example_is_plain_c99():
    assert os.path.exists(_compile_c())


@pytest.mark.parametrize("mocks", [False, True])
def test_the_adaptor_example_compiles_as_cxx11_plain_and_against_the_eigen_and_opencv_mocks(mocks):
    assert os.path.exists(_compile_cpp(mocks))


def _lines(stdout):
    """{tag: {"kept": {level: count}, "checksum": float, "isnan": int}} of the lines an example printed"""
    out = {}
    for ln in stdout.strip().splitlines():
        t = ln.split()
        entry = out.setdefault(t[0], {"kept": {}, "checksum": None, "isnan": None})
        if t[1] == "kept":
            entry["kept"][int(t[2])] = int(t[3])
        elif t[1] == "checksum":
            entry["checksum"], entry["isnan"] = float(t[2]), int(t[4])
    return out


@pytest.mark.gpu
def test_the_examples_print_what_the_python_binding_computes(tmp_path, small_pair):
    from dvo_slam_amd import capi

    (Ir, Zr), (Ic, Zc), _, K = small_pair
    paths = []
    for name, arr in (("ri", Ir), ("rz", Zr), ("ci", Ic), ("cz", Zc)):
        p = tmp_path / (name + ".f32")
        np.ascontiguousarray(arr, dtype=np.float32).tofile(p)
        paths.append(str(p))
    args = [str(W), str(H)] + [repr(float(k)) for k in K] + paths + [str(K0), str(CELL)]
    cpp = subprocess.run([_compile_cpp()] + args, capture_output=True, text=True)
    assert cpp.returncode == 0, cpp.stderr
    c = subprocess.run([_compile_c()] + args, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr

    cfg = capi.Config(FirstLevel=LEVELS - 1, LastLevel=0)
    thresholds = (cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold)
    trk = capi.DenseTracker(cfg)
    ref, cur = capi.RgbdImagePyramid(Ir, Zr, K, LEVELS), capi.RgbdImagePyramid(Ic, Zc, K, LEVELS)
    topk = capi.SelectionMask.from_budget(ref, capi.BUDGET_TOPK, budget=capi.level_budgets(K0, LEVELS), thresholds=thresholds)
    grid = capi.SelectionMask.from_budget(ref, capi.BUDGET_GRID, cell=CELL, thresholds=thresholds)
    want = {"plain": {"kept": {}, "result": trk.match(ref, cur)}}
    for tag, mask in (("topk", topk), ("grid", grid)):
        want[tag] = {"kept": dict(enumerate(mask.info()["kept"])), "result": trk.match(ref, cur, mask=mask)}
    assert want["topk"]["kept"] == {l: K0 >> (2 * l) for l in range(LEVELS)}  # (the pair has more candidates than that)
    from_c, from_cpp = _lines(c.stdout), _lines(cpp.stdout)
    assert from_c == from_cpp  # same library, same points: the same bits (%.17g)
    assert sorted(from_c) == ["grid", "plain", "topk"]
    for tag, w in want.items():
        assert from_c[tag]["kept"] == w["kept"], tag
        assert from_c[tag]["isnan"] == 0 and not w["result"].isNaN(), tag
        assert from_c[tag]["checksum"] == cases.pose_checksum(w["result"].Transformation), tag
    assert len({from_c[tag]["checksum"] for tag in from_c}) == 3
