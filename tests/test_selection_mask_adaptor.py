"""Selection masks through the C++ adaptor and from C: examples/masked_selection_adaptor_example.cpp (a user-defined
PointSelectionPredicate as a caller of the reference writes one, evaluated on the host and tracked behind a device mask; and
dvo::core::MaskedGradientThresholdPredicate) and examples/masked_selection_example.c (the C ABI, C99).
CPU: both compile with -Werror.  GPU: both print what the Python binding computes for the equivalent masks."""
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
RECT = (5, 3, 17, 11)  # x0, y0, x1, y1: inside every level of a 160x120 pyramid (level 3 is 20x15)


def _out(name):
    from dvo_slam_amd import _build

    _build.build()
    os.makedirs(os.path.join(ROOT, "examples", "_build"), exist_ok=True)
    return os.path.join(ROOT, "examples", "_build", name)


def _compile_cpp(mocks=False):
    exe = _out("masked_selection_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "masked_selection_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("masked_selection_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "masked_selection_example.c"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_the_c_example_is_plain_c99():
    assert os.path.exists(_compile_c())


@pytest.mark.parametrize("mocks", [False, True])
def test_the_adaptor_example_compiles_as_cxx11_plain_and_against_the_eigen_and_opencv_mocks(mocks):
    assert os.path.exists(_compile_cpp(mocks))


def _lines(stdout, tag=None):
    """{"count": {level: count}, "checksum": float, "isnan": int} of the lines an example printed (tag: their prefix)"""
    counts, checksum, isnan = {}, None, None
    for ln in stdout.strip().splitlines():
        t = ln.split()
        if tag is not None:
            if t[0] != tag:
                continue
            t = t[1:]
        if t[0] == "count":
            counts[int(t[1])] = int(t[2])
        elif t[0] == "checksum":
            checksum, isnan = float(t[1]), int(t[3])
    return {"count": counts, "checksum": checksum, "isnan": isnan}


@pytest.mark.gpu
def test_the_examples_print_what_the_python_binding_computes(tmp_path, small_pair):
    from dvo_slam_amd import capi

    (Ir, Zr), (Ic, Zc), _, K = small_pair
    paths = []
    for name, arr in (("ri", Ir), ("rz", Zr), ("ci", Ic), ("cz", Zc)):
        p = tmp_path / (name + ".f32")
        np.ascontiguousarray(arr, dtype=np.float32).tofile(p)
        paths.append(str(p))
    args = [str(W), str(H)] + [repr(float(k)) for k in K] + paths + [str(v) for v in RECT]
    cpp = subprocess.run([_compile_cpp()] + args, capture_output=True, text=True)
    assert cpp.returncode == 0, cpp.stderr
    c = subprocess.run([_compile_c()] + args, capture_output=True, text=True)
    assert c.returncode == 0, c.stderr

    x0, y0, x1, y1 = RECT
    trk = capi.DenseTracker(capi.Config(FirstLevel=LEVELS - 1, LastLevel=0))
    ref, cur = capi.RgbdImagePyramid(Ir, Zr, K, LEVELS), capi.RgbdImagePyramid(Ic, Zc, K, LEVELS)

    # the user-defined predicate: valid and outside the rectangle, in every level's own pixel coordinates
    planes = []
    for l in range(LEVELS):
        keep = cases.threshold_predicate(ref, l, -1.0, -1.0)
        keep[y0:y1, x0:x1] = 0
        planes.append(keep)
    user = capi.SelectionMask.from_levels(planes)
    want = trk.match(ref, cur, mask=user, thresholds=(-1.0, -1.0))
    got = _lines(cpp.stdout, "user")
    assert got["isnan"] == 0 and not want.isNaN()
    assert got["count"] == {l: ref.select(l, -1.0, -1.0, mask=user)[0] for l in range(LEVELS)}
    assert got["count"] == {l: int(planes[l].sum()) for l in range(LEVELS)}
    assert got["checksum"] == cases.pose_checksum(want.Transformation)  # same library, same points: the same bits (%.17g)

    # MaskedGradientThresholdPredicate with a level-0 mask == the C example == the binding's from_level0
    keep0 = np.ones((H, W), np.uint8)
    keep0[y0:y1, x0:x1] = 0
    m = capi.SelectionMask.from_level0(keep0, LEVELS, capi.MASK_ALL)
    want = trk.match(ref, cur, mask=m)
    masked, from_c = _lines(cpp.stdout, "masked"), _lines(c.stdout)
    assert masked == from_c
    assert sorted(from_c["count"]) == list(range(LEVELS)) and from_c["isnan"] == 0
    assert from_c["count"] == {l: ref.select(l, mask=m)[0] for l in range(LEVELS)}
    assert from_c["checksum"] == cases.pose_checksum(want.Transformation)
    assert from_c["checksum"] != got["checksum"]
