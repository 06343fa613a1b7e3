"""Mask components through the C++ adaptor and from C: examples/mask_components_adaptor_example.cpp
(dvo::core::SelectionMask::filterComponents, ::reconstruct, ::components, ::depthComponents) and examples/mask_components_example.c
(the C ABI, C99).  Each runs the whole chain once: match, inlier mask, erode, reconstruct from the eroded seeds, warp to the next
keyframe, masked match -- and a depth despeckle.  CPU: both compile with -Werror, the adaptor example also against the Eigen and
OpenCV mocks.  GPU: both print what the Python binding computes for the same chain."""
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
TAGS = ("inliers", "eroded", "reconstructed", "warped", "despeckled")


def _out(name):
    from dvo_slam_amd import _build

    _build.build()
    os.makedirs(os.path.join(ROOT, "examples", "_build"), exist_ok=True)
    return os.path.join(ROOT, "examples", "_build", name)


def _compile_cpp(mocks=False):
    exe = _out("mask_components_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "mask_components_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("mask_components_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "mask_components_example.c"), "-o", exe] + LINK
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


def stream_with_an_object(synth):
    """three frames of a short stream; an object is planted into frame 1 only (a rectangle pushed 30 % farther, its intensity
    inverted): the match against the keyframe down-weights it, the inlier mask drops it"""
    frames = [synth.render(W, H, synth.se3_exp(0.5 * k * synth.XI_GT_PAIR), frame_id=k) for k in range(3)]
    I, Z = frames[1][0].copy(), frames[1][1].copy()
    y0, y1, x0, x1 = H // 3, H // 3 + H // 4, W // 2, W // 2 + W // 4
    Z[y0:y1, x0:x1] *= np.float32(1.3)
    I[y0:y1, x0:x1] = np.float32(255.0) - I[y0:y1, x0:x1]
    frames[1] = (I, Z)
    return frames, (y0, y1, x0, x1)


@pytest.mark.gpu
def test_the_examples_print_what_the_python_binding_computes(tmp_path, synth):
    from dvo_slam_amd import capi

    K = synth.intrinsics_for(W, H)
    frames, (y0, y1, x0, x1) = stream_with_an_object(synth)
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

    cfg = capi.Config()  # the default configuration: level 0 is not run and takes level 1's precision
    assert cfg.FirstLevel == LEVELS - 1 and cfg.LastLevel == 1
    trk = capi.DenseTracker(cfg)
    kf, f1, f2 = [capi.RgbdImagePyramid(I, Z, K, LEVELS) for I, Z in frames]
    first = trk.match(kf, f1)
    masks = {"inliers": capi.SelectionMask.from_residuals(trk, kf, f1, result=first)}
    masks["eroded"] = masks["inliers"].erode(1)
    masks["reconstructed"] = masks["inliers"].reconstruct(masks["eroded"])
    masks["warped"] = masks["reconstructed"].warp(kf, f1, first.Transformation)
    masks["despeckled"] = f1.depth_components(min_area=capi.level_areas(10, LEVELS))
    result = trk.match(f1, f2, mask=masks["warped"])

    from_c, from_cpp = _lines(c.stdout), _lines(cpp.stdout)
    assert from_c == from_cpp  # same library, same doubles handed over: the same bits (%.17g)
    assert sorted(from_c) == sorted(TAGS + ("track",))
    for tag in TAGS:
        assert from_c[tag]["kept"] == dict(enumerate(masks[tag].info()["kept"])), tag
    kept = {tag: masks[tag].info()["kept"] for tag in TAGS}
    # the reconstruction lies between the erosion and the mask: it restores the rims and leaves the speckle out
    assert all(0 < kept["eroded"][l] <= kept["reconstructed"][l] <= kept["inliers"][l] for l in range(LEVELS))
    assert kept["eroded"][0] < kept["reconstructed"][0] < kept["inliers"][0]
    assert 0 < kept["despeckled"][0] <= int(np.isfinite(frames[1][1]).sum())
    assert from_c["track"]["isnan"] == 0 and not result.isNaN()
    assert from_c["track"]["checksum"] == cases.pose_checksum(result.Transformation)
    assert from_c["track"]["checksum"] != cases.pose_checksum(trk.match(f1, f2).Transformation)
    # the planted object is what the mask drops: inside its rectangle fewer pixels of the keyframe are kept than outside
    plane = masks["inliers"].download(0)
    inside = np.zeros_like(plane, bool)
    inside[y0:y1, x0:x1] = True
    assert plane[inside].mean() < plane[~inside].mean()
