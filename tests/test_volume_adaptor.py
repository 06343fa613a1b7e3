"""The signed-distance volume through the C++ adaptor and from C: examples/volume_adaptor_example.cpp
(dvo::visualization::SurfaceVolume) and examples/volume_example.c (the C ABI, C99).  Each runs the chain once: two frames tracked,
fused into a volume, the volume raycast, its surface pulled, the second frame tracked against the model view.  CPU: both compile
with -Werror, the adaptor also against the mocks.  GPU: both print what the Python binding computes for the same chain."""
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
    exe = _out("volume_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "volume_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("volume_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "volume_example.c"), "-o", exe] + LINK
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
        if t[:2] == ["insert", "counts"]:
            out["insert"] = [int(v) for v in t[2:]]
        elif t[:2] == ["raycast", "stats"]:
            out["stats"] = [int(v) for v in t[2:]]
        elif t[:2] == ["raycast", "checksum"]:
            out["raycast"] = float(t[2])
        elif t[:2] == ["extract", "counts"]:
            out["extract"], out["surface"] = [int(t[2]), int(t[3])], float(t[5])
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
    poses = [synth.se3_exp(3 * k * synth.XI_STEP_STREAM) for k in range(2)]
    frames = []
    for k in range(2):
        grey, raw = synth.sensor_frame(W, H, poses[k], frame_id=k)
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
    pcd = tmp_path / "surface.pcd"
    c = subprocess.run([_compile_c()] + args + [str(pcd)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr

    cfg = capi.Config()
    assert cfg.FirstLevel == LEVELS - 1
    trk = capi.DenseTracker(cfg)
    first, second = [capi.RgbdImagePyramid(I, Z, K, LEVELS) for I, Z in frames]
    T = trk.match(first, second).Transformation
    vol = capi.SurfaceVolume()
    counts = vol.insert([0, 1], [first, second], [np.eye(4), T])
    view = vol.raycast(np.eye(4), K, W, H, planes=("depth",))
    xyz, rgb, ec = vol.extract()
    model = vol.raycast_pyramid(np.eye(4), K, W, H, LEVELS, timestamp=2.0)
    result = trk.match(model, second)

    from_c, from_cpp = _lines(c.stdout), _lines(cpp.stdout)
    assert from_c == from_cpp  # same library, same doubles handed over: the same bits (%.17g)
    assert sorted(from_c) == ["extract", "insert", "isnan", "raycast", "stats", "surface", "track"]
    assert from_c["insert"] == [int(counts[k][f]) for k in range(2) for f in capi.VOLUME_COUNTS]
    assert from_c["stats"] == [view["stats"][f] for f in ("pixels", "hit", "backface", "missed", "uncoloured")]
    assert from_c["stats"][1] > 0.5 * W * H
    d = view["depth"].ravel()
    assert from_c["raycast"] == _scan_sum(d[~np.isnan(d)])
    assert from_c["extract"] == [ec["points"], ec["uncoloured"]] and ec["points"] == len(xyz) > 1000
    assert from_c["surface"] == _scan_sum(xyz[:, 0])
    assert from_c["isnan"] == 0 and not result.isNaN()
    assert from_c["track"] == cases.pose_checksum(result.Transformation)
    # the PCD file holds the extracted points
    blob = pcd.read_bytes()
    at = blob.index(b"DATA binary\n") + len(b"DATA binary\n")
    assert b"POINTS %d\n" % len(xyz) in blob[:at]
    stored = np.frombuffer(blob[at:], np.float32).reshape(-1, 4)
    assert np.array_equal(stored[:, :3].view(np.uint32), xyz.view(np.uint32)) and np.array_equal(stored[:, 3].view(np.uint32), rgb)
    # the model view is a reference the tracker accepts: it finds the motion the frame-to-frame match found
    assert synth.pose_error(result.Transformation, T) < 0.5 * synth.pose_error(np.eye(4), T)
