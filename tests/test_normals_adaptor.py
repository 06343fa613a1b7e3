"""Surface normals through the C++ adaptor and from C: examples/normals_adaptor_example.cpp (RgbdImage::calculateNormals, normals,
angles; dvo::core::SelectionMask::fromNormals; BuildJob::buildWithNormals) and examples/normals_example.c (the C ABI, C99).  Each
runs the chain once: the reference's normal planes, a facing mask over every level, the mask eroded, the next frame tracked behind
it, the cloud with normals.  CPU: both compile with -Werror, the adaptor as plain C++11 and against the Eigen / OpenCV mocks.
GPU: both print and write what the Python binding computes for the same chain, bit for bit."""
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
RADII = (3, 2, 1, 0)


def _out(name):
    from dvo_slam_amd import _build

    _build.build()
    os.makedirs(os.path.join(ROOT, "examples", "_build"), exist_ok=True)
    return os.path.join(ROOT, "examples", "_build", name)


def _compile_cpp(mocks=False):
    exe = _out("normals_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "normals_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("normals_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "normals_example.c"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_the_c_example_is_plain_c99():
    assert os.path.exists(_compile_c())


@pytest.mark.parametrize("mocks", [False, True])
def test_the_adaptor_example_compiles_as_cxx11_plain_and_against_the_eigen_and_opencv_mocks(mocks):
    assert os.path.exists(_compile_cpp(mocks))


def _lines(stdout):
    out = {"mask": [], "eroded": []}
    for ln in stdout.strip().splitlines():
        t = ln.split()
        if t[:2] == ["normals", "counts"]:
            out["normals"] = [int(v) for v in t[2:]]
        elif t[:2] == ["mask", "counts"]:
            out["mask"].append([int(v) for v in t[3:]])
        elif t[:2] == ["eroded", "kept"]:
            out["eroded"].append(int(t[3]))
        elif t[:2] == ["track", "checksum"]:
            out["track"], out["isnan"] = float(t[2]), int(t[4])
        elif t[:2] == ["cloud", "points"]:
            out["cloud"] = int(t[2])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mocks", [False, True])
def test_the_examples_print_and_write_what_the_python_binding_computes(tmp_path, synth, mocks):
    from dvo_slam_amd import capi

    K = synth.intrinsics_for(W, H)
    frames = [synth.raw_to_float(*synth.sensor_frame(W, H, synth.se3_exp(k * synth.XI_STEP_STREAM), frame_id=k)) for k in range(2)]
    paths = []
    for k, (I, Z) in enumerate(frames):
        for name, arr in (("i", I), ("z", Z)):
            p = tmp_path / f"f{k}{name}.f32"
            np.ascontiguousarray(arr, dtype=np.float32).tofile(p)
            paths.append(str(p))
    args = [str(W), str(H)] + [repr(float(k)) for k in K] + paths
    cpp_out, c_out, pcd = str(tmp_path / "cpp.bin"), str(tmp_path / "c.bin"), str(tmp_path / "cloud.pcd")
    cpp = subprocess.run([_compile_cpp(mocks)] + args + [cpp_out], capture_output=True, text=True)
    assert cpp.returncode == 0, cpp.stderr
    c = subprocess.run([_compile_c()] + args + [c_out, pcd], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr

    cfg = capi.Config()
    assert cfg.FirstLevel == LEVELS - 1
    trk = capi.DenseTracker(cfg)
    kf, f1 = [capi.RgbdImagePyramid(I, Z, K, LEVELS) for I, Z in frames]
    normals, angles, counts = kf.normals(0)  # the default options: what RgbdImage::normals / angles hold
    opt = dict(radius=RADII, depth_step_ratio=0.02, facing=capi.NORMAL_FACING_RAY, toward_camera=1)
    mask, mask_counts = capi.SelectionMask.from_normals(kf, 0.5, opt, counts=True)
    eroded = mask.erode(1)
    result = trk.match(kf, f1, mask=eroded)
    xyz, rgb, cloud_normals = kf.point_cloud(normals=opt, tracker=trk)

    from_c, from_cpp = _lines(c.stdout), _lines(cpp.stdout)
    assert from_c == from_cpp
    assert sorted(from_c) == ["cloud", "eroded", "isnan", "mask", "normals", "track"]
    assert from_c["normals"] == [counts["defined"], counts["undefined"]] and counts["undefined"] > 0
    assert from_c["mask"] == [[int(v) for v in rec] for rec in mask_counts]
    assert from_c["eroded"] == eroded.info()["kept"] and all(0 < k for k in from_c["eroded"])
    assert from_c["isnan"] == 0 and not result.isNaN()
    assert from_c["track"] == cases.pose_checksum(result.Transformation)
    assert from_c["cloud"] == W * H

    planes = normals.tobytes() + angles.tobytes() + b"".join(mask.download(l).tobytes() for l in range(LEVELS))
    c_blob, cpp_blob = open(c_out, "rb").read(), open(cpp_out, "rb").read()
    assert c_blob == planes                                   # RgbdImage::normals / angles == the C entry with default options,
    assert cpp_blob[:len(planes)] == planes                   # fromNormals == dvo_amd_mask_from_normals
    assert cpp_blob[len(planes):] == np.ascontiguousarray(cloud_normals[..., :3]).tobytes()
    # the C example's PCD file: the header, then x y z rgb normal_x normal_y normal_z curvature per point
    blob = open(pcd, "rb").read()
    head, _, body = blob.partition(b"DATA binary\n")
    assert b"FIELDS x y z rgb normal_x normal_y normal_z curvature\n" in head and (b"WIDTH %d\nHEIGHT %d\n" % (W, H)) in head
    rec = np.frombuffer(body, np.uint32).reshape(W * H, 8)
    assert rec[:, :3].tobytes() == xyz.reshape(-1, 3).tobytes() and rec[:, 3].tobytes() == rgb.reshape(-1).tobytes()
    assert rec[:, 4:7].tobytes() == np.ascontiguousarray(cloud_normals.reshape(-1, 4)[:, :3]).tobytes() and not rec[:, 7].any()
