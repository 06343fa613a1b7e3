"""The volume's mesh through the C++ adaptor and from C: examples/volume_mesh_adaptor_example.cpp
(dvo::visualization::SurfaceVolume::extractMesh / upload / writePly) and examples/volume_mesh_example.c (the C ABI, C99).  Each runs
the chain once: two frames tracked, fused into a volume, the volume meshed, its records put into a second volume and meshed again.
CPU: both compile with -Werror, the adaptor also against the mocks.  GPU: both print what the Python binding computes for the
same chain, and the PLY files hold its mesh."""
import os
import subprocess

import numpy as np
import pytest

from test_volume_mesh import read_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCKS = os.path.join(ROOT, "tests", "mock_include")
LIBDIR = os.path.join(ROOT, "dvo_slam_amd")
LINK = ["-L" + LIBDIR, "-ldvo_amd", "-Wl,-rpath," + LIBDIR, "-Wl,--allow-shlib-undefined"]
W, H, LEVELS = 160, 120, 4


@pytest.fixture(autouse=True)
def the_feature():
    """none of these tests passes against a library without the mesh"""
    from dvo_slam_amd import capi

    assert "dvo_amd_volume_mesh" in capi.EXPORTS and hasattr(capi.lib(), "dvo_amd_volume_mesh")


def _out(name):
    from dvo_slam_amd import _build

    _build.build()
    os.makedirs(os.path.join(ROOT, "examples", "_build"), exist_ok=True)
    return os.path.join(ROOT, "examples", "_build", name)


def _compile_cpp(mocks=False):
    exe = _out("volume_mesh_adaptor_example" + ("_mock" if mocks else ""))
    cmd = ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-pthread"] + (["-I" + MOCKS] if mocks else []) + [
        "-I" + os.path.join(ROOT, "include", "dvo_amd_compat"), "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "examples", "volume_mesh_adaptor_example.cpp"), "-o", exe] + LINK
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _compile_c():
    exe = _out("volume_mesh_example")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Wpedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "examples", "volume_mesh_example.c"), "-o", exe] + LINK
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
        if t[:2] == ["mesh", "counts"]:
            out["counts"] = [int(v) for v in t[2:]]
        elif t[:2] == ["mesh", "checksum"]:
            out["x"], out["nz"], out["indices"] = float(t[2]), float(t[3]), int(t[4])
        elif t[:2] == ["restore", "same"]:
            out["same"] = int(t[2])
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
    ply_cpp, ply_c = tmp_path / "adaptor.ply", tmp_path / "c.ply"
    cpp = subprocess.run([_compile_cpp()] + args + [str(ply_cpp)], capture_output=True, text=True)
    assert cpp.returncode == 0, cpp.stderr
    c = subprocess.run([_compile_c()] + args + [str(ply_c)], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr

    trk = capi.DenseTracker(capi.Config())
    first, second = [capi.RgbdImagePyramid(I, Z, K, LEVELS) for I, Z in frames]
    T = trk.match(first, second).Transformation
    vol = capi.SurfaceVolume()
    vol.integrate([first, second], [np.eye(4), T])
    xyz, rgb, normals, tri, cnt = vol.mesh()

    from_c, from_cpp = _lines(c.stdout), _lines(cpp.stdout)
    assert from_c == from_cpp  # same library, same doubles handed over: the same bits (%.17g)
    assert sorted(from_c) == ["counts", "indices", "nz", "same", "x"]
    assert from_c["counts"] == [cnt[n] for n in ("vertices", "triangles", "open_edges", "uncoloured", "flat")]
    assert cnt["vertices"] > 1000 and cnt["triangles"] > 1000
    assert from_c["x"] == _scan_sum(xyz[:, 0]) and from_c["nz"] == _scan_sum(normals[:, 2])
    assert from_c["indices"] == int(tri.astype(np.int64).sum()) and from_c["same"] == 1
    # the PLY files hold the mesh
    assert ply_c.read_bytes() == ply_cpp.read_bytes()
    got = read_ply(str(ply_c))
    assert np.array_equal(got[0].view(np.uint32), xyz.view(np.uint32)) and np.array_equal(got[1].view(np.uint32), normals.view(np.uint32))
    assert np.array_equal(got[3], tri) and np.array_equal(got[2][:, 0], (rgb >> 16) & 255)
    # ... and the normals look back at the camera: the cameras were at z below the surface
    assert from_c["nz"] < 0
