"""The volume's surface as an indexed triangle mesh (include/dvo_amd.h, "The mesh"): dvo_amd_volume_mesh, and with it
dvo_amd_volume_upload (the inverse of download) and dvo_amd_write_ply.  The rule is pinned in the header and restated twice in
tests/volume_mesh_ref.py.  Every comparison with the library is equality -- counts and indices as integers, coordinates and
normals on their bit patterns.  The inequalities are properties of the rule on a sphere and a torus (closed, oriented, on the
surface), not of the library.
CPU: exports, argument checks that need no device, the two restatements against each other on the solids and on crafted cases
that assert they hit their case, triangles/2 + open_edges == extract's points, the PLY file.  GPU: the library against the
restatement."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volume_mesh_ref as mref  # noqa: E402
import volume_ref as ref  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_volume_mesh", "dvo_amd_volume_upload", "dvo_amd_write_ply"]
INVALID, NO_DEVICE, CAPACITY, IO = 1, 2, 7, 11
W, H = 64, 48
ROOM = dict(nx=64, ny=52, nz=56, voxel=0.05, origin=(-1.7, -1.35, 0.4), trunc=0.15, near_z=0.4, far_z=5.0)
SHAPES = [dict(nx=70, ny=5, nz=3, voxel=0.05, origin=(-1.7, 0.9, 2.9), trunc=0.15, near_z=0.4, far_z=5.0),
          dict(nx=2, ny=2, nz=2, voxel=0.05, origin=(0.0, 0.0, 2.975), trunc=0.15, near_z=0.4, far_z=5.0),
          dict(nx=12, ny=10, nz=8, voxel=0.1, origin=(-0.5, -0.4, 2.55), trunc=0.2, near_z=0.4, far_z=3.0)]
COUNT_NAMES = ("vertices", "triangles", "open_edges", "uncoloured", "flat")


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(a, b):
    return a.dtype == b.dtype == F and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_mesh(a, b):
    """(xyz, rgb, normals, triangles, counts) twice: the same bits, the same integers"""
    return (same_bits(a[0], b[0]) and a[1].dtype == b[1].dtype and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2])
            and a[3].dtype == b[3].dtype == np.int32 and a[3].shape == b[3].shape and np.array_equal(a[3], b[3]) and a[4] == b[4])


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


@pytest.fixture(autouse=True)
def the_feature(capi):
    """every test of this file is about the mesh, the upload or the PLY writer: none passes against a library without them"""
    assert all(name in capi.EXPORTS and hasattr(capi.lib(), name) for name in NEW_SYMBOLS)
    assert hasattr(capi.SurfaceVolume, "mesh") and hasattr(capi.SurfaceVolume, "upload")


# ---- the inputs: records made in numpy ---------------------------------------------------------------------------------------------

GRID = dict(nx=14, ny=14, nz=14, voxel=0.1, origin=(-0.65, -0.65, -0.65), trunc=0.2, near_z=0.4, far_z=5.0, weight=ref.CONSTANT)
SPHERE_C, SPHERE_R = (0.03, -0.02, 0.01), 0.45
TORUS_R, TORUS_r = 0.4, 0.17


def from_distance(opt, d):
    """weight-1 records of a signed distance d [nz, ny, nx] (metres, positive outside): q = rint(clip(d/trunc, -1, 1)*2047); the
    grey value varies with the position"""
    rec = ref.empty(opt)
    q = np.rint(np.clip(d / float(opt.trunc), -1.0, 1.0) * 2047.0).astype(np.int64)
    iz, iy, ix = np.meshgrid(np.arange(opt.nz), np.arange(opt.ny), np.arange(opt.nx), indexing="ij")
    rec[..., 0] = 1
    rec[..., 1] = q & 0xFFFFFFFF
    rec[..., 2] = 1
    rec[..., 3] = 400 + 200 * ix + 30 * iy + 7 * iz
    return rec


def grid_points(opt):
    iz, iy, ix = np.meshgrid(np.arange(opt.nz), np.arange(opt.ny), np.arange(opt.nx), indexing="ij")
    o, v = opt.origin.astype(np.float64), float(opt.voxel)
    return o[0] + ix * v, o[1] + iy * v, o[2] + iz * v


def signs(opt, inside, weights=None, colour=None):
    """records with F = -1000/2047*... inside and +1000 outside: sd_sum = -/+1000 at weight 1; weights / colour: arrays that
    replace w_sum (sd_sum scales with it) and iw_sum"""
    rec = ref.empty(opt)
    w = np.ones(inside.shape, np.int64) if weights is None else np.asarray(weights, np.int64)
    rec[..., 0] = w
    rec[..., 1] = (np.where(inside, -1000, 1000) * w) & 0xFFFFFFFF
    rec[..., 2] = 1 if colour is None else colour
    rec[..., 3] = 1600 * rec[..., 2]
    return rec


def slab_volume(values, weights=None, grey=None, n=6):
    """(a copy of tests/test_volume.py's helper) records of an n x n x len(values) volume whose signed distance depends on z
    alone: F = values[iz] (in q / 2047 units of a weight-1 observation); weights[iz] = 0 leaves the slab unobserved"""
    opt = ref.Options(n, n, len(values), 0.25, (-0.5, -0.5, 1.0), 0.25, 0.5, 4.0, ref.CONSTANT)
    rec = ref.empty(opt)
    for iz, v in enumerate(values):
        w = 1 if weights is None else weights[iz]
        g = 1600 if grey is None else grey[iz]
        rec[iz, :, :, 0] = w
        rec[iz, :, :, 1] = np.int64(v * w) & 0xFFFFFFFF
        rec[iz, :, :, 2] = w if g is not None else 0
        rec[iz, :, :, 3] = (g or 0) * w
    return opt, rec


def cube(n):
    return ref.Options(n, n, n, 0.25, (-0.5, -0.5, 1.0), 0.25, 0.5, 4.0, ref.CONSTANT)


@functools.lru_cache(maxsize=None)
def solids():
    opt = ref.Options(**GRID)
    x, y, z = grid_points(opt)
    sphere = np.sqrt((x - SPHERE_C[0]) ** 2 + (y - SPHERE_C[1]) ** 2 + (z - SPHERE_C[2]) ** 2) - SPHERE_R
    torus = np.sqrt((np.sqrt(x * x + y * y) - TORUS_R) ** 2 + z * z) - TORUS_r
    return {"sphere": (opt, from_distance(opt, sphere)), "torus": (opt, from_distance(opt, torus))}


@functools.lru_cache(maxsize=None)
def crafted():
    """name -> (options, records, min_weight)"""
    out = {}
    inside = np.zeros((6, 6, 6), bool)
    inside[1:3, 1:3, 1:3] = inside[1:3, 3:5, 3:5] = True  # two 2x2x2 solids that share the edge x = 2.5, y = 2.5
    out["touching"] = (cube(6), signs(cube(6), inside), 1)
    one = np.zeros((2, 2, 2), bool)
    one[0, 0, 0] = True
    out["one_corner"] = (cube(2), signs(cube(2), one), 1)
    centre = np.zeros((3, 3, 3), bool)
    centre[1, 1, 1] = True
    out["centre"] = (cube(3), signs(cube(3), centre), 1)
    iz, iy, ix = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    out["checkerboard"] = (cube(2), signs(cube(2), (ix + iy + iz) % 2 == 0), 1)
    weights = np.full((3, 3, 3), 2)
    weights[0, 0, 0] = 1
    out["unknown_corner"] = (cube(3), signs(cube(3), centre, weights=weights), 2)
    colour = np.ones((2, 2, 2), np.int64)
    colour[0, 0, 0] = 0
    out["uncoloured"] = (cube(2), signs(cube(2), one, colour=colour), 1)
    out["zero_at_b"] = slab_volume([2047, 1000, 0, -1000], n=3) + (1,)
    out["wall"] = slab_volume([2047, 1000, 500, -500, -1000, -2047]) + (1,)
    for v in out.values():
        v[1].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stream():
    """eight 64x48 sensor frames along the stream, as tests/test_volume.py makes them: (frames as (Z, I, K, pose), K, poses)"""
    from dvo_slam_amd import synth

    K = tuple(float(k) for k in synth.intrinsics_for(W, H))
    poses = [synth.se3_exp(4 * synth.XI_STEP_STREAM * t) for t in range(8)]
    frames = []
    for t, T in enumerate(poses):
        grey, raw_z = synth.sensor_frame(W, H, T, frame_id=t)
        I, Z = synth.raw_to_float(grey, raw_z)
        frames.append((Z, I, K, T))
    return frames, K, poses


@functools.lru_cache(maxsize=None)
def room():
    """the room of tests/test_volume.py: 8 frames into 64 x 52 x 56, by the restatement"""
    opt = ref.Options(weight=ref.SENSOR, **ROOM)
    rec = ref.empty(opt)
    ref.integrate(opt, rec, stream()[0])
    rec.setflags(write=False)
    return opt, rec


@functools.lru_cache(maxsize=None)
def reference(name, min_weight=None):
    """the vectorised restatement of a named input, computed once and shared"""
    if name == "room":
        opt, rec = room()
        mw = 1
    elif name in solids():
        (opt, rec), mw = solids()[name], 1
    else:
        opt, rec, mw = crafted()[name]
    out = mref.mesh(opt, rec, mw if min_weight is None else min_weight)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def both(opt, rec, min_weight=1, want=None):
    a = mref.mesh(opt, rec, min_weight) if want is None else want
    b = mref.mesh_scalar(opt, rec, min_weight)
    assert same_mesh(a, b), (a[4], b[4])
    return a


# ---- properties of a mesh ----------------------------------------------------------------------------------------------------------

def directed_edges(tri):
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64)
    return e[:, 0] * (1 << 32) + e[:, 1], e[:, 1] * (1 << 32) + e[:, 0]


def is_closed(tri):
    """every directed edge occurs once, and its reverse occurs once"""
    fwd, back = directed_edges(tri)
    return len(np.unique(fwd)) == len(fwd) and np.array_equal(np.sort(fwd), np.sort(back))


def euler(n_vertices, tri):
    fwd, back = directed_edges(tri)
    return n_vertices - len(np.unique(np.minimum(fwd, back))) + len(tri)


def signed_volume(xyz, tri):
    p = xyz.astype(np.float64)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def faces_agree_with_normals(xyz, normals, tri):
    p = xyz.astype(np.float64)
    g = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    return bool((np.einsum("ij,ij->i", g, normals[tri[:, 0]].astype(np.float64)) > 0).all())


# ---- CPU: exports and argument checks ----------------------------------------------------------------------------------------------

def test_exports_and_layout(capi):
    L = capi.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    assert all(re.search(r"\b%s\s*\(" % name, header) for name in NEW_SYMBOLS)
    assert L.dvo_amd_abi_version() == 3
    assert C.sizeof(capi.CVolumeMeshCounts) == 40 and tuple(n for n, _ in capi.CVolumeMeshCounts._fields_) == COUNT_NAMES
    from dvo_slam_amd import tum
    assert callable(tum.write_ply)


def test_argument_errors_fire_before_a_device_is_looked_for(capi, tmp_path):
    L = capi.lib()

    def refused(entry, rc, *words):
        err = L.dvo_amd_last_error().decode()
        assert rc == INVALID and err.startswith(entry + ": ") and all(w in err for w in words), (entry, rc, err)

    cnt = capi.CVolumeMeshCounts(1, 2, 3, 4, 5)
    pts, tri = (C.c_float * 4)(), (C.c_int * 3)()
    refused("dvo_amd_volume_mesh", L.dvo_amd_volume_mesh(None, 0, None, None, 0, None, 0, C.byref(cnt)), "min_weight")
    assert [getattr(cnt, n) for n in COUNT_NAMES] == [0] * 5
    refused("dvo_amd_volume_mesh", L.dvo_amd_volume_mesh(None, 1, pts, None, -1, None, 0, C.byref(cnt)), "vertex capacity")
    refused("dvo_amd_volume_mesh", L.dvo_amd_volume_mesh(None, 1, None, None, 1, None, 0, C.byref(cnt)), "vertex capacity")
    refused("dvo_amd_volume_mesh", L.dvo_amd_volume_mesh(None, 1, None, None, 0, tri, -1, C.byref(cnt)), "triangle capacity")
    refused("dvo_amd_volume_mesh", L.dvo_amd_volume_mesh(None, 1, None, None, 0, None, 1, C.byref(cnt)), "triangle capacity")
    refused("dvo_amd_volume_mesh", L.dvo_amd_volume_mesh(None, 1, None, None, 0, None, 0, C.byref(cnt)), "NULL")
    refused("dvo_amd_volume_mesh", L.dvo_amd_volume_mesh(None, 1, None, None, 0, None, 0, None), "NULL")
    rec = np.zeros(8, capi.VOLUME_VOXEL_DTYPE)
    refused("dvo_amd_volume_upload", L.dvo_amd_volume_upload(None, None, rec.ctypes.data, -1), "negative")
    refused("dvo_amd_volume_upload", L.dvo_amd_volume_upload(None, None, rec.ctypes.data, 8), "NULL")
    refused("dvo_amd_volume_upload", L.dvo_amd_volume_upload(None, None, None, 0), "NULL")
    path = os.fsencode(str(tmp_path / "x.ply"))
    one = (C.c_int * 3)(0, 1, 2)
    three = (C.c_float * 12)()
    refused("dvo_amd_write_ply", L.dvo_amd_write_ply(None, three, None, 3, one, 1), "NULL")
    refused("dvo_amd_write_ply", L.dvo_amd_write_ply(path, None, None, 3, one, 1), "NULL")
    refused("dvo_amd_write_ply", L.dvo_amd_write_ply(path, three, None, 3, None, 1), "NULL")
    refused("dvo_amd_write_ply", L.dvo_amd_write_ply(path, three, None, -1, None, 0), "negative")
    refused("dvo_amd_write_ply", L.dvo_amd_write_ply(path, three, None, 3, one, -1), "negative")
    refused("dvo_amd_write_ply", L.dvo_amd_write_ply(path, three, None, 2, one, 1), "triangle 0", "vertex 2")
    refused("dvo_amd_write_ply", L.dvo_amd_write_ply(path, three, None, 3, (C.c_int * 3)(0, -1, 2), 1), "vertex -1")
    assert not os.path.exists(path)  # a refused call writes nothing
    assert L.dvo_amd_write_ply(b"/nowhere/x.ply", three, None, 3, one, 1) == IO


# ---- CPU: the rule on two solids ---------------------------------------------------------------------------------------------------

def test_the_sphere_is_closed_oriented_and_on_the_sphere():
    opt, rec = solids()["sphere"]
    xyz, rgb, normals, tri, cnt = both(opt, rec, want=reference("sphere"))
    assert cnt["vertices"] == len(xyz) and cnt["triangles"] == len(tri) and cnt["open_edges"] == cnt["uncoloured"] == cnt["flat"] == 0
    assert is_closed(tri) and euler(len(xyz), tri) == 2 and len(np.unique(tri)) == len(xyz)
    volume = signed_volume(xyz, tri)
    radius = np.linalg.norm(xyz.astype(np.float64) - np.asarray(SPHERE_C), axis=1)
    print("sphere: %d vertices, %d triangles, radii %.4f .. %.4f, volume %.4f (a ball of %.2f: %.4f)"
          % (len(xyz), len(tri), radius.min(), radius.max(), volume, SPHERE_R, 4.0 / 3.0 * np.pi * SPHERE_R ** 3))
    assert volume > 0
    assert faces_agree_with_normals(xyz, normals, tri)
    assert np.abs(radius - SPHERE_R).max() <= float(opt.voxel) / 2
    assert np.all(np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1.0) < 1e-6)


def test_the_torus_is_closed_with_one_handle():
    opt, rec = solids()["torus"]
    xyz, rgb, normals, tri, cnt = both(opt, rec, want=reference("torus"))
    print("torus: %d vertices, %d triangles" % (len(xyz), len(tri)))
    assert cnt["open_edges"] == 0 and is_closed(tri) and euler(len(xyz), tri) == 0
    assert signed_volume(xyz, tri) > 0 and faces_agree_with_normals(xyz, normals, tri)


# ---- CPU: crafted cases, each asserting that it hits its case ------------------------------------------------------------------------

def test_crafted_cases_hit_their_case():
    def run(name):
        opt, rec, mw = crafted()[name]
        return both(opt, rec, mw, want=reference(name))

    # two solids that touch along an edge: one vertex serves both sheets, the mesh is not manifold there (the documented ambiguity)
    xyz, rgb, normals, tri, cnt = run("touching")
    fwd, _ = directed_edges(tri)
    assert cnt["open_edges"] == 0 and cnt["triangles"] == 2 * 2 * 24 and not is_closed(tri) and len(np.unique(fwd)) < len(fwd)
    # one inside corner in the only cell: a vertex, no face, three open edges
    xyz, rgb, normals, tri, cnt = run("one_corner")
    assert cnt == dict(vertices=1, triangles=0, open_edges=3, uncoloured=0, flat=0) and tri.shape == (0, 3)
    third = (F(0.0) + F(0.5) / F(3.0)) * F(0.25)  # three crossings at s = 1/2, one along each axis
    assert np.array_equal(bits(xyz[0]), bits(np.array([F(-0.5) + third, F(-0.5) + third, F(1.0) + third], F)))
    assert np.all(normals[0] > 0) and rgb[0] == 0x646464  # out of the solid: away from the inside corner
    # the smallest volume that holds a face: one inside voxel in the middle of 3x3x3 gives an octahedron-like closed mesh
    xyz, rgb, normals, tri, cnt = run("centre")
    assert cnt == dict(vertices=8, triangles=12, open_edges=0, uncoloured=0, flat=0)
    assert is_closed(tri) and euler(8, tri) == 2 and signed_volume(xyz, tri) > 0 and faces_agree_with_normals(xyz, normals, tri)
    # a 3-D checkerboard of signs: every edge crosses, the gradient cancels
    xyz, rgb, normals, tri, cnt = run("checkerboard")
    assert cnt == dict(vertices=1, triangles=0, open_edges=12, uncoloured=0, flat=1) and not normals.any()
    assert np.array_equal(bits(xyz[0]), bits(np.array([-0.375, -0.375, 1.125], F)))  # twelve crossings at s = 1/2: the cell's middle
    # a corner below min_weight: its cell is not known, has no vertex, and the three crossing edges around it are open
    opt, rec, mw = crafted()["unknown_corner"]
    known, active = mref.cells(opt, rec, mw)
    assert not known[0, 0, 0] and known.sum() == 7 and active.sum() == 7
    xyz, rgb, normals, tri, cnt = run("unknown_corner")
    assert cnt == dict(vertices=7, triangles=6, open_edges=3, uncoloured=0, flat=0) and not is_closed(tri)
    assert both(opt, rec, 1)[4] == dict(vertices=8, triangles=12, open_edges=0, uncoloured=0, flat=0)
    assert both(opt, rec, 3)[4] == dict(vertices=0, triangles=0, open_edges=0, uncoloured=0, flat=0)
    # no colour on one side of every crossing edge
    xyz, rgb, normals, tri, cnt = run("uncoloured")
    assert cnt == dict(vertices=1, triangles=0, open_edges=3, uncoloured=1, flat=0) and rgb[0] == 0
    # Fb == 0 exactly: s = 1, the vertices lie on slab 2's centres
    xyz, rgb, normals, tri, cnt = run("zero_at_b")
    assert cnt == dict(vertices=4, triangles=2, open_edges=8, uncoloured=0, flat=0)
    assert np.all(bits(xyz[:, 2]) == bits(F(1.5))) and np.all(rgb == 0x646464)
    # the wall of tests/test_volume.py: a flat sheet, every normal (0, 0, -1) -- F falls with z, the cameras look along +z
    xyz, rgb, normals, tri, cnt = run("wall")
    assert cnt == dict(vertices=25, triangles=2 * 16, open_edges=36 - 16, uncoloured=0, flat=0)
    assert np.array_equal(normals, np.tile(np.array([0, 0, -1], F), (25, 1))) and len(np.unique(bits(xyz[:, 2]))) == 1
    assert F(1.5) < xyz[0, 2] < F(1.75) and faces_agree_with_normals(xyz, normals, tri)


def test_triangles_and_open_edges_add_up_to_the_points_of_extract():
    inputs = {name: solids()[name] + (1,) for name in solids()}
    inputs.update(crafted())
    inputs["room"] = room() + (1,)
    for name, (opt, rec, mw) in inputs.items():
        cnt = reference(name)[4]
        assert cnt["triangles"] % 2 == 0 and cnt["triangles"] // 2 + cnt["open_edges"] == ref.extract(opt, rec, mw)[2]["points"], (name, cnt)
    opt, rec = room()
    for mw in (2, 400):
        cnt = mref.mesh(opt, rec, mw)[4]
        assert cnt["triangles"] // 2 + cnt["open_edges"] == ref.extract(opt, rec, mw)[2]["points"], (mw, cnt)
    cnt = reference("room")[4]
    assert cnt["vertices"] > 1000 and cnt["triangles"] > 2000 and cnt["open_edges"] > 0


# ---- CPU: the PLY file -------------------------------------------------------------------------------------------------------------

def read_ply(path):
    """(xyz, normals or None, rgb bytes [n, 3], triangles) of a binary little-endian PLY with exactly the properties the writer emits"""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode().splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    elements, props = [], {}
    for ln in lines[2:-1]:
        t = ln.split()
        if t[0] == "element":
            elements.append((t[1], int(t[2])))
            props[t[1]] = []
        elif t[0] == "property":
            props[elements[-1][0]].append(tuple(t[1:]))
    assert [e[0] for e in elements] == ["vertex", "face"] and props["face"] == [("list", "uchar", "int", "vertex_indices")]
    kinds = {"float": "<f4", "uchar": "u1"}
    vt = np.dtype([(p[1], kinds[p[0]]) for p in props["vertex"]])
    names = [p[1] for p in props["vertex"]]
    assert names in (["x", "y", "z", "red", "green", "blue"], ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"])
    nv, nf = elements[0][1], elements[1][1]
    v = np.frombuffer(blob, vt, nv, end)
    ft = np.dtype([("n", "u1"), ("v", "<i4", 3)])
    f = np.frombuffer(blob, ft, nf, end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nf * ft.itemsize == len(blob) and np.all(f["n"] == 3)
    xyz = np.stack([v["x"], v["y"], v["z"]], axis=-1).reshape(-1, 3)
    nrm = np.stack([v["nx"], v["ny"], v["nz"]], axis=-1).reshape(-1, 3) if "nx" in names else None
    return xyz, nrm, np.stack([v["red"], v["green"], v["blue"]], axis=-1).reshape(-1, 3), f["v"].reshape(-1, 3)


def test_write_ply_round_trip(tmp_path):
    from dvo_slam_amd import tum

    xyz, rgb, normals, tri, _ = reference("sphere")
    rgb = rgb.copy()
    rgb[:3] = [0x010203, 0xFF8000, 0x0000FE]  # red, green and blue apart
    for with_normals in (True, False):
        path = str(tmp_path / ("n.ply" if with_normals else "p.ply"))
        tum.write_ply(path, xyz, rgb, tri, normals=normals if with_normals else None)
        got = read_ply(path)
        assert same_bits(got[0].astype(F), xyz) and np.array_equal(got[3], tri)
        assert (got[1] is None) != with_normals and (not with_normals or same_bits(got[1].astype(F), normals))
        assert np.array_equal(got[2][:, 0].astype(np.uint32) << 16 | got[2][:, 1].astype(np.uint32) << 8 | got[2][:, 2], rgb)
        assert got[2][:3].tolist() == [[1, 2, 3], [255, 128, 0], [0, 0, 254]]
    empty = str(tmp_path / "empty.ply")
    tum.write_ply(empty, np.zeros((0, 3), F), np.zeros(0, np.uint32), np.zeros((0, 3), np.int32))
    got = read_ply(empty)
    assert len(got[0]) == 0 and len(got[3]) == 0
    with pytest.raises(ValueError):
        tum.write_ply(empty, xyz, rgb, tri, normals=normals[:2])


# ---- GPU: the library against the restatement ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


def records(vol, box=None):
    d = vol.download(box)
    return np.stack([d[n] for n in ("w_sum", "sd_sum", "iw_sum", "i_sum")], axis=-1)


def uploaded(gpu, opt, rec):
    vol = gpu.SurfaceVolume(opt.fields())
    vol.upload(ref.public(rec))
    return vol


@pytest.mark.gpu
def test_upload_is_the_inverse_of_download(gpu):
    opt, rec = solids()["sphere"]
    vol = gpu.SurfaceVolume(opt.fields())
    rng = np.random.RandomState(3)
    noise = rng.randint(-2 ** 31, 2 ** 31, size=rec.shape, dtype=np.int64).astype(np.int32)
    vol.upload(noise)
    assert np.array_equal(records(vol), noise)
    vol.upload(vol.download())  # a structured array, as download() returns it
    assert np.array_equal(records(vol), noise)
    box = (3, 0, 7, 9, 13, 8)
    part = ref.public(rec)[7:9, 0:14, 3:10]
    vol.upload(part, box)
    want = noise.copy()
    want[7:9, 0:14, 3:10] = part
    assert np.array_equal(records(vol), want) and np.array_equal(records(vol, box), part)
    vol.upload(ref.public(rec)[13:, 13:, 13:], (13, 13, 13, 13, 13, 13))
    want[13, 13, 13] = ref.public(rec)[13, 13, 13]
    assert np.array_equal(records(vol), want)
    # what is refused leaves the volume as it was
    for call in (lambda: vol.upload(part, (3, 0, 7, 9, 13, 9)), lambda: vol.upload(part), lambda: vol.upload(part, (3, 0, 7, 9, 14, 8)),
                 lambda: vol.upload(noise[:0])):
        with pytest.raises(gpu.DvoAmdError) as e:
            call()
        assert e.value.status == INVALID and "dvo_amd_volume_upload" in str(e.value)
    with pytest.raises(ValueError):
        vol.upload(np.zeros((14, 14, 14, 3), np.int32))
    assert np.array_equal(records(vol), want)


class Resident:
    """the stream's pyramids on the device"""

    def __init__(self, capi):
        frames, K, poses = stream()
        self.K, self.poses = K, poses
        self.pyramids = [capi.RgbdImagePyramid(I, Z, K, 2) for Z, I, _, _ in frames]


@pytest.fixture(scope="module")
def resident(gpu):
    return Resident(gpu)


@pytest.mark.gpu
def test_upload_and_the_two_forms_of_integration(gpu, resident):
    opt, rec = room()
    vol = gpu.SurfaceVolume(opt.fields())
    vol.insert([4], resident.pyramids[:1], resident.poses[:1])
    before = records(vol)
    with pytest.raises(gpu.DvoAmdError) as e:  # the tracked form holds a keyframe: its contract would break
        vol.upload(ref.public(rec))
    assert e.value.status == INVALID and "keyframes" in str(e.value) and np.array_equal(records(vol), before)
    vol.remove([4])
    assert not records(vol).any()
    vol.integrate(resident.pyramids[:2], resident.poses[:2])  # the anonymous form keeps nothing: upload replaces the records
    assert records(vol).any()
    vol.upload(ref.public(rec))
    assert np.array_equal(records(vol), ref.public(rec))
    vol.integrate(resident.pyramids, resident.poses, sign=-1)  # ... which are the eight frames' sums: -1 leaves nothing
    assert not records(vol).any()
    assert vol.mesh()[4] == dict(vertices=0, triangles=0, open_edges=0, uncoloured=0, flat=0)
    t = gpu.volume_timing(True)
    assert (t["launches"], t["synchronisations"]) == (3, 2)  # no vertex: nothing is written


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere", "torus"] + list(crafted()))
def test_the_device_mesh_equals_the_restatement(gpu, name):
    if name in solids():
        (opt, rec), mw = solids()[name], 1
    else:
        opt, rec, mw = crafted()[name]
    vol = uploaded(gpu, opt, rec)
    gpu.volume_timing(True)
    got = vol.mesh(mw)
    want = reference(name)
    assert same_mesh(got, want), (got[4], want[4])
    if name == "sphere":  # 13^3 = 2197 cells: more than one tile of 2048, rows of 13 cells that never align with a 64-bit word
        assert (opt.nx - 1) * (opt.ny - 1) * (opt.nz - 1) == 2197
        plain = vol.mesh(mw, normals=False)
        assert plain[2] is None and same_bits(plain[0], want[0]) and np.array_equal(plain[3], want[3]) and plain[4] == want[4]
    ex = vol.extract(mw)[2]["points"]
    assert got[4]["triangles"] // 2 + got[4]["open_edges"] == ex


@pytest.mark.gpu
def test_the_room_from_the_resident_stream(gpu, resident):
    opt, rec = room()
    vol = gpu.SurfaceVolume(opt.fields())
    vol.integrate(resident.pyramids, resident.poses)
    assert np.array_equal(records(vol), ref.public(rec))
    gpu.volume_timing(True)
    want = reference("room")
    got = vol.mesh()
    t = gpu.volume_timing(True)
    assert same_mesh(got, want), (got[4], want[4])
    assert (t["launches"], t["synchronisations"]) == (5, 2)  # cells, edges, scan | vertices, faces: whatever the volume holds
    again = vol.mesh()
    assert same_mesh(again, got)  # two runs are identical
    for mw in (2, 400):
        assert same_mesh(vol.mesh(mw), mref.mesh(opt, rec, mw)), mw
    # the capacity protocol: one short array is refused with both sizes reported and nothing written
    V, T = want[4]["vertices"], want[4]["triangles"]
    L = gpu.lib()
    for cap_v, cap_t in ((V - 1, T), (V, T - 1), (0, 0)):
        pts, nrm, tri = np.full((V, 4), 7, F), np.full((V, 3), 7, F), np.full((T, 3), 7, np.int32)
        cnt = gpu.CVolumeMeshCounts()
        rc = L.dvo_amd_volume_mesh(vol._h, 1, pts.ctypes.data, nrm.ctypes.data_as(C.POINTER(C.c_float)), cap_v,
                                   tri.ctypes.data_as(C.POINTER(C.c_int)), cap_t, C.byref(cnt))
        assert rc == CAPACITY and (cnt.vertices, cnt.triangles, cnt.open_edges) == (V, T, want[4]["open_edges"])
        assert np.all(pts == 7) and np.all(nrm == 7) and np.all(tri == 7)
        t = gpu.volume_timing(True)
        assert (t["launches"], t["synchronisations"]) == (3, 1)
    with pytest.raises(gpu.DvoAmdError) as e:
        vol.mesh(capacity=(V, T - 2))
    assert e.value.status == CAPACITY and vol.last_mesh_size == (V, T)
    assert same_mesh(vol.mesh(capacity=(V, T)), want) and same_mesh(vol.mesh(capacity=(V + 5, T + 1)), want)
    with pytest.raises(gpu.DvoAmdError) as e:
        vol.mesh(0)
    assert e.value.status == INVALID
    # after the frames are taken out again the mesh is empty
    vol.integrate(resident.pyramids, resident.poses, sign=-1)
    assert vol.mesh()[4] == dict(vertices=0, triangles=0, open_edges=0, uncoloured=0, flat=0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_the_shapes_of_the_volume_tests(gpu, resident, shape):
    opt = ref.Options(weight=ref.SENSOR, **SHAPES[shape])
    vol = gpu.SurfaceVolume(opt.fields())
    vol.integrate([resident.pyramids[0], resident.pyramids[4]], [resident.poses[0], resident.poses[4]])
    rec = records(vol).view(np.uint32)
    want = mref.mesh(opt, rec)
    got = vol.mesh()
    assert same_mesh(got, want), (got[4], want[4])
    assert want[4]["vertices"] > 0  # the wall z = 3 runs through every one of them
    assert got[4]["triangles"] // 2 + got[4]["open_edges"] == vol.extract()[2]["points"]


@pytest.mark.gpu
def test_a_wall_across_more_tiles_than_one_chunk_of_the_scan(gpu):
    # the scan of the tile totals takes 256 tiles of 2048 cells (or voxels) at a time: 129 * 129 * 33 cells are more than 524 288.
    # F depends on x alone, so the sheet x = const has vertices in every z: in every tile, on both sides of the chunk's end
    opt = ref.Options(130, 130, 34, 0.02, (-1.0, -1.0, 1.0), 0.06, 0.4, 5.0, ref.CONSTANT)
    assert (opt.nx - 1) * (opt.ny - 1) * (opt.nz - 1) > 256 * 2048
    rec = ref.empty(opt)
    ix = np.arange(opt.nx)
    rec[..., 0] = 3
    rec[..., 1] = (np.clip((70.3 - ix) * 400, -2047, 2047).astype(np.int64) * 3) & 0xFFFFFFFF
    rec[..., 2] = 2
    rec[..., 3] = 2 * (500 + 20 * ix)
    vol = uploaded(gpu, opt, rec)
    want = mref.mesh(opt, rec, 2)
    got = vol.mesh(2)
    assert same_mesh(got, want), (got[4], want[4])
    assert want[4] == dict(vertices=129 * 33, triangles=2 * 128 * 32, open_edges=130 * 34 - 128 * 32, uncoloured=0, flat=0)
    assert want[3].max() == 129 * 33 - 1 and 256 * 2048 // (129 * 129) < 32  # cells of the last z-layers lie behind the chunk's end
    assert np.array_equal(got[2], np.tile(np.array([-1, 0, 0], F), (len(got[2]), 1)))
