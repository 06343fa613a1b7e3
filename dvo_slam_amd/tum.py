"""TUM RGB-D benchmark on-disk formats over the C ABI.

Mirrors what dvo_benchmark reads and writes around the tracker: the association file (`rgb_ts rgb_file depth_ts depth_file`
per line, rgbd_pair.h:59-71 read through file_reader.h:36-113), the frame loader `load()` of benchmark_slam.cpp:46-93
(cv::imread + gray conversion + depth scaling, here: PNG decode on the host, conversion on the GPU), and the estimated
trajectory (`timestamp tx ty tz qx qy qz qw`, benchmark_slam.cpp:490-504).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import capi

TUM_DEPTH_SCALE = 1.0 / 5000.0  # benchmark_slam.cpp:77
TUM_FR1_INTRINSICS = (517.3, 516.5, 318.6, 255.3)  # benchmark_slam.cpp:384

_bound = False


def _lib():
    global _bound
    L = capi.lib()
    if not _bound:
        ip = C.POINTER(C.c_int)
        L.dvo_amd_png_info.argtypes = [C.c_char_p, ip, ip, ip, ip]
        L.dvo_amd_png_read_bgr8.argtypes = [C.c_char_p, C.POINTER(C.c_ubyte), C.c_int, C.c_int]
        L.dvo_amd_png_read_gray16.argtypes = [C.c_char_p, C.POINTER(C.c_ushort), C.c_int, C.c_int]
        L.dvo_amd_format_trajectory_line.argtypes = [C.c_double, C.POINTER(C.c_double), C.c_char_p, C.c_int]
        _bound = True
    return L


def png_info(path: str):
    w, h, c, b = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    capi._check(_lib().dvo_amd_png_info(os.fsencode(path), C.byref(w), C.byref(h), C.byref(c), C.byref(b)), f"png_info({path})")
    return w.value, h.value, c.value, b.value


def imread_color(path: str) -> np.ndarray:
    """cv::imread(path, 1): HxWx3 uint8, B G R."""
    w, h, _, _ = png_info(path)
    out = np.empty((h, w, 3), np.uint8)
    capi._check(_lib().dvo_amd_png_read_bgr8(os.fsencode(path), out.ctypes.data_as(C.POINTER(C.c_ubyte)), w, h),
                f"png_read_bgr8({path})")
    return out


def imread_depth(path: str) -> np.ndarray:
    """cv::imread(path, -1) of a TUM depth image: HxW uint16."""
    w, h, _, _ = png_info(path)
    out = np.empty((h, w), np.uint16)
    capi._check(_lib().dvo_amd_png_read_gray16(os.fsencode(path), out.ctypes.data_as(C.POINTER(C.c_ushort)), w, h),
                f"png_read_gray16({path})")
    return out


class RgbdPair:
    """dvo_benchmark::RgbdPair (rgbd_pair.h:32-47)."""

    def __init__(self, rgb_timestamp: float, rgb_file: str, depth_timestamp: float, depth_file: str):
        self.RgbTimestamp, self.RgbFile, self.DepthTimestamp, self.DepthFile = rgb_timestamp, rgb_file, depth_timestamp, depth_file

    def __repr__(self):
        return f"RgbdPair({self.RgbTimestamp!r}, {self.RgbFile!r}, {self.DepthTimestamp!r}, {self.DepthFile!r})"


def read_assoc(path: str, reference_trailing_entry: bool = False):
    """FileReader<RgbdPair>::skipComments() + readAllEntries() (file_reader.h:63-102, benchmark_slam.cpp:168-169,399).
    Leading '#' lines are skipped; entries are whitespace-separated tokens, four per entry (line breaks do not matter to
    operator>>).  reference_trailing_entry=True reproduces the reference's end-of-file behaviour for a file that ends in a
    newline: one more next() succeeds on a stream that then fails, which appends a copy of the last entry whose
    timestamps are 0 (value-initialised by a failed C++11 extraction)."""
    with open(path, "r") as f:
        text = f.read()
    pos = 0
    while pos < len(text) and text[pos] == "#":  # skipComments: only while the NEXT character is '#'
        nl = text.find("\n", pos)
        pos = len(text) if nl < 0 else nl + 1
    body = text[pos:]
    tokens = body.split()
    entries = []
    for i in range(0, len(tokens) - len(tokens) % 4, 4):
        entries.append(RgbdPair(float(tokens[i]), tokens[i + 1], float(tokens[i + 2]), tokens[i + 3]))
    if reference_trailing_entry and entries and body[-1:].isspace():
        last = entries[-1]
        entries.append(RgbdPair(0.0, last.RgbFile, 0.0, last.DepthFile))
    return entries


def read_groundtruth(path: str):
    """groundtruth.txt / a trajectory file: [(timestamp, 4x4 pose)] from `timestamp tx ty tz qx qy qz qw` lines."""
    out = []
    with open(path, "r") as f:
        for line in f:
            t = line.split()
            if len(t) < 8 or line.lstrip().startswith("#"):
                continue
            ts, tx, ty, tz, qx, qy, qz, qw = [float(v) for v in t[:8]]
            n = np.sqrt(qx * qx + qy * qy + qz * qz + qw * qw)
            qx, qy, qz, qw = qx / n, qy / n, qz / n, qw / n
            T = np.eye(4)
            T[:3, :3] = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                         [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                         [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]]
            T[:3, 3] = [tx, ty, tz]
            out.append((ts, T))
    return out


def load(K, rgb_file: str, depth_file: str, levels: int, device: int = 0, timestamp: float = 0.0,
         depth_scale: float = TUM_DEPTH_SCALE, remap: "capi.Remap | None" = None, depth_filter=None) -> capi.RgbdImagePyramid:
    """`load()` of benchmark_slam.cpp:46-93: imread both files, BGR -> gray float, raw depth -> metres with 0 -> NaN,
    camera.create(...).  Decoding happens on the host, both conversions and the pyramid on the GPU.
    remap: a capi.Remap through which both images are resampled on the way in (K is then the rectified camera's).  There is no
    preset: TUM's depth PNGs were registered by the driver with default intrinsics, so whether to resample them with the
    colour camera's distortion is the caller's decision.
    depth_filter: None, or what RgbdImagePyramid.filter_depth takes as options (a capi.DepthFilterOptions or a dict of its fields;
    {} for the defaults): the pyramid's level-0 depth is filtered on the device after ingest and the filtered pyramid returned."""
    bgr = imread_color(rgb_file)
    depth = imread_depth(depth_file)
    pyramid = capi.RgbdImagePyramid.from_raw(bgr, depth, K, levels, depth_scale=depth_scale, device=device, timestamp=timestamp,
                                             remap=remap)
    return pyramid if depth_filter is None else pyramid.filter_depth(depth_filter)


def load_batch(entries, K, levels: int, device: int = 0, base: str = "", depth_scale: float = TUM_DEPTH_SCALE, selection=None,
               depth_filter=None):
    """load() for several entries of an association file (RgbdPair: RgbFile, DepthFile, RgbTimestamp; file names relative to
    `base`) in ONE pyramid build (capi.RgbdImagePyramid.from_raw_batch): the PNGs are decoded on the host one after the other,
    then every frame's conversions and pyramid share the same few kernel launches.  Returns the pyramids in the entries' order,
    each with its entry's RgbTimestamp, each what load() makes of that entry.  selection: None, or (intensity_threshold,
    depth_threshold) -- a tracker's two derivative thresholds -- to have every pyramid's point selection built in the same call.
    Resampling through a remap stays with load().  depth_filter: see load(); all pyramids are filtered in one further call
    (capi.filter_depth_many).  A filtered pyramid has no selection yet: `selection` is then built with the first use, not here."""
    bgr = [imread_color(os.path.join(base, p.RgbFile)) for p in entries]
    depth = [imread_depth(os.path.join(base, p.DepthFile)) for p in entries]
    pyramids = capi.RgbdImagePyramid.from_raw_batch(bgr, depth, K, levels, depth_scale=depth_scale, device=device,
                                                    timestamps=[p.RgbTimestamp for p in entries],
                                                    selection=selection if depth_filter is None else None)
    return pyramids if depth_filter is None else capi.filter_depth_many(pyramids, depth_filter)


def format_trajectory_line(timestamp: float, T) -> str:
    """One line of the estimated trajectory as benchmark_slam.cpp:490-504 prints it (including the trailing blank)."""
    Tc = np.ascontiguousarray(np.asarray(T, dtype=np.float64).T)
    buf = C.create_string_buffer(256)
    n = _lib().dvo_amd_format_trajectory_line(float(timestamp), Tc.ctypes.data_as(C.POINTER(C.c_double)), buf, 256)
    if n < 0:
        raise RuntimeError("dvo_amd_format_trajectory_line failed")
    return buf.raw[:n].decode()


def replay(assoc_path: str, trajectory_path: str | None = None, K=TUM_FR1_INTRINSICS, config: capi.Config | None = None,
           device: int = 0, max_frames: int | None = None, remap: "capi.Remap | None" = None):
    """Frame-to-frame odometry over an association file (the EstimateTrajectory mode of dvo_benchmark without the SLAM back
    end): pose_t = pose_{t-1} * T_t^-1 with T_t = match(frame_{t-1}, frame_t), one trajectory line per frame.
    Returns [(timestamp, 4x4 pose)].  remap: see load()."""
    cfg = config or capi.Config(FirstLevel=3, LastLevel=1)
    trk = capi.DenseTracker(cfg, device=device)
    base = os.path.dirname(os.path.abspath(assoc_path))
    pairs = read_assoc(assoc_path)
    if max_frames is not None:
        pairs = pairs[:max_frames]
    pose = np.eye(4)
    prev = None
    out = []
    fh = open(trajectory_path, "w") if trajectory_path else None
    try:
        for p in pairs:
            cur = load(K, os.path.join(base, p.RgbFile), os.path.join(base, p.DepthFile), cfg.getNumLevels(), device,
                       p.RgbTimestamp, remap=remap)
            if prev is not None:
                r = trk.match(prev, cur)
                if not r.isNaN():
                    pose = pose @ np.linalg.inv(r.Transformation)
            out.append((p.RgbTimestamp, pose.copy()))
            if fh:
                fh.write(format_trajectory_line(p.RgbTimestamp, pose))
            prev = cur
    finally:
        if fh:
            fh.close()
    return out


def write_pcd(path: str, xyz, rgb, normals=None):
    """Binary PCD v0.7 of a coloured cloud as pcl::io::savePCDFileBinary writes PointXYZRGB (dvo_amd_write_pcd).  xyz [h, w, 3]
    with rgb [h, w] is written organized (WIDTH w, HEIGHT h); xyz [n, 3] with rgb [n] as n x 1.  With normals ([h, w, 4] or
    [n, 4], as point_cloud(normals=...) returns them) the file is a PointXYZRGBNormal cloud (dvo_amd_write_pcd_normals)."""
    xyz = np.asarray(xyz, dtype=np.float32)
    rgb = np.asarray(rgb, dtype=np.uint32)
    if xyz.ndim == 3:
        height, width = xyz.shape[:2]
    else:
        height, width = 1, len(xyz)
    pts = capi._pack_points(xyz, rgb)
    if normals is not None:
        nrm = np.ascontiguousarray(np.asarray(normals, dtype=np.float32).reshape(-1, 4))
        if len(nrm) != len(pts):
            raise ValueError("xyz and normals must hold the same number of points")
        capi._check(_lib().dvo_amd_write_pcd_normals(os.fsencode(path), pts.ctypes.data, capi._fp(nrm), len(pts), width, height),
                    "dvo_amd_write_pcd_normals")
        return
    capi._check(_lib().dvo_amd_write_pcd(os.fsencode(path), pts.ctypes.data, len(pts), width, height), "dvo_amd_write_pcd")


def write_ply(path: str, xyz, rgb, triangles, normals=None):
    """Binary little-endian PLY of an indexed triangle mesh (dvo_amd_write_ply): vertices xyz [V, 3] with packed rgb [V] and,
    when given, normals [V, 3]; triangles int32 [T, 3] -- what SurfaceVolume.mesh() returns."""
    pts = capi._pack_points(xyz, rgb)
    tri = np.ascontiguousarray(np.asarray(triangles, dtype=np.int32).reshape(-1, 3))
    nrm = None
    if normals is not None:
        nrm = np.ascontiguousarray(np.asarray(normals, dtype=np.float32).reshape(-1, 3))
        if len(nrm) != len(pts):
            raise ValueError("xyz and normals must hold the same number of vertices")
    capi._check(_lib().dvo_amd_write_ply(os.fsencode(path), pts.ctypes.data, None if nrm is None else capi._fp(nrm), len(pts),
                                         tri.ctypes.data_as(C.POINTER(C.c_int)), len(tri)), "dvo_amd_write_ply")
