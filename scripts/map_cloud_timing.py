"""Time of the keyframe map's voxel aggregate (dvo_amd_map_cloud): 50 keyframes of 640x480 at distinct poses, 1 cm leaf.

Prints one line: device time of the call's kernels (hipEvents inside the call, dvo_amd_debug_map_timing), end to end,
Mpoints/s of both, the copy of the voxels to the host (reported apart), and the numpy restatement of tests/test_map_cloud.py
on the same input.  Usage: python scripts/map_cloud_timing.py [--keyframes 50] [--reps 10]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dvo_slam_amd import capi, synth  # noqa: E402
from test_map_cloud import cloud_ref, voxel_ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--leaf", type=float, default=0.01)
    a = ap.parse_args()
    w, h = 640, 480
    K = synth.intrinsics_for(w, h)
    poses = [synth.se3_exp(np.array([0.02, -0.01, 0.015, 0.01, -0.02, 0.005]) * 0.5 * k) for k in range(a.keyframes)]
    pyrs, bgrs = [], []
    for k, T in enumerate(poses):
        I, Z = synth.render(w, h, T, frame_id=k)
        bgr, raw = synth.to_raw(I, Z)
        pyrs.append(capi.RgbdImagePyramid.from_raw(bgr, raw, K, 1))
        bgrs.append(bgr)
    trk = capi.DenseTracker()
    xyz, rgb, st = trk.map_cloud(pyrs, poses, bgrs, leaf=a.leaf)  # warm: the workspace is grown here
    dev, e2e, copy = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        trk.map_cloud(pyrs, poses, bgrs, leaf=a.leaf, capacity=st["voxels"])
        e2e.append((time.perf_counter() - t0) * 1e3)
        d, c, _ = trk.map_timing()
        dev.append(d)
        copy.append(c)
    t0 = time.perf_counter()
    clouds = [cloud_ref(p.plane(0, 1), p.plane(0, 0), K, T, b) for p, T, b in zip(pyrs, poses, bgrs)]
    rx, rr, rst = voxel_ref(np.concatenate([c[0].reshape(-1, 3) for c in clouds]),
                            np.concatenate([c[1].reshape(-1) for c in clouds]), a.leaf)
    t_np = (time.perf_counter() - t0) * 1e3
    assert rst == st and rx.tobytes() == xyz.tobytes() and rr.tobytes() == rgb.tobytes(), "GPU result != restatement"
    n = st["points_in"]
    dm, em = float(np.median(dev)), float(np.median(e2e))
    print(f"map_cloud {a.keyframes} x {w}x{h} ({n / 1e6:.1f} M points -> {st['voxels']} voxels, leaf {a.leaf} m): "
          f"device {dm:.3f} ms ({n / dm / 1e3:.0f} Mpoints/s), end to end {em:.2f} ms ({n / em / 1e3:.0f} Mpoints/s), "
          f"voxel copy to host {float(np.median(copy)):.3f} ms; numpy restatement {t_np:.0f} ms "
          f"(medians of {a.reps}; result = restatement bit for bit)")


if __name__ == "__main__":
    main()
