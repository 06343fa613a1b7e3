"""Time of the keyframe map kept on the device (dvo_amd_map_*) against the rebuild (dvo_amd_map_cloud) it replaces.

640x480 keyframes along a slow sweep, N = 10, 50, 200, leaf 0.01.  For every N, interleaved in one process after a warm-up
cycle, medians of 7 with [min, max]:
  rebuild      one dvo_amd_map_cloud over the N keyframes (the only way to the same answer without the map)
  insert       the N-th keyframe into a map of N - 1
  move_one     dvo_amd_map_set_poses of one keyframe
  move_all     dvo_amd_map_set_poses of all N (the rebuild rule of DESIGN.md 4.6 applies)
  extract      the whole map
  extract_box  a box of about a tenth of the map's bounding volume
Device time (hipEvents inside the call: dvo_amd_debug_keyframe_map_timing, dvo_amd_debug_map_timing; for the extracts the
kernels, with the copy to the host apart) and whole-call time are reported separately.  Every cycle ends with the map checked
against the rebuild, bit for bit.  Writes profiles/keyframe_map.json.
Usage: python scripts/keyframe_map_timing.py [--sizes 10 50 200] [--reps 7] [--out profiles/keyframe_map.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dvo_slam_amd import capi, synth  # noqa: E402

W, H = 640, 480


def pose(k, alt=0.0):
    return synth.se3_exp(np.array([0.02, -0.01, 0.015, 0.01, -0.02, 0.005]) * 0.5 * k + alt * np.array([1, 2, -1, 0.5, -0.5, 1]) * 1e-3)


def summary(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10, 50, 200])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--leaf", type=float, default=0.01)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_map.json"))
    a = ap.parse_args()
    K = synth.intrinsics_for(W, H)
    pyrs, bgrs = [], []
    for k in range(max(a.sizes)):
        I, Z = synth.render(W, H, pose(k), frame_id=k)
        bgr, raw = synth.to_raw(I, Z)
        pyrs.append(capi.RgbdImagePyramid.from_raw(bgr, raw, K, 1))
        bgrs.append(bgr if k % 2 == 0 else None)
    trk = capi.DenseTracker()
    report = {"image": [W, H], "leaf": a.leaf, "reps": a.reps, "format": "[median, min, max] ms", "sizes": {}}
    for N in a.sizes:
        ids = list(range(N))
        m = capi.KeyframeMap(trk, a.leaf)
        for k in range(N - 1):
            m.insert(k, pyrs[k], pose(k), bgrs[k])
        t = {op: {"device_ms": [], "call_ms": []} for op in ("rebuild", "insert", "move_one", "move_all", "extract", "extract_box")}
        copy_ms, info = [], {}
        cap = None

        def timed(op, fn, device):
            t0 = time.perf_counter()
            out = fn()
            ms = (time.perf_counter() - t0) * 1e3
            if rep > 0:
                t[op]["call_ms"].append(ms)
                t[op]["device_ms"].append(device())
            return out

        for rep in range(a.reps + 1):  # cycle 0 warms every buffer up
            alt = 1.0 + (rep % 2)
            now = [pose(k) for k in ids]
            xyz, rgb, st = timed("rebuild", lambda: trk.map_cloud(pyrs[:N], now, bgrs[:N], leaf=a.leaf, capacity=cap),
                                 lambda: trk.map_timing()[0])
            cap = st["voxels"] + 1
            timed("insert", lambda: m.insert(N - 1, pyrs[N - 1], pose(N - 1), bgrs[N - 1]), lambda: m.timing()[0])
            info["insert_delta_voxels"] = m.timing()[3]
            got = m.extract()
            assert got[0].tobytes() == xyz.tobytes() and got[1].tobytes() == rgb.tobytes(), "map != rebuild"
            timed("move_one", lambda: m.set_poses([N // 2], [pose(N // 2, alt)]), lambda: m.timing()[0])
            info["move_one_delta_voxels"] = m.timing()[3]
            timed("move_all", lambda: m.set_poses(ids, [pose(k, alt) for k in ids]), lambda: m.timing()[0])
            full = timed("extract", lambda: m.extract(), lambda: m.timing()[0])
            if rep > 0:
                copy_ms.append(m.timing()[1])
            lo, hi = full[0].min(axis=0), full[0].max(axis=0)
            mid, half = (lo + hi) / 2, (hi - lo) / 2 * 0.1 ** (1.0 / 3.0)
            part = timed("extract_box", lambda: m.extract(np.r_[mid - half, mid + half]), lambda: m.timing()[0])
            info["box_voxels"] = len(part[0])
            moved = trk.map_cloud(pyrs[:N], [pose(k, alt) for k in ids], bgrs[:N], leaf=a.leaf, capacity=cap)
            assert full[0].tobytes() == moved[0].tobytes() and full[1].tobytes() == moved[1].tobytes(), "moved map != rebuild"
            m.set_poses(ids, now)
            m.remove([N - 1])
        entry = {"points": N * W * H, "voxels": st["voxels"], "extract_copy_ms": summary(copy_ms), **info}
        for op, v in t.items():
            entry[op] = {k: summary(x) for k, x in v.items()}
        report["sizes"][str(N)] = entry
        r = entry["rebuild"]
        print(f"N = {N}: {st['voxels']} voxels; rebuild device {r['device_ms']} call {r['call_ms']} ms")
        for op in ("insert", "move_one", "move_all", "extract", "extract_box"):
            e = entry[op]
            print(f"  {op:12s} device {e['device_ms']} call {e['call_ms']} ms   (rebuild / {op}, call medians: "
                  f"{r['call_ms'][0] / e['call_ms'][0]:.1f}x)")
        del m
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
