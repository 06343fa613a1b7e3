"""Time of the map render (dvo_amd_map_render, dvo_amd_map_render_pyramid) next to dvo_amd_map_extract, the only other way to
use the device map, and what tracking against the rendered model gives on one synthetic sequence.

The maps are those of scripts/keyframe_map_timing.py: 640x480 keyframes along a slow sweep, N = 10, 50, 200, leaf 0.01.  For
every N, interleaved in one process after a warm-up cycle, medians of 7 with [min, max]:
  render          all four planes of a 640x480 view at the pose halfway along the sweep, copied to the host
  render_pyramid  the same view as a 4-level pyramid, nothing copied to the host
  extract         the whole map (the row of profiles/keyframe_map.json, taken again in this run)
Device time (hipEvents around the kernels inside the call, dvo_amd_debug_keyframe_map_timing; the copies to the host and the
pyramid build are not in it) and whole-call time are reported separately.
Tracking: keyframes 0 .. k-1 of the sweep are in the map; frame k is aligned to the model view rendered at the pose of frame
k-1 and, for comparison, to keyframe k-1 itself; the error is that of the estimated relative pose against the ground truth.
Writes profiles/map_render.json.
Usage: python scripts/map_render_timing.py [--sizes 10 50 200] [--reps 7] [--out profiles/map_render.json]"""
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


def pose(k):
    return synth.se3_exp(np.array([0.02, -0.01, 0.015, 0.01, -0.02, 0.005]) * 0.5 * k)


def summary(v):
    return [round(float(np.median(v)), 4), round(float(np.min(v)), 4), round(float(np.max(v)), 4)]


def pose_error(T_est, T_gt):
    """(translation error in metres, rotation error in degrees) of an estimated relative pose"""
    D = np.linalg.inv(T_gt) @ T_est
    return float(np.linalg.norm(D[:3, 3])), float(np.degrees(np.arccos(np.clip((np.trace(D[:3, :3]) - 1) / 2, -1, 1))))


def tracking(trk, K, leaf, n_frames):
    full = []
    for k in range(n_frames):
        I, Z = synth.render(W, H, pose(k), frame_id=k)
        full.append(capi.RgbdImagePyramid.from_raw(*synth.to_raw(I, Z), K, 4))
    m = capi.KeyframeMap(trk, leaf)
    rows = []
    for k in range(1, n_frames):
        m.insert(k - 1, full[k - 1], pose(k - 1), None)
        gt = np.linalg.inv(pose(k - 1)) @ pose(k)
        model = m.render_pyramid(pose(k - 1), K, W, H, 4)
        e_model = pose_error(trk.match(model, full[k]).Transformation, gt)
        e_kf = pose_error(trk.match(full[k - 1], full[k]).Transformation, gt)
        rows.append({"frame": k, "keyframes_in_map": k, "coverage": round(model.render_stats["covered_pixels"] / float(W * H), 4),
                     "model_view": [round(e_model[0], 6), round(e_model[1], 5)], "previous_keyframe": [round(e_kf[0], 6), round(e_kf[1], 5)]})
        print(f"  frame {k}: model view {rows[-1]['model_view']}  previous keyframe {rows[-1]['previous_keyframe']}  (m, deg)")
    mean = lambda key: [round(float(np.mean([r[key][i] for r in rows])), 6) for i in range(2)]  # noqa: E731
    return {"format": "[translation error m, rotation error deg] of the relative pose", "step_m": round(float(np.linalg.norm(
        (np.linalg.inv(pose(0)) @ pose(1))[:3, 3])), 5), "frames": rows, "mean_model_view": mean("model_view"),
        "mean_previous_keyframe": mean("previous_keyframe")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10, 50, 200])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--leaf", type=float, default=0.01)
    ap.add_argument("--track-frames", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_render.json"))
    a = ap.parse_args()
    K = synth.intrinsics_for(W, H)
    trk = capi.DenseTracker()
    report = {"image": [W, H], "view": [W, H], "leaf": a.leaf, "reps": a.reps, "format": "[median, min, max] ms", "sizes": {}}
    pyrs, bgrs = [], []
    m = capi.KeyframeMap(trk, a.leaf)
    for N in sorted(a.sizes):  # one map, grown from size to size: the same keyframes scripts/keyframe_map_timing.py inserts
        for k in range(len(pyrs), N):
            I, Z = synth.render(W, H, pose(k), frame_id=k)
            bgr, raw = synth.to_raw(I, Z)
            pyrs.append(capi.RgbdImagePyramid.from_raw(bgr, raw, K, 1))
            bgrs.append(bgr if k % 2 == 0 else None)
            m.insert(k, pyrs[k], pose(k), bgrs[k])
        view_pose = pose((N - 1) / 2.0)
        t = {op: {"device_ms": [], "call_ms": []} for op in ("render", "render_pyramid", "extract")}
        copy_ms = {"render": [], "extract": []}
        stats = None
        for rep in range(a.reps + 1):  # cycle 0 warms every buffer up
            for op, fn in (("render", lambda: m.render(view_pose, K, W, H)), ("render_pyramid", lambda: m.render_pyramid(view_pose, K, W, H, 4)),
                           ("extract", lambda: m.extract())):
                t0 = time.perf_counter()
                out = fn()
                ms = (time.perf_counter() - t0) * 1e3
                if op == "render":
                    stats = out["stats"]
                if rep > 0:
                    t[op]["call_ms"].append(ms)
                    t[op]["device_ms"].append(m.timing()[0])
                    if op in copy_ms:
                        copy_ms[op].append(m.timing()[1])
                del out
        entry = {"voxels": stats["voxels"], "render_stats": stats, "coverage": round(stats["covered_pixels"] / float(W * H), 4),
                 "render_copy_ms": summary(copy_ms["render"]), "extract_copy_ms": summary(copy_ms["extract"])}
        for op, v in t.items():
            entry[op] = {k: summary(x) for k, x in v.items()}
        report["sizes"][str(N)] = entry
        print(f"N = {N}: {stats}")
        for op in t:
            print(f"  {op:15s} device {entry[op]['device_ms']} call {entry[op]['call_ms']} ms")
    del m
    if a.track_frames > 1:
        print("tracking:")
        report["tracking"] = tracking(trk, K, a.leaf, a.track_frames)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
