"""What fusing tracked frames' depth into their keyframe costs at 640x480 with four levels, and what it buys, from one run:

  fuse_n1, fuse_n8, fuse_n30   dvo_amd_pyramid_fuse_depth with 1, 8 and 30 frames: one fusion launch, then the pyramid's build
  many_16x8                    dvo_amd_pyramid_fuse_depth_many: 16 keyframes with 8 frames each, one fusion launch, 16 builds
  host_n*                      what the call replaces, on the same build: n + 1 depth planes downloaded, the numpy restatement
                               (tests/depth_fusion_ref.py), dvo_amd_pyramid_create of the result

device_ms is the fusion launch alone between two events (dvo_amd_debug_fuse_timing); call_ms is the host clock around the
synchronous call: tables, launch, synchronisation, the build of the new pyramid(s).  Medians of --samples timed calls after a
warm-up, with [min, max]; the host route is timed --host-samples times.  bytes: what the launch must move at least (the keyframe's
depth read and the fused plane written once, every frame's depth plane read once) and what its loads ask for (four taps per pixel
and frame), with the fraction of the 8 TB/s HBM peak the first amounts to at device_ms.  The frames are the sensor-regime stream
of dvo_slam_amd.synth at its ground-truth poses.
tracking: a frame at synth.XI_GT_PAIR tracked against the unfused keyframe and against the keyframe fused with 8 frames (at the
ground-truth poses and at the poses match() returned), pose error against the ground truth.
One process, one GPU.  Writes profiles/depth_fusion.json.
Usage: python scripts/depth_fusion_bench.py [--samples 7] [--host-samples 3] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, LEVELS = 640, 480, 4
COUNTS = (1, 8, 30)
MANY_KEYFRAMES, MANY_FRAMES = 16, 8
HBM_PEAK = 8e12  # bytes / s


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--host-samples", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_fusion.json"))
    a = ap.parse_args()

    import depth_fusion_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("depth_fusion_bench.py needs a HIP device (no CPU fallback)")
    K = synth.intrinsics_for(W, H)
    n_frames = max(max(COUNTS) + 1, MANY_KEYFRAMES + MANY_FRAMES)
    poses = [synth.se3_exp(t * synth.XI_STEP_STREAM) for t in range(n_frames)]
    host = [synth.raw_to_float(*synth.sensor_frame(W, H, poses[t], frame_id=t)) for t in range(n_frames)]
    pyr = [capi.RgbdImagePyramid(I, Z, K, LEVELS) for I, Z in host]
    px = W * H

    def relative(j, k):
        return np.linalg.inv(poses[j]) @ poses[k]

    def fuse(n):
        return pyr[0].fuse_depth(pyr[1:n + 1], poses[1:n + 1])

    many_args = ([pyr[j] for j in range(MANY_KEYFRAMES)],
                 [[pyr[j + 1 + k] for k in range(MANY_FRAMES)] for j in range(MANY_KEYFRAMES)],
                 [[relative(j, j + 1 + k) for k in range(MANY_FRAMES)] for j in range(MANY_KEYFRAMES)])

    def many():
        return capi.RgbdImagePyramid.fuse_depth_many(*many_args)

    def host_route(n):
        planes = [p.plane(0, 1) for p in pyr[:n + 1]]
        fused = ref.fuse_ref((planes[0], K), [(z, K) for z in planes[1:]], poses[1:n + 1])[0]
        return capi.RgbdImagePyramid(host[0][0], fused, K, LEVELS)

    # the two routes give the same pyramid
    for n in (1, 8):
        got, want = fuse(n), host_route(n)
        assert all(np.array_equal(got.plane(l, p), want.plane(l, p), equal_nan=True) for l in range(LEVELS) for p in range(6)), n

    routes = {f"fuse_n{n}": (lambda n=n: fuse(n)) for n in COUNTS}
    routes[f"many_{MANY_KEYFRAMES}x{MANY_FRAMES}"] = many
    device_ms, call_ms = {k: [] for k in routes}, {k: [] for k in routes}
    capi.fuse_timing(True)
    try:
        for fn in routes.values():  # warm-up: code objects loaded, pools and areas grown
            fn()
            fn()
        for _ in range(a.samples):
            for k, fn in routes.items():
                t0 = time.perf_counter()
                out = fn()
                call_ms[k].append((time.perf_counter() - t0) * 1e3)
                device_ms[k].append(capi.fuse_timing(True))
                del out
    finally:
        capi.fuse_timing(False)
    host_ms = {}
    for n in COUNTS:
        host_route(n)
        times = []
        for _ in range(a.host_samples):
            t0 = time.perf_counter()
            out = host_route(n)
            times.append((time.perf_counter() - t0) * 1e3)
            del out
        host_ms[f"host_n{n}"] = spread(times, 2)

    def bytes_of(keyframes, frames_each):
        least = keyframes * px * (8 + 4 * frames_each)
        asked = keyframes * px * (8 + 16 * frames_each)
        return least, asked

    report = {"image": [W, H], "levels": LEVELS, "samples": a.samples, "host_samples": a.host_samples, "sample": "bilinear",
              "what": "device_ms: the fusion launch between two events; call_ms: host clock around the synchronous call, the "
                      "build of the new pyramid(s) included; routes interleaved; one process",
              "routes": {}, "host_route_ms": host_ms}
    for k in routes:
        keyframes, frames_each = (MANY_KEYFRAMES, MANY_FRAMES) if k.startswith("many") else (1, int(k[len("fuse_n"):]))
        least, asked = bytes_of(keyframes, frames_each)
        d = spread(device_ms[k])
        report["routes"][k] = {"keyframes": keyframes, "frames_per_keyframe": frames_each, "device_ms": d, "call_ms": spread(call_ms[k]),
                               "bytes_least": least, "bytes_asked_for": asked,
                               "fraction_of_hbm_peak": round(least / (d["median"] * 1e-3) / HBM_PEAK, 4)}
    report["ratios"] = {f"host_n{n}_over_call": round(host_ms[f"host_n{n}"]["median"] / report["routes"][f"fuse_n{n}"]["call_ms"]["median"], 1)
                        for n in COUNTS}
    report["ratios"]["many_over_16_calls_of_n8"] = round(
        report["routes"][f"many_{MANY_KEYFRAMES}x{MANY_FRAMES}"]["call_ms"]["median"] / (MANY_KEYFRAMES * report["routes"]["fuse_n8"]["call_ms"]["median"]), 3)

    # what it buys: a frame tracked against the unfused and against the fused keyframe
    trk = capi.DenseTracker(capi.Config(FirstLevel=LEVELS - 1, LastLevel=0))
    T_gt = synth.se3_exp(synth.XI_GT_PAIR)
    probe = capi.RgbdImagePyramid(*synth.raw_to_float(*synth.sensor_frame(W, H, T_gt, frame_id=101)), K, LEVELS)
    tracked = [trk.match(pyr[0], p).Transformation for p in pyr[1:9]]
    fused_gt = pyr[0].fuse_depth(pyr[1:9], poses[1:9], dict(depth_sigmas=3.0))
    fused_tracked = pyr[0].fuse_depth(pyr[1:9], tracked, dict(depth_sigmas=3.0))
    truth = synth.render(W, H, np.eye(4), nan_fraction=0, hole=False)[1]

    def rms_mm(z):
        both = np.isfinite(z) & np.isfinite(truth)
        return round(1e3 * float(np.sqrt(np.mean((z[both].astype(np.float64) - truth[both]) ** 2))), 3)

    report["tracking"] = {
        "frames_fused": 8, "depth_sigmas": 3.0,
        "depth_rms_mm": {"unfused": rms_mm(host[0][1]), "fused_at_ground_truth_poses": rms_mm(fused_gt.plane(0, 1)),
                         "fused_at_tracked_poses": rms_mm(fused_tracked.plane(0, 1))},
        "pose_error": {"unfused": synth.pose_error(trk.match(pyr[0], probe).Transformation, T_gt),
                       "fused_at_ground_truth_poses": synth.pose_error(trk.match(fused_gt, probe).Transformation, T_gt),
                       "fused_at_tracked_poses": synth.pose_error(trk.match(fused_tracked, probe).Transformation, T_gt)},
        "tracked_pose_error_max": max(synth.pose_error(T, P) for T, P in zip(tracked, poses[1:9])),
    }
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
