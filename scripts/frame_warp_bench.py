"""What the frame warps cost on the 640x480, four-level workload of bench.py (keyframe 0 = the fixed frame, the first current frame
of the synthetic workload = the moving frame, the pose a match returned): dvo_amd_warp_inverse and dvo_amd_warp_forward at level
0 as planes and as pyramids, for n = 1 and for n = 64 items in one call, and next to them, from the same run, the only way to
get the same result without these entries:

  host round trip   download of the level-0 planes, the numpy restatement (tests/warp_ref.py), dvo_amd_pyramid_create of the result

  device_ms   between two events on the library's internal stream around the call's own launches (dvo_amd_debug_warp_timing): one
              kernel for an inverse warp, three for a forward warp; not the table's upload, the copies back or a pyramid's build
  call_ms     host clock around the call, which ends in its synchronisation (a pyramid form: in its builder's): scratch, upload,
              launches, and either the copies of the planes to the host or the build of the pyramids

Medians of --samples timed calls after a warm-up, the variants interleaved call by call, with [min, max].  bytes: what the
operation must move per call -- inverse: the fixed depth (4 B/px), four 8-byte taps counted once (8), two planes out (8); forward:
the moving depth and grey value (8), the 64-bit depth buffer cleared, updated and read (24), three planes out (12) -- and the
fraction of the HBM peak (8.0 TB/s) that device_ms implies.  Also the use: the mean absolute grey difference between the fixed
frame and the inverse-warped moving frame over the warped pixels, at the match's pose and at the identity.  One process, one GPU.
Writes profiles/frame_warp.json.
Usage: python scripts/frame_warp_bench.py [--samples 7] [--out PATH]"""
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
HBM_PEAK = 8.0e12


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_warp.json"))
    a = ap.parse_args()

    import bench
    import warp_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("frame_warp_bench.py needs a HIP device (no CPU fallback)")
    K = synth.intrinsics_for(W, H)
    f0, f1 = bench.workload_ref_frame(synth, W, H, 0, 0), bench.workload_cur_frame(synth, W, H, 0, 0)
    fixed, moving = capi.RgbdImagePyramid(f0[0], f0[1], K, LEVELS), capi.RgbdImagePyramid(f1[0], f1[1], K, LEVELS)
    trk = capi.DenseTracker(capi.Config(FirstLevel=LEVELS - 1, LastLevel=0))
    T = trk.match(fixed, moving).Transformation
    n_px = W * H
    N = 64
    footprint = dict(splat=capi.WARP_SPLAT_FOOTPRINT)

    def planes(p):
        return p.plane(0, 0), p.plane(0, 1), tuple(p.level_info(0)[2])

    def host_inverse():
        f, m = planes(fixed), planes(moving)
        I, Z, _, cls = ref.inverse_ref((f[1], f[2]), m, T)
        I, Z = ref.empty_rule(I, Z, cls, 0.0)
        return capi.RgbdImagePyramid(I, Z, K, LEVELS)

    def host_forward():
        d, i, x, _ = ref.forward_ref(planes(moving), T, None, footprint)
        return capi.RgbdImagePyramid(np.where(x >= 0, i, np.float32(0)), d, K, LEVELS)

    inv_bytes, fwd_bytes = (4 + 8 + 8) * n_px, (8 + 24 + 12) * n_px
    device_ops = {
        "inverse_planes_n1": (lambda: moving.warp_inverse(fixed, T, 0), inv_bytes),
        "inverse_pyramid_n1": (lambda: moving.warp_inverse(fixed, T), inv_bytes),
        "inverse_planes_n64": (lambda: capi.warp_inverse_many([fixed] * N, [moving] * N, [T] * N, 0), N * inv_bytes),
        "inverse_pyramid_n64": (lambda: capi.warp_inverse_many([fixed] * N, [moving] * N, [T] * N), N * inv_bytes),
        "forward_nearest_planes_n1": (lambda: moving.warp_forward(T, None, 0), fwd_bytes),
        "forward_footprint_planes_n1": (lambda: moving.warp_forward(T, None, 0, footprint), fwd_bytes),
        "forward_footprint_pyramid_n1": (lambda: moving.warp_forward(T, None, None, footprint), fwd_bytes),
        "forward_footprint_planes_n64": (lambda: capi.warp_forward_many([moving] * N, [T] * N, None, 0, footprint), N * fwd_bytes),
        "forward_footprint_pyramid_n64": (lambda: capi.warp_forward_many([moving] * N, [T] * N, None, None, footprint), N * fwd_bytes),
    }
    before = {"host_round_trip_inverse": host_inverse, "host_round_trip_forward": host_forward}
    capi.warp_timing(True)
    call = {k: [] for k in list(device_ops) + list(before)}
    device = {k: [] for k in device_ops}
    for fn in [v[0] for v in device_ops.values()] + list(before.values()):  # warm-up: code objects loaded, pools grown
        fn()
        fn()
    for _ in range(a.samples):
        for k, (fn, _) in device_ops.items():
            t0 = time.perf_counter()
            got = fn()
            call[k].append((time.perf_counter() - t0) * 1e3)
            device[k].append(capi.warp_timing(True)["ms"])
            del got
        for k, fn in before.items():
            t0 = time.perf_counter()
            got = fn()
            call[k].append((time.perf_counter() - t0) * 1e3)
            del got
    capi.warp_timing(False)

    def mean_abs_difference(pose):
        I = moving.warp_inverse(fixed, pose, 0)[0]
        m = ~np.isnan(I)
        return round(float(np.abs(f0[0][m].astype(np.float64) - I[m]).mean()), 4), int(m.sum())

    report = {"image": [W, H], "levels": LEVELS, "samples": a.samples, "items_per_many_call": N, "hbm_peak_bytes_per_s": HBM_PEAK,
              "build_id": capi.build_id(),
              "what": "device_ms: two events around the call's own launches; call_ms: host clock around the synchronous call; one process",
              "ops": {}, "before": {}}
    for k, (_, nbytes) in device_ops.items():
        d = spread(device[k])
        report["ops"][k] = {"device_ms": d, "call_ms": spread(call[k]), "bytes": nbytes,
                            "fraction_of_hbm_peak": round(nbytes / (d["median"] * 1e-3) / HBM_PEAK, 5) if d["median"] > 0 else None}
    for k in before:
        report["before"][k] = {"call_ms": spread(call[k])}
    ops, bef = report["ops"], report["before"]
    report["ratios"] = {
        "host_round_trip_over_device_call_inverse": round(bef["host_round_trip_inverse"]["call_ms"]["median"] / ops["inverse_pyramid_n1"]["call_ms"]["median"], 2),
        "host_round_trip_over_device_call_forward": round(bef["host_round_trip_forward"]["call_ms"]["median"] / ops["forward_footprint_pyramid_n1"]["call_ms"]["median"], 2),
        "inverse_pyramid_n64_call_over_64_n1_calls": round(ops["inverse_pyramid_n64"]["call_ms"]["median"] / (N * ops["inverse_pyramid_n1"]["call_ms"]["median"]), 4),
        "forward_pyramid_n64_call_over_64_n1_calls": round(ops["forward_footprint_pyramid_n64"]["call_ms"]["median"] / (N * ops["forward_footprint_pyramid_n1"]["call_ms"]["median"]), 4),
    }
    at_T, at_I = mean_abs_difference(T), mean_abs_difference(np.eye(4))
    report["use"] = {"mean_abs_grey_difference_at_T": at_T[0], "warped_pixels_at_T": at_T[1],
                     "mean_abs_grey_difference_at_identity": at_I[0], "warped_pixels_at_identity": at_I[1]}
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
