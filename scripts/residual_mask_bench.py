"""What an inlier mask from an alignment's residuals costs on the 640x480, four-level workload of bench.py (keyframe 0 and the first
current frame of the synthetic workload, at the pose and with the precisions a match returned), three ways, from one run:

  call         dvo_amd_mask_from_residuals: one launch over the four levels, one synchronisation
  many_n64     dvo_amd_mask_from_residuals_many over 64 pairs (the same pair 64 times): one launch, one synchronisation
  host_route   what the call replaces, on the same build: dvo_amd_residuals per level (a tracker configured with thresholds
               (-1, -1); a tick through a tracker slot, a scatter to the host), the distance and the threshold in numpy
               (tests/residual_mask_ref.py), dvo_amd_mask_create_levels -- 2 * levels host round trips

call_ms is the host clock around the synchronous call: allocation, launch, copies, the synchronisation.  Medians of --samples
timed calls after a warm-up, the three interleaved call by call, with [min, max].  bytes: what the kernel must move per call (the
reference's depth, {Zx, Zy} and intensity planes read once, six 16 / 8-byte taps of the current gathered per pixel, one mask byte
written), for the record; the kernel is not tuned against it.  The three masks are compared before anything is timed: the host
route must give the planes the call gives.  One process, one GPU.  Writes profiles/residual_mask.json.
Usage: python scripts/residual_mask_bench.py [--samples 9] [--out PATH]"""
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
N = 64


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_mask.json"))
    a = ap.parse_args()

    import bench
    import residual_mask_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("residual_mask_bench.py needs a HIP device (no CPU fallback)")
    K = synth.intrinsics_for(W, H)
    f0, f1 = bench.workload_ref_frame(synth, W, H, 0, 0), bench.workload_cur_frame(synth, W, H, 0, 0)
    kf, cur = capi.RgbdImagePyramid(f0[0], f0[1], K, LEVELS), capi.RgbdImagePyramid(f1[0], f1[1], K, LEVELS)
    trk = capi.DenseTracker(capi.Config(FirstLevel=LEVELS - 1, LastLevel=0))
    result = trk.match(kf, cur)
    T = capi.rigid_inverse(result.Transformation)
    opt = capi.residual_mask_options(result, LEVELS)
    P = [np.array(list(opt.precision[l]), np.float32) for l in range(LEVELS)]
    # the host route's probe: thresholds (-1, -1), so that dvo_amd_residuals walks the validity selection
    probe = capi.DenseTracker(capi.Config(FirstLevel=LEVELS - 1, LastLevel=0, IntensityDerivativeThreshold=-1.0,
                                          DepthDerivativeThreshold=-1.0))
    evaluated = [ref.evaluated_ref(*(kf.plane(l, k) for k in (1, 4, 5))) for l in range(LEVELS)]  # (pose-independent: not timed)
    px = [(W >> l) * (H >> l) for l in range(LEVELS)]

    def call():
        return capi.SelectionMask.from_residuals(trk, kf, cur, T=T, options=opt)

    def many():
        return capi.SelectionMask.from_residuals_many(trk, [kf] * N, [cur] * N, Ts=[T] * N, options=[opt] * N)

    def host_route():
        planes = []
        for l in range(LEVELS):
            res, _ = probe.residuals(kf, cur, l, T)
            planes.append(ref.residual_mask_ref(evaluated[l], res, P[l])[0])
        return capi.SelectionMask.from_levels(planes)

    # the three give the same mask
    want = call()
    for other in (many()[0], many()[N - 1], host_route()):
        assert other.info() == want.info()
        assert all(np.array_equal(other.download(l), want.download(l)) for l in range(LEVELS))
    kept = want.info()["kept"]

    routes = {"call": call, "many_n64": many, "host_route": host_route}
    ms = {k: [] for k in routes}
    for fn in routes.values():  # warm-up: code objects loaded, pools and areas grown
        fn()
        fn()
    for _ in range(a.samples):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            m = fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
            del m
    per_pixel = 4 + 8 + 4 + 4 * 16 + 2 * 16 + 1
    report = {"image": [W, H], "levels": LEVELS, "samples": a.samples, "many_pairs": N, "pixels_per_call": sum(px),
              "kept_per_level": kept, "bytes_per_call": per_pixel * sum(px),
              "what": "call_ms: host clock around the synchronous call; the three routes interleaved; one process",
              "call_ms": {k: spread(v) for k, v in ms.items()}}
    c = report["call_ms"]
    report["ratios"] = {
        "host_route_over_call": round(c["host_route"]["median"] / c["call"]["median"], 2),
        "many_n64_over_64_calls": round(c["many_n64"]["median"] / (N * c["call"]["median"]), 4),
        "many_n64_ms_per_pair": round(c["many_n64"]["median"] / N, 4),
    }
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
