"""What exposure compensation costs on the device at 640x480 with four levels, against the route a user had before, from one run:

  estimate_one     dvo_amd_estimate_exposure of one pair at level 0, default options (refits 4: five launches, five synchronisations)
  estimate_many64  dvo_amd_estimate_exposure_many of 64 pairs in one call: still five launches
  adjust_one       dvo_amd_pyramid_adjust_intensity: one launch, then the builder derives the new pyramid
  host_estimate    the route without the entries: the four level-0 planes downloaded and the numpy restatement of the rule
                   (tests/exposure_ref.py) run on them
  host_adjust      the intensity plane and the depth plane downloaded, numpy, dvo_amd_pyramid_create of the two float planes

device_ms is the launches alone, each between two events, added up (dvo_amd_debug_exposure_timing); call_ms is the host clock around
the synchronous call.  Medians of --samples timed calls after a warm-up, with [min, max]; the host routes are timed --host-samples
times.  The pair is the sensor-regime pair of dvo_slam_amd.synth with the current frame exposed as I -> 0.7 I + 20 (the 64 pairs:
that pair 64 times; the kernel reads 64 pairs of planes either way).  The two routes are compared for equality before anything is
timed.  Recorded next to the timings, asserted nowhere: the pose error of the plain and of the compensated match on that pair.
One process, one GPU.  Writes profiles/exposure.json.
Usage: python scripts/exposure_bench.py [--samples 9] [--host-samples 3] [--out PATH]"""
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
MANY = 64
EXPOSURE = (0.7, 20.0)


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--host-samples", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure.json"))
    a = ap.parse_args()

    import exposure_ref as er
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("exposure_bench.py needs a HIP device (no CPU fallback)")
    ref, cur, T_gt, K = er.exposure_pair(synth, *EXPOSURE, w=W, h=H, scale=1.0)
    reference, current = capi.RgbdImagePyramid(ref[0], ref[1], K, LEVELS), capi.RgbdImagePyramid(cur[0], cur[1], K, LEVELS)
    trk = capi.DenseTracker(capi.Config())

    def host_estimate():
        a_, b_ = [(p.plane(0, 0), p.plane(0, 1), K) for p in (reference, current)]
        return er.estimate_ref(a_, b_)

    def host_adjust(gain, bias):
        return capi.RgbdImagePyramid(er.adjust_ref(current.plane(0, 0), gain, bias), current.plane(0, 1), K, LEVELS)

    # ---- the two routes agree
    estimate = current.estimate_exposure(reference, tracker=trk)
    assert estimate.as_dict() == host_estimate()
    made, restated = current.adjust_intensity(estimate.gain, estimate.bias), host_adjust(estimate.gain, estimate.bias)
    assert all(np.array_equal(made.plane(l, k), restated.plane(l, k), equal_nan=True) for l in range(LEVELS) for k in range(6))

    capi.exposure_timing(enable=True)

    def timed(call, samples, device_time=True):
        call()  # warm-up
        host, device = [], []
        for _ in range(samples):
            t0 = time.perf_counter()
            call()
            host.append((time.perf_counter() - t0) * 1e3)
            device.append(capi.exposure_timing(enable=True))
        return {"call_ms": spread(host), "device_ms": spread(device)} if device_time else {"call_ms": spread(host)}

    c = {
        "estimate_one": timed(lambda: current.estimate_exposure(reference, tracker=trk), a.samples),
        "estimate_many64": timed(lambda: capi.estimate_exposure_many(trk, [reference] * MANY, [current] * MANY), a.samples),
        "adjust_one": timed(lambda: current.adjust_intensity(estimate.gain, estimate.bias), a.samples),
        "host_estimate": timed(host_estimate, a.host_samples, device_time=False),
        "host_adjust": timed(lambda: host_adjust(estimate.gain, estimate.bias), a.host_samples, device_time=False),
    }
    capi.exposure_timing(enable=False)
    plain = trk.match(reference, current)
    result, _, _ = trk.match_compensated(reference, current)
    out = {"size": [W, H], "levels": LEVELS, "many": MANY, "samples": a.samples, "host_samples": a.host_samples, "build_id": capi.build_id(),
           "exposure": {"gain": EXPOSURE[0], "bias": EXPOSURE[1], "true_model": [1.0 / EXPOSURE[0], -EXPOSURE[1] / EXPOSURE[0]]},
           "estimate": {k: v for k, v in estimate.as_dict().items()}, "cases": c,
           "pose_error": {"plain": float(synth.pose_error(T_gt, plain.Transformation)),
                          "compensated": float(synth.pose_error(T_gt, result.Transformation))}}
    for name in ("estimate_one", "estimate_many64", "adjust_one"):
        print(f"{name}: {c[name]['device_ms']['median']:.4f} ms device / {c[name]['call_ms']['median']:.3f} ms call")
    print(f"host_estimate: {c['host_estimate']['call_ms']['median']:.1f} ms; host_adjust: {c['host_adjust']['call_ms']['median']:.1f} ms")
    print("pose error:", out["pose_error"], "estimate:", estimate.gain, estimate.bias, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
