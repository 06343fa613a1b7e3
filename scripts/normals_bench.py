"""What surface normals cost on the device at 640x480 with four levels, against the route a user had before, from one run:

  plane_r*   dvo_amd_pyramid_normals of level 0 with window radius r: one launch, normals and facing copied to the host
  mask_r*    dvo_amd_mask_from_normals over all four levels with radius r on every level: one launch, nothing copied back
  host_r*    the route without the entries: every level's depth plane downloaded, the numpy restatement of the rule
             (tests/normals_ref.py), the result uploaded with dvo_amd_mask_create_levels

device_ms is the launch alone between two events (dvo_amd_debug_normals_timing); call_ms is the host clock around the synchronous
call.  Medians of --samples timed calls after a warm-up, with [min, max]; the host route is timed --host-samples times.  The frame
is the sensor-regime frame of dvo_slam_amd.synth; ratio 0.02, facing = cosine to the viewing ray, min_facing 0.5.
One process, one GPU.  Writes profiles/normals.json.
Usage: python scripts/normals_bench.py [--samples 9] [--host-samples 3] [--out PATH]"""
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
RADII = (0, 1, 3, 8)
RATIO, MIN_FACING = 0.02, 0.5


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--host-samples", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals.json"))
    a = ap.parse_args()

    import normals_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("normals_bench.py needs a HIP device (no CPU fallback)")
    img, raw = synth.sensor_frame(W, H, frame_id=0)
    pyr = capi.RgbdImagePyramid.from_raw(img, raw, synth.intrinsics_for(W, H), LEVELS)
    capi.normals_timing(enable=True)

    def timed(call, samples):
        call()  # warm-up
        host, device = [], []
        for _ in range(samples):
            t0 = time.perf_counter()
            call()
            host.append((time.perf_counter() - t0) * 1e3)
            device.append(capi.normals_timing(enable=True)["ms"])
        return {"call_ms": spread(host), "device_ms": spread(device)}

    out = {"size": [W, H], "levels": LEVELS, "ratio": RATIO, "min_facing": MIN_FACING, "samples": a.samples,
           "host_samples": a.host_samples, "cases": {}}
    for r in RADII:
        opt = capi.normal_options(radius=r, depth_step_ratio=RATIO, facing=capi.NORMAL_FACING_RAY)
        out["cases"][f"plane_r{r}"] = timed(lambda: pyr.normals(0, opt), a.samples)
        out["cases"][f"mask_r{r}"] = timed(lambda: capi.SelectionMask.from_normals(pyr, MIN_FACING, opt), a.samples)

        def host_route():
            planes = []
            for l in range(LEVELS):
                Z, K = pyr.plane(l, 1), pyr.level_info(l)[2]
                planes.append(ref.mask_ref(Z, K, MIN_FACING, 0, radius=r, ratio=RATIO, facing=ref.FACING_RAY)[0])
            return capi.SelectionMask.from_levels(planes)

        times = []
        for _ in range(a.host_samples):
            t0 = time.perf_counter()
            m = host_route()
            times.append((time.perf_counter() - t0) * 1e3)
        out["cases"][f"host_r{r}"] = {"call_ms": spread(times)}
        # the two routes build the same mask
        dev = capi.SelectionMask.from_normals(pyr, MIN_FACING, opt)
        assert all(np.array_equal(dev.download(l), m.download(l)) for l in range(LEVELS)), r
        c = out["cases"]
        print(f"r = {r}: plane {c[f'plane_r{r}']['device_ms']['median']:.4f} ms device / {c[f'plane_r{r}']['call_ms']['median']:.3f} ms call;"
              f" mask {c[f'mask_r{r}']['device_ms']['median']:.4f} ms device / {c[f'mask_r{r}']['call_ms']['median']:.3f} ms call;"
              f" host route {c[f'host_r{r}']['call_ms']['median']:.1f} ms", flush=True)
    capi.normals_timing(enable=False)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
