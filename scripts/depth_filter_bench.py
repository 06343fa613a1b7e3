"""What depth filtering costs on the device at 640x480 with four levels, against the route a user had before, from one run:

  one_r*[_fill2]     dvo_amd_pyramid_filter_depth of one pyramid with window radius r (fill off, or fill radius 2): one launch,
                     then the builder derives the new pyramid
  many64_r*[_fill2]  dvo_amd_pyramid_filter_depth_many of 64 pyramids in one call: one launch, then 64 builds
  single64_r*        the same 64 pyramids in 64 single calls (reported next to many64, not judged)
  host_r*[_fill2]    the route without the entries: the depth plane downloaded, the numpy restatement of the rule
                     (tests/depth_filter_ref.py), dvo_amd_pyramid_create of the two float planes

device_ms is the launch alone between two events (dvo_amd_debug_depth_filter_timing); call_ms is the host clock around the
synchronous call.  Medians of --samples timed calls after a warm-up, with [min, max]; the host route is timed --host-samples times.
The frame is the sensor-regime frame of dvo_slam_amd.synth (the many form: eight frames of that view with their own noise, eight
times each); 3 sigmas, min_support 1.
One process, one GPU.  Writes profiles/depth_filter.json.
Usage: python scripts/depth_filter_bench.py [--samples 9] [--host-samples 3] [--out PATH]"""
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
RADII = (0, 2, 4, 8)
FILLS = (0, 2)
MANY = 64


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--host-samples", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_filter.json"))
    a = ap.parse_args()

    import depth_filter_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("depth_filter_bench.py needs a HIP device (no CPU fallback)")
    K = synth.intrinsics_for(W, H)
    img, raw = synth.sensor_frame(W, H, frame_id=0)
    pyr = capi.RgbdImagePyramid.from_raw(img, raw, K, LEVELS)
    I0 = pyr.plane(0, 0)
    exact = synth.render(W, H)
    many = [pyr] + [capi.RgbdImagePyramid.from_raw(*synth.sensor_from_analytic(*exact, frame_id=k), K, LEVELS) for k in range(1, 8)]
    many = [many[k % 8] for k in range(MANY)]  # 64 inputs over 8 different frames: the kernel reads 64 planes either way
    capi.depth_filter_timing(enable=True)

    def timed(call, samples, device_time=True):
        call()  # warm-up
        host, device = [], []
        for _ in range(samples):
            t0 = time.perf_counter()
            call()
            host.append((time.perf_counter() - t0) * 1e3)
            device.append(capi.depth_filter_timing(enable=True))
        return {"call_ms": spread(host), "device_ms": spread(device)} if device_time else {"call_ms": spread(host)}

    out = {"size": [W, H], "levels": LEVELS, "range_sigmas": 3.0, "min_support": 1, "many": MANY, "samples": a.samples,
           "host_samples": a.host_samples, "cases": {}}
    c = out["cases"]
    for fill in FILLS:
        for r in RADII:
            tag = f"r{r}" + (f"_fill{fill}" if fill else "")
            opt = capi.depth_filter_options(radius=r, fill_radius=fill)
            c[f"one_{tag}"] = timed(lambda: pyr.filter_depth(opt), a.samples)
            c[f"many64_{tag}"] = timed(lambda: capi.filter_depth_many(many, opt), a.samples)
            if not fill:
                c[f"single64_{tag}"] = timed(lambda: [p.filter_depth(opt) for p in many], a.samples, device_time=False)

            def host_route():
                Z = pyr.plane(0, 1)
                return capi.RgbdImagePyramid(I0, ref.filter_ref(Z, radius=r, fill_radius=fill)[0], K, LEVELS)

            times = []
            for _ in range(a.host_samples):
                t0 = time.perf_counter()
                host = host_route()
                times.append((time.perf_counter() - t0) * 1e3)
            c[f"host_{tag}"] = {"call_ms": spread(times)}
            # the two routes build the same pyramid
            dev = pyr.filter_depth(opt)
            assert all(np.array_equal(dev.plane(l, 1), host.plane(l, 1), equal_nan=True) for l in range(LEVELS)), tag
            line = (f"{tag}: one {c[f'one_{tag}']['device_ms']['median']:.4f} ms device / {c[f'one_{tag}']['call_ms']['median']:.3f} ms call;"
                    f" 64 in one call {c[f'many64_{tag}']['device_ms']['median']:.4f} ms device / {c[f'many64_{tag}']['call_ms']['median']:.3f} ms call;")
            if not fill:
                line += f" 64 single calls {c[f'single64_{tag}']['call_ms']['median']:.3f} ms;"
            print(line + f" host route {c[f'host_{tag}']['call_ms']['median']:.1f} ms", flush=True)
    capi.depth_filter_timing(enable=False)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
