"""What the component filter costs on the 640x480, four-level workload of bench.py, next to the only way to get the same mask
without it, from the same run on the same machine: dvo_amd_mask_filter_components / _many with min_area = level_areas(10), 4- and
8-connected, with and without the keyframe's depth, for 1 item and for 64 items in one call.

  device_ms         between two events on the library's internal stream, from before the call's table upload to behind its last
                    kernel (dvo_amd_debug_components_timing): the five launches
  call_ms           host clock around the call, which ends in its one synchronisation: allocation, launches, the counter copies
  host round trip   download of every level (and of the depth planes where depth takes part), labelling on the host, the area filter
                    with numpy.bincount, SelectionMask.from_levels.  Without depth the labelling is scipy.ndimage.label; with depth
                    ndimage cannot express the edge rule and the labelling is the restatement's scipy.sparse.csgraph
                    (tests/mask_components_ref.py).  For 64 items the host makes its round trips one after the other; 8 of them are timed
                    and the time is multiplied by 8.

The mask is a region of interest with 3 % speckle outside it and 2 % pinholes inside, as a residual mask looks.  Medians of --samples
timed calls after a warm-up, the variants interleaved call by call, with [min, max]; the 64-item host round trips are timed
--host-samples times.  One process, one GPU.  Nothing is tuned towards either side: the figures are printed as they come.
Writes profiles/mask_components.json.
Usage: python scripts/mask_components_bench.py [--samples 7] [--host-samples 2] [--out PATH]"""
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
HOST_TRIPS = 8  # of a 64-item call's 64 sequential host round trips, this many are timed


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--host-samples", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_components.json"))
    a = ap.parse_args()

    from scipy import ndimage

    import bench
    import mask_components_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("mask_components_bench.py needs a HIP device (no CPU fallback)")
    K = synth.intrinsics_for(W, H)
    f0 = bench.workload_ref_frame(synth, W, H, 0, 0)
    kf = capi.RgbdImagePyramid(f0[0], f0[1], K, LEVELS)
    rng = np.random.default_rng(1)
    m0 = np.zeros((H, W), np.uint8)
    m0[H // 5:(4 * H) // 5, W // 6:(5 * W) // 6] = 1
    m0 |= (rng.uniform(size=(H, W)) < 0.03).astype(np.uint8)
    m0 &= 1 - (rng.uniform(size=(H, W)) < 0.02).astype(np.uint8)
    A = capi.SelectionMask.from_level0(m0, LEVELS, capi.MASK_ANY)
    areas = capi.level_areas(10, LEVELS)

    def device(connectivity, depth, n):
        d = kf if depth else None
        if n == 1:
            return lambda: A.filter_components(depth=d, connectivity=connectivity, min_area=areas)
        return lambda: capi.SelectionMask.filter_components_many([A] * n, [d] * n, connectivity=connectivity, min_area=areas)

    def host_once(connectivity, depth):
        planes = []
        for l in range(LEVELS):
            m = A.download(l)
            if depth:
                planes.append(ref.filter_components(m, kf.plane(l, 1), connectivity=connectivity, min_area=areas[l])[0])
                continue
            labels, n = ndimage.label(m, structure=np.ones((3, 3), int) if connectivity == 8 else None)
            keep = np.bincount(labels.ravel(), minlength=n + 1) >= areas[l]
            keep[0] = False
            planes.append(keep[labels].astype(np.uint8))
        return capi.SelectionMask.from_levels(planes)

    def host(connectivity, depth, n):
        return lambda: [host_once(connectivity, depth) for _ in range(min(n, HOST_TRIPS))]

    variants = [(c, d, n) for n in (1, N) for d in (False, True) for c in (4, 8)]
    name = lambda c, d, n: f"{c}-connected, {'mask and depth' if d else 'mask'}, {n} item{'s' if n > 1 else ''}"  # noqa: E731
    # the two sides agree before they are timed
    for c, d, _ in variants[:4]:
        got, want = device(c, d, 1)(), host_once(c, d)
        assert all(np.array_equal(got.download(l), want.download(l)) for l in range(LEVELS)), name(c, d, 1)

    capi.components_timing(True)
    dev_call = {v: [] for v in variants}
    dev_ms = {v: [] for v in variants}
    host_call = {v: [] for v in variants}
    for v in variants:  # warm-up: code objects loaded, the working area grown to the largest call
        device(*v)()
        device(*v)()
    for s in range(a.samples):
        for v in variants:
            t0 = time.perf_counter()
            m = device(*v)()
            dev_call[v].append((time.perf_counter() - t0) * 1e3)
            dev_ms[v].append(capi.components_timing(True))
            del m
            if v[2] == 1 or s < a.host_samples:
                t0 = time.perf_counter()
                m = host(*v)()
                host_call[v].append((time.perf_counter() - t0) * 1e3 * (v[2] / min(v[2], HOST_TRIPS)))
                del m
    capi.components_timing(False)

    report = {"image": [W, H], "levels": LEVELS, "samples": a.samples, "host_samples_64": a.host_samples, "min_area": areas,
              "foreground_level0": int(A.info()["kept"][0]),
              "what": "device_ms: two events inside the call; call_ms: host clock around the synchronous call; host_round_trip_ms: "
                      "download, host labelling, bincount, upload; one process", "variants": {}}
    for v in variants:
        d, c, h = spread(dev_ms[v]), spread(dev_call[v]), spread(host_call[v])
        report["variants"][name(*v)] = {"device_ms": d, "call_ms": c, "host_round_trip_ms": h,
                                        "host_round_trip_over_call": round(h["median"] / c["median"], 2)}
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
