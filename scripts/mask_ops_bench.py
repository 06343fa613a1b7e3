"""What the mask operations cost on the 640x480, four-level workload of bench.py (keyframe 0 and the first current frame of the
synthetic workload, the pose a match returned): dvo_amd_mask_combine, dvo_amd_mask_morph at level-0 radii of 1, 3 and 8
(capi.level_radii), dvo_amd_mask_warp (n = 1) and dvo_amd_mask_warp_many (n = 64), and next to them, from the same run, the two
things that existed before:

  host round trip   download of every level, the numpy restatement (tests/mask_ops_ref.py), SelectionMask.from_levels: the only
                    way to get the same mask without these entries
  mask_create       dvo_amd_mask_create from a level-0 plane in device memory: a kernel chain of the same traffic shape (byte
                    planes in, byte planes out, kept counts), one launch per level

  device_ms   between two events on the library's internal stream, from before the call's first upload to behind its last kernel
              (dvo_amd_debug_mask_ops_timing); the mask operations only -- dvo_amd_mask_create has no such bracket
  call_ms     host clock around the call, which ends in its one synchronisation: allocation, launches, the counter copy

Medians of --samples timed calls after a warm-up, the variants interleaved call by call, with [min, max].  bytes: what the
operation must move per call (every input plane read once, every output plane written once; a warp's gathers counted as one
depth and one byte per target pixel), and the fraction of the HBM peak (8.0 TB/s) that device_ms implies.  One process, one GPU.
Writes profiles/mask_ops.json.
Usage: python scripts/mask_ops_bench.py [--samples 7] [--out PATH]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_ops.json"))
    a = ap.parse_args()

    import torch

    import bench
    import mask_ops_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("mask_ops_bench.py needs a HIP device (no CPU fallback)")
    K = synth.intrinsics_for(W, H)
    f0, f1 = bench.workload_ref_frame(synth, W, H, 0, 0), bench.workload_cur_frame(synth, W, H, 0, 0)
    kf, cur = capi.RgbdImagePyramid(f0[0], f0[1], K, LEVELS), capi.RgbdImagePyramid(f1[0], f1[1], K, LEVELS)
    trk = capi.DenseTracker(capi.Config(FirstLevel=LEVELS - 1, LastLevel=0))
    T = trk.match(kf, cur).Transformation
    m0 = np.ones((H, W), np.uint8)
    m0[H // 5:(3 * H) // 5, W // 4:(2 * W) // 3] = 0
    A = capi.SelectionMask.from_level0(m0, LEVELS)
    B = capi.SelectionMask.from_budget(kf, capi.BUDGET_GRID, cell=4)
    d_m0 = torch.from_numpy(m0).cuda()
    torch.cuda.synchronize()
    px = [(W >> l) * (H >> l) for l in range(LEVELS)]
    n_px = sum(px)
    N = 64

    def host_morph(r0):
        planes = [A.download(l) for l in range(LEVELS)]
        return capi.SelectionMask.from_levels([ref.morph_ref(p, ref.ERODE, r) for p, r in zip(planes, capi.level_radii(r0, LEVELS))])

    def host_combine():
        return capi.SelectionMask.from_levels([ref.combine_ref(A.download(l), B.download(l), ref.AND) for l in range(LEVELS)])

    def host_warp():
        out = []
        for l in range(LEVELS):
            pt, ps = (cur.plane(l, 1), tuple(cur.level_info(l)[2])), (kf.plane(l, 1), tuple(kf.level_info(l)[2]))
            out.append(ref.warp_ref(A.download(l), pt, ps, T)[0])
        return capi.SelectionMask.from_levels(out)

    device_ops = {
        "combine_and": (lambda: A & B, 3 * n_px),
        "erode_r1": (lambda: A.erode(1), 2 * n_px),
        "erode_r3": (lambda: A.erode(3), 2 * n_px),
        "erode_r8": (lambda: A.erode(8), 2 * n_px),
        "dilate_r8": (lambda: A.dilate(8), 2 * n_px),
        "warp_n1": (lambda: A.warp(kf, cur, T), (4 + 4 + 1 + 1) * n_px),
        "warp_n64": (lambda: capi.SelectionMask.warp_many([A] * N, [kf] * N, [cur] * N, [T] * N), N * (4 + 4 + 1 + 1) * n_px),
    }
    before = {
        "mask_create_from_device_memory": (lambda: capi.SelectionMask.from_level0_device(d_m0.data_ptr(), W, H, LEVELS),
                                           px[0] + 2 * sum(px[1:]) + sum(px[:-1])),
        "host_round_trip_combine": (host_combine, None),
        "host_round_trip_erode_r1": (lambda: host_morph(1), None),
        "host_round_trip_erode_r8": (lambda: host_morph(8), None),
        "host_round_trip_warp": (host_warp, None),
    }
    capi.mask_ops_timing(True)
    call = {k: [] for k in list(device_ops) + list(before)}
    device = {k: [] for k in device_ops}
    for k, (fn, _) in list(device_ops.items()) + list(before.items()):  # warm-up: code objects loaded, pools grown
        fn()
        fn()
    for _ in range(a.samples):
        for k, (fn, _) in device_ops.items():
            t0 = time.perf_counter()
            m = fn()
            call[k].append((time.perf_counter() - t0) * 1e3)
            device[k].append(capi.mask_ops_timing(True))
            del m
        for k, (fn, _) in before.items():
            t0 = time.perf_counter()
            m = fn()
            call[k].append((time.perf_counter() - t0) * 1e3)
            del m
    capi.mask_ops_timing(False)

    report = {"image": [W, H], "levels": LEVELS, "samples": a.samples, "warp_many_pairs": N, "hbm_peak_bytes_per_s": HBM_PEAK,
              "what": "device_ms: two events inside the call; call_ms: host clock around the synchronous call; one process",
              "ops": {}, "before": {}}
    for k, (_, nbytes) in device_ops.items():
        d = spread(device[k])
        report["ops"][k] = {"device_ms": d, "call_ms": spread(call[k]), "bytes": nbytes,
                            "fraction_of_hbm_peak": round(nbytes / (d["median"] * 1e-3) / HBM_PEAK, 5) if d["median"] > 0 else None}
    for k, (_, nbytes) in before.items():
        report["before"][k] = {"call_ms": spread(call[k]), "bytes": nbytes}
    ops, bef = report["ops"], report["before"]
    report["ratios"] = {
        "host_round_trip_over_device_call_combine": round(bef["host_round_trip_combine"]["call_ms"]["median"] / ops["combine_and"]["call_ms"]["median"], 2),
        "host_round_trip_over_device_call_erode_r1": round(bef["host_round_trip_erode_r1"]["call_ms"]["median"] / ops["erode_r1"]["call_ms"]["median"], 2),
        "host_round_trip_over_device_call_erode_r8": round(bef["host_round_trip_erode_r8"]["call_ms"]["median"] / ops["erode_r8"]["call_ms"]["median"], 2),
        "host_round_trip_over_device_call_warp": round(bef["host_round_trip_warp"]["call_ms"]["median"] / ops["warp_n1"]["call_ms"]["median"], 2),
        "warp_n64_call_over_64_warp_n1_calls": round(ops["warp_n64"]["call_ms"]["median"] / (N * ops["warp_n1"]["call_ms"]["median"]), 4),
    }
    mc = bef["mask_create_from_device_memory"]["call_ms"]["median"]
    for k in device_ops:
        report["ratios"][f"{k}_call_over_mask_create_call"] = round(ops[k]["call_ms"]["median"] / mc, 3)
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
