"""Cost of the rectifying ingest (dvo_amd_pyramid_create_raw_remapped) next to the plain raw ingest (dvo_amd_pyramid_create_raw)
in the same run: the yardstick for "cheap enough" is the plain ingest, nothing else, and no figure is fixed in advance.

Frame: 640x480, 4 levels, the synthetic room in the sensor regime; the remap is fr1's lens (dvo_amd_remap_create_undistort).
One process, a warm-up cycle, then medians of 7 with [min, max], the variants interleaved within every cycle:
  raw frames from the host and from device memory, 1 and 3 channels, plain and remapped: device time (two events on the internal
  stream inside the call, dvo_amd_debug_ingest_timing: uploads, ingest or remap, every level's planes) and whole-call time
  dvo_amd_remap_create_undistort and dvo_amd_remap_create (the same table from the host): whole-call time, once each, after
  one call that takes the process's start-up cost (recorded apart)
Writes profiles/rectify_ingest.json.
Usage: python scripts/rectify_timing.py [--reps 7] [--out profiles/rectify_ingest.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dvo_slam_amd import capi, synth, tum  # noqa: E402

W, H, LEVELS = 640, 480, 4
FR1_DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)


def summary(v):
    return [round(float(np.median(v)), 5), round(float(np.min(v)), 5), round(float(np.max(v)), 5)]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_ingest.json"))
    a = ap.parse_args()
    import torch

    K = tum.TUM_FR1_INTRINSICS
    (grey, raw_z), _, _ = synth.sensor_pair(W, H)
    bgr = np.ascontiguousarray(np.stack([grey, np.roll(grey, 1, 1), np.roll(grey, 1, 0)], -1))
    report = {"image": [W, H], "levels": LEVELS, "reps": a.reps, "format": "[median, min, max] ms"}
    # the first device call of the process pays for HIP's start-up, the code objects and the internal stream: recorded apart
    _, ms = timed(lambda: capi.Remap.undistort((W, H), K, (W, H), K, FR1_DIST))
    report["first_device_call_of_the_process_ms"] = round(ms, 4)
    remap, ms = timed(lambda: capi.Remap.undistort((W, H), K, (W, H), K, FR1_DIST))
    report["remap_create_undistort_call_ms"] = round(ms, 4)
    mx, my = remap.download()
    host_remap, ms = timed(lambda: capi.Remap.from_maps(mx, my, (W, H)))
    report["remap_create_call_ms"] = round(ms, 4)
    report["n_inside"] = remap.info()["n_inside"]
    assert host_remap.info() == remap.info()
    d_z = torch.from_numpy(raw_z.view(np.int16).copy()).cuda()
    d_img = {1: torch.from_numpy(grey.copy()).cuda(), 3: torch.from_numpy(bgr).cuda()}
    torch.cuda.synchronize()
    host_img = {1: grey, 3: bgr}
    variants = {}
    for source in ("host", "device"):
        for channels in (1, 3):
            for rm in (None, remap):
                if source == "host":
                    fn = (lambda c=channels, r=rm: capi.RgbdImagePyramid.from_raw(host_img[c], raw_z, K, LEVELS, remap=r))
                else:
                    fn = (lambda c=channels, r=rm: capi.RgbdImagePyramid.from_raw_device(d_img[c].data_ptr(), c, d_z.data_ptr(), W, H, K,
                                                                                         LEVELS, remap=r))
                variants[f"{source}_{channels}ch_{'remapped' if rm else 'plain'}"] = fn
    capi.ingest_timing(True)
    dev = {k: [] for k in variants}
    call = {k: [] for k in variants}
    for rep in range(a.reps + 1):  # cycle 0 warms the slab pool and the staging area up
        for name, fn in variants.items():
            p, ms = timed(fn)
            del p
            if rep > 0:
                call[name].append(ms), dev[name].append(capi.ingest_timing(True))
    capi.ingest_timing(False)
    report["variants"] = {k: {"device_ms": summary(dev[k]), "call_ms": summary(call[k])} for k in variants}
    report["remapped_over_plain"] = {}
    for source in ("host", "device"):
        for channels in (1, 3):
            k = f"{source}_{channels}ch"
            report["remapped_over_plain"][k] = {
                "device": round(float(np.median(dev[k + "_remapped"]) / np.median(dev[k + "_plain"])), 3),
                "call": round(float(np.median(call[k + "_remapped"]) / np.median(call[k + "_plain"])), 3)}
    for k, v in report["variants"].items():
        print(f"  {k:28s} device {v['device_ms']} call {v['call_ms']}")
    print("  remapped / plain:", report["remapped_over_plain"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
