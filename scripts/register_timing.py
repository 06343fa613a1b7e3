"""Cost of the registered ingest (dvo_amd_pyramid_create_raw_registered) next to the plain raw ingest (dvo_amd_pyramid_create_raw)
in the same run: the yardstick is the plain ingest, nothing else, and no figure is fixed in advance.

Frame: 640x480, 4 levels, 3 channels, the synthetic room in the sensor regime; the depth frames are rendered at a depth camera
(575.8, 575.8, 314.5, 235.5 at 640x480) 2.5 cm beside the colour camera; the remap is fr1's lens.
One process, a warm-up cycle, then medians of 7 with [min, max], the variants interleaved within every cycle:
  plain            dvo_amd_pyramid_create_raw (with a remap: dvo_amd_pyramid_create_raw_remapped)
  registered_fill0 a 640x480 depth frame, one pixel per measurement
  registered_fill1 a 640x480 depth frame, footprints
  registered_half  a 320x240 depth frame, footprints
  each of them without and with the remap, the raw frame from the host and from device memory; and, from device memory,
  collapse         a 640x480 depth frame whose every measurement lands on one pixel (fx = fy = 1e-3): the atomics' worst case
Device time is two events on the internal stream inside the call (dvo_amd_debug_ingest_timing: uploads, clear, splat, count,
every level's planes); call time is the whole call.  Writes profiles/register_ingest.json.
Usage: python scripts/register_timing.py [--reps 7] [--out profiles/register_ingest.json]"""
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
XI_DEPTH_TO_COLOUR = [0.025, 0.001, -0.004, 0.003, -0.005, 0.002]


def summary(v):
    return [round(float(np.median(v)), 5), round(float(np.min(v)), 5), round(float(np.max(v)), 5)]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def depth_K(dw):
    s = dw / 640.0
    return (575.8 * s, 575.8 * s, 314.5 * s, 235.5 * s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_ingest.json"))
    a = ap.parse_args()
    import torch

    K = tum.TUM_FR1_INTRINSICS
    T = synth.se3_exp(XI_DEPTH_TO_COLOUR)
    (grey, raw_z), _, _ = synth.sensor_pair(W, H)
    bgr = np.ascontiguousarray(np.stack([grey, np.roll(grey, 1, 1), np.roll(grey, 1, 0)], -1))
    z_full = synth.sensor_frame(W, H, T, K=depth_K(W))[1]
    z_half = synth.sensor_frame(W // 2, H // 2, T, K=depth_K(W // 2))[1]
    report = {"image": [W, H], "levels": LEVELS, "channels": 3, "reps": a.reps, "format": "[median, min, max] ms"}
    _, ms = timed(lambda: capi.Remap.undistort((W, H), K, (W, H), K, FR1_DIST))
    report["first_device_call_of_the_process_ms"] = round(ms, 4)
    remap = capi.Remap.undistort((W, H), K, (W, H), K, FR1_DIST)
    regs = {"registered_fill0": (capi.Registration(K_depth=depth_K(W), T=T, fill=False), z_full),
            "registered_fill1": (capi.Registration(K_depth=depth_K(W), T=T, fill=True), z_full),
            "registered_half": (capi.Registration(K_depth=depth_K(W // 2), T=T, fill=True), z_half)}
    d_img = torch.from_numpy(bgr).cuda()
    d_z = {id(z): torch.from_numpy(z.view(np.int16).copy()).cuda() for z in (raw_z, z_full, z_half)}
    torch.cuda.synchronize()
    variants, stats = {}, {}
    for source in ("host", "device"):
        for rm in (None, remap):
            tail = f"{source}{'_remapped' if rm else ''}"
            if source == "host":
                variants["plain_" + tail] = lambda r=rm: capi.RgbdImagePyramid.from_raw(bgr, raw_z, K, LEVELS, remap=r)
            else:
                variants["plain_" + tail] = lambda r=rm: capi.RgbdImagePyramid.from_raw_device(d_img.data_ptr(), 3, d_z[id(raw_z)].data_ptr(), W,
                                                                                              H, K, LEVELS, remap=r)
            for name, (reg, z) in regs.items():
                if source == "host":
                    fn = lambda r=rm, g=reg, z=z: capi.RgbdImagePyramid.from_raw(bgr, z, K, LEVELS, remap=r, registration=g)
                else:
                    fn = lambda r=rm, g=reg, z=z: capi.RgbdImagePyramid.from_raw_device(d_img.data_ptr(), 3, d_z[id(z)].data_ptr(), W, H, K, LEVELS,
                                                                                       remap=r, registration=g,
                                                                                       depth_size=(z.shape[1], z.shape[0]))
                variants[f"{name}_{tail}"] = fn
    for fill in (0, 1):
        g = capi.Registration(K_depth=depth_K(W), T=np.eye(4), fill=bool(fill))
        variants[f"collapse_fill{fill}_device"] = lambda g=g: capi.RgbdImagePyramid.from_raw_device(
            d_img.data_ptr(), 3, d_z[id(z_full)].data_ptr(), W, H, (1e-3, 1e-3, K[2], K[3]), LEVELS, registration=g, depth_size=(W, H))
    capi.ingest_timing(True)
    dev = {k: [] for k in variants}
    call = {k: [] for k in variants}
    for rep in range(a.reps + 1):  # cycle 0 warms the slab pool and the staging area up
        for name, fn in variants.items():
            p, ms = timed(fn)
            stats[name] = p.registration_stats
            del p
            if rep > 0:
                call[name].append(ms), dev[name].append(capi.ingest_timing(True))
    capi.ingest_timing(False)
    report["variants"] = {k: {"device_ms": summary(dev[k]), "call_ms": summary(call[k]), "stats": stats[k]} for k in variants}
    report["over_plain"] = {}
    for k in variants:
        base = "plain_device" if k.startswith("collapse") else "plain_" + k.split("_", 2)[2] if k.startswith("registered") else None
        if base:
            report["over_plain"][k] = {"device": round(float(np.median(dev[k]) / np.median(dev[base])), 3),
                                       "call": round(float(np.median(call[k]) / np.median(call[base])), 3)}
    for k, v in report["variants"].items():
        print(f"  {k:36s} device {v['device_ms']} call {v['call_ms']}")
    print("  over the plain ingest of the same source:", report["over_plain"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
