"""Frame preparation one frame per call against one call for all frames, in the same process: 64 raw 640x480 frames, 4 levels,
each pyramid with its first point selection.

  (a) loop    64 x dvo_amd_pyramid_create_raw, each followed by the first dvo_amd_pyramid_select (count only): the path a caller
              had before the batched entry, and the baseline
  (b) batch   one dvo_amd_pyramid_create_raw_batch with build_selection

Both from raw frames resident in device memory and from host frames.  After a warm-up of each variant that fills the slab pool
(64 slabs), three repeats, (a) and (b) interleaved within every repeat; a repeat times `--rounds` rounds of 64 frames back to back
(wall clock around the calls, which end in a stream synchronise; the pyramids are released outside the timed window).  No figure
is fixed in advance: the batch stands if it beats the loop from device memory by more than the spread of the repeats.
A last, untimed pass with dvo_amd_debug_ingest_timing on records the device time of the stages: per frame the build and the
selection of (a), per call the whole of (b).
Writes profiles/ingest_batch.json.
Usage: python scripts/ingest_batch_bench.py [--count 64] [--repeats 3] [--rounds 4] [--out profiles/ingest_batch.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dvo_slam_amd import capi, synth, tum  # noqa: E402

W, H, LEVELS = 640, 480, 4
SCALE = 1.0 / 5000.0
SEL = (0.0, 0.0)  # DenseTracker::Config's default thresholds: the selection a default tracker asks for


def make_frames(count):
    """`count` different BGR + depth frames: four rendered views of the synthetic room, shifted by a frame-dependent offset"""
    views = [synth.sensor_frame(W, H, synth.se3_exp(np.array([0.01, -0.004, 0.006, 0.003, -0.002, 0.004]) * v), frame_id=v) for v in range(4)]
    frames = []
    for f in range(count):
        grey, z = views[f % 4]
        grey, z = np.roll(grey, f // 4, 1), np.roll(z, f // 4, 1)
        bgr = np.ascontiguousarray(np.stack([grey, np.roll(grey, 1, 1), np.roll(grey, 1, 0)], -1), np.uint8)
        frames.append((bgr, np.ascontiguousarray(z, np.uint16)))
    return frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_batch.json"))
    a = ap.parse_args()
    import torch

    L = capi.lib()
    if L.dvo_amd_device_count() < 1:
        raise SystemExit("needs a GPU: there is nothing to measure without one")
    n = a.count
    K = [float(k) for k in tum.TUM_FR1_INTRINSICS]
    frames = make_frames(n)
    d_img = [torch.from_numpy(b).cuda() for b, _ in frames]
    d_z = [torch.from_numpy(z.view(np.int16).copy()).cuda() for _, z in frames]
    torch.cuda.synchronize()
    ptrs = {"host": ([b.ctypes.data for b, _ in frames], [z.ctypes.data for _, z in frames]),
            "device": ([t.data_ptr() for t in d_img], [t.data_ptr() for t in d_z])}

    def release(handles):
        for h in handles:
            L.dvo_amd_pyramid_release(h)

    def loop(source):
        ip, zp = ptrs[source]
        on_device = int(source == "device")
        handles, cnt = [], C.c_int()
        for f in range(n):
            h = C.c_void_p()
            capi._check(L.dvo_amd_pyramid_create_raw(0, ip[f], 3, 3 * W, zp[f], W, SCALE, on_device, W, H, *K, LEVELS, 0.0, C.byref(h)), "create_raw")
            capi._check(L.dvo_amd_pyramid_select(h, 0, SEL[0], SEL[1], C.byref(cnt), None), "select")
            handles.append(h)
        return handles

    def batch(source):
        ip, zp = ptrs[source]
        b = capi.CRawBatch()
        b.count, b.images, b.depths, b.timestamps = n, (C.c_void_p * n)(*ip), (C.c_void_p * n)(*zp), None
        b.channels, b.image_stride_bytes, b.depth_stride, b.depth_scale, b.on_device = 3, 3 * W, W, SCALE, int(source == "device")
        b.width, b.height, b.levels = W, H, LEVELS
        b.fx, b.fy, b.ox, b.oy = K
        b.build_selection, b.intensity_threshold, b.depth_threshold = 1, SEL[0], SEL[1]
        out = (C.c_void_p * n)()
        capi._check(L.dvo_amd_pyramid_create_raw_batch(0, C.byref(b), out), "create_raw_batch")
        return [C.c_void_p(out[f]) for f in range(n)]

    variants = [(kind, source) for source in ("device", "host") for kind in ("loop", "batch")]
    run = {"loop": loop, "batch": batch}

    def timed_rounds(kind, source, rounds):
        total = 0.0
        for _ in range(rounds):
            t0 = time.perf_counter()
            handles = run[kind](source)
            total += time.perf_counter() - t0
            release(handles)
        return total

    # the batch and the loop build the same thing: counts of level 0 of every frame, before anything is timed
    hb, hl = batch("device"), loop("device")
    cb, cl = C.c_int(), C.c_int()
    for f in range(n):
        capi._check(L.dvo_amd_pyramid_select(hb[f], 0, SEL[0], SEL[1], C.byref(cb), None), "select")
        capi._check(L.dvo_amd_pyramid_select(hl[f], 0, SEL[0], SEL[1], C.byref(cl), None), "select")
        assert cb.value == cl.value > 0, (f, cb.value, cl.value)
    release(hb), release(hl)
    for kind, source in variants:  # warm-up: every variant once more, the slab pool full
        timed_rounds(kind, source, 1)
    seconds = {v: [] for v in variants}
    for _ in range(a.repeats):
        for v in variants:
            seconds[v].append(timed_rounds(v[0], v[1], a.rounds))
    report = {"image": [W, H], "levels": LEVELS, "count": n, "repeats": a.repeats, "rounds_per_repeat": a.rounds,
              "selection_thresholds": list(SEL), "batch_build_stats": capi.batch_build_stats(), "frames_per_second": {}, "batch_over_loop": {}}
    for source in ("device", "host"):
        rates = {kind: [a.rounds * n / s for s in seconds[kind, source]] for kind in ("loop", "batch")}
        for kind in ("loop", "batch"):
            r = rates[kind]
            report["frames_per_second"][f"{kind}_{source}"] = {"repeats": [round(x, 1) for x in r], "median": round(float(np.median(r)), 1),
                                                               "spread": round(float(max(r) - min(r)), 1)}
        ratios = [b / l for b, l in zip(rates["batch"], rates["loop"])]
        report["batch_over_loop"][source] = {"repeats": [round(x, 3) for x in ratios], "median": round(float(np.median(ratios)), 3),
                                             "worst_case": round(min(rates["batch"]) / max(rates["loop"]), 3)}
    # device time of the stages, untimed pass
    capi.ingest_timing(True)
    stages = {}
    for source in ("device", "host"):
        ip, zp = ptrs[source]
        build_ms, select_ms, cnt = [], [], C.c_int()
        for f in range(n):
            h = C.c_void_p()
            capi._check(L.dvo_amd_pyramid_create_raw(0, ip[f], 3, 3 * W, zp[f], W, SCALE, int(source == "device"), W, H, *K, LEVELS, 0.0, C.byref(h)),
                        "create_raw")
            build_ms.append(capi.ingest_timing(True))
            capi._check(L.dvo_amd_pyramid_select(h, 0, SEL[0], SEL[1], C.byref(cnt), None), "select")
            select_ms.append(capi.ingest_timing(True))
            L.dvo_amd_pyramid_release(h)
        release(batch(source))
        stages[source] = {"loop_build_device_ms_per_frame": round(float(np.median(build_ms)), 5),
                          "loop_selection_device_ms_per_frame": round(float(np.median(select_ms)), 5),
                          "batch_device_ms_per_call": round(capi.ingest_timing(True), 5)}
        stages[source]["batch_device_ms_per_frame"] = round(stages[source]["batch_device_ms_per_call"] / n, 5)
    capi.ingest_timing(False)
    report["device_time"] = stages
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
