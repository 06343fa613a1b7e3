"""What the signed-distance volume costs at 640x480, four levels: eight sensor keyframes of the synthetic stream fused into a 256^3
and a 512^3 volume over the room (dvo_amd_volume_*), and next to each call, from the same run,

  the map            dvo_amd_map_insert of the eight keyframes (eight calls) / dvo_amd_map_render_pyramid of the same view, leaf = the
                     volume's voxel, in the same interleaved rounds
  host round trip    256^3 only, timed once: the records downloaded and tests/volume_ref.py's vectorised numpy (one frame integrated,
                     one view raycast); the library has no upload entry, so what a host path would add on top is missing from it

  device_ms   between two events on the library's internal stream around the call's own launches (dvo_amd_debug_volume_timing)
  call_ms     host clock around the synchronous call (a raycast pyramid: with its builder)

Medians of --samples timed calls after a warm-up, the variants interleaved call by call, with [min, max].  bytes: what a call must
move -- an integration reads and writes both 8-byte planes of every voxel of its launch box (32 B/voxel; a voxel no frame updates
is not written, so this is an upper bound) and reads 8 B per frame and voxel from the frames; an extract reads plane a twice with
three neighbours each time (counted once per pass: 16 B/voxel) and writes 16 B per point; a raycast is latency-bound gathers and
has no meaningful byte count -- and the fraction of the HBM peak (8.0 TB/s) that device_ms implies at most (hbm_fraction_at_most:
the byte counts are upper bounds).  The extract is timed with its capacity known: one call of the entry.  Also the use: the pose error
of match(model view at the previous keyframe's pose, next frame) for the raycast view and for the map's render.  One process, one
GPU.  Writes profiles/volume.json.
Usage: python scripts/volume_bench.py [--samples 7] [--sizes 256,512] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, LEVELS, N_KF = 640, 480, 4, 8
HBM_PEAK = 8.0e12
EXTENT, ORIGIN = 3.3, (-1.7, -1.35, 0.4)


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume.json"))
    a = ap.parse_args()

    import volume_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("volume_bench.py needs a HIP device (no CPU fallback)")
    K = tuple(float(k) for k in synth.intrinsics_for(W, H))
    poses = [synth.se3_exp(4 * synth.XI_STEP_STREAM * t) for t in range(N_KF + 1)]
    frames = []
    for t, T in enumerate(poses):
        grey, raw_z = synth.sensor_frame(W, H, T, frame_id=t)
        frames.append(synth.raw_to_float(grey, raw_z))
    pyr = [capi.RgbdImagePyramid(I, Z, K, LEVELS) for I, Z in frames]
    ids = list(range(N_KF))
    trk = capi.DenseTracker(capi.Config(FirstLevel=LEVELS - 1, LastLevel=0))
    result = {"build_id": capi.build_id(), "width": W, "height": H, "levels": LEVELS, "keyframes": N_KF, "samples": a.samples, "sizes": {}}

    for n in [int(s) for s in a.sizes.split(",")]:
        voxel = EXTENT / n
        trunc = max(3.0 * voxel, 0.03)
        opt = dict(nx=n, ny=n, nz=n, voxel=voxel, origin=ORIGIN, trunc=trunc, near_z=0.4, far_z=5.0, weight=capi.VOLUME_WEIGHT_SENSOR)
        vol = capi.SurfaceVolume(opt)
        kmap = capi.KeyframeMap(trk, leaf=voxel)
        capi.volume_timing(True)
        state = {"moved": False, "points": None}

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3, capi.volume_timing(True)["ms"]

        def insert1():
            vol.insert(ids[:1], pyr[:1], poses[:1])

        def insert8():
            vol.insert(ids, pyr[:N_KF], poses[:N_KF])

        def move():
            state["moved"] = not state["moved"]
            vol.set_poses([ids[1]], [poses[5] if state["moved"] else poses[1]])

        def raycast():
            vol.raycast_pyramid(poses[N_KF - 1], K, W, H, LEVELS)

        def extract():
            # with the capacity known the binding calls the entry once (count, scan, write); capacity=None would call it twice
            state["points"] = vol.extract(capacity=state["points"])[2]["points"]

        def map_insert8():
            for k in ids:
                kmap.insert(k, pyr[k], poses[k])

        def map_render():
            kmap.render_pyramid(poses[N_KF - 1], K, W, H, LEVELS)

        # the map's two calls run in the same rounds as the volume's, after the same warm-up round (host clock only: the volume's
        # event bracket does not see them)
        variants = {"insert_1": (insert1, lambda: vol.remove(ids[:1])), "insert_8": (insert8, None), "map_insert_8": (map_insert8, None),
                    "move": (move, None), "raycast_pyramid": (raycast, None), "map_render_pyramid": (map_render, None),
                    "extract": (extract, None)}
        samples = {k: [] for k in variants}
        for rep in range(a.samples + 1):  # (the first round is the warm-up)
            for name, (fn, undo) in variants.items():
                s = timed(fn)
                if rep:
                    samples[name].append(s)
                if undo:
                    undo()
            if state["moved"]:
                move()  # back to where it was inserted
            if rep < a.samples:
                vol.remove(ids)
                kmap.remove(ids)
        # the use: the next frame aligned to the model seen from the last keyframe's pose
        gt = np.linalg.inv(poses[N_KF - 1]) @ poses[N_KF]
        err = {}
        for name, model in (("raycast", vol.raycast_pyramid(poses[N_KF - 1], K, W, H, LEVELS)),
                            ("map_render", kmap.render_pyramid(poses[N_KF - 1], K, W, H, LEVELS)),
                            ("keyframe", pyr[N_KF - 1])):
            err[name] = float(synth.pose_error(trk.match(model, pyr[N_KF]).Transformation, gt))
        view_stats = vol.raycast_pyramid(poses[N_KF - 1], K, W, H, LEVELS).raycast_stats
        points = vol.extract()[2]["points"]
        n_vox = n ** 3
        row = {"voxel": voxel, "trunc": trunc, "view": view_stats, "surface_points": points, "pose_error": err}
        bytes_of = {"insert_1": (32 + 8) * n_vox, "insert_8": (32 + 8 * N_KF) * n_vox, "move": (32 + 16) * n_vox,
                    "extract": 16 * n_vox + 16 * points}
        for name, s in samples.items():
            call, dev = [c for c, _ in s], [d for _, d in s]
            row[name] = {"call_ms": spread(call)}
            if name.startswith("map_"):
                continue
            row[name]["device_ms"] = spread(dev)
            if name in bytes_of:
                row[name]["bytes_upper_bound"] = bytes_of[name]
                row[name]["hbm_fraction_at_most"] = round(bytes_of[name] / (float(np.median(dev)) * 1e-3) / HBM_PEAK, 4)
        if n <= 256:  # the host path, once
            t0 = time.perf_counter()
            d = vol.download()
            t_down = (time.perf_counter() - t0) * 1e3
            rec = np.stack([d[f] for f in ("w_sum", "sd_sum", "iw_sum", "i_sum")], axis=-1).view(np.uint32)
            ropt = ref.Options(**opt)
            t0 = time.perf_counter()
            ref.integrate(ropt, rec, [(frames[0][1], frames[0][0], K, poses[0])], -1)
            t_int = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            ref.raycast(ropt, rec, poses[N_KF - 1], K, W, H, fill=0.0)
            t_ray = (time.perf_counter() - t0) * 1e3
            row["host_round_trip_ms_once"] = {"download": round(t_down, 1), "numpy_integrate_1": round(t_int, 1), "numpy_raycast": round(t_ray, 1)}
        result["sizes"][str(n)] = row
        print(json.dumps({str(n): row}))
        del vol, kmap
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
