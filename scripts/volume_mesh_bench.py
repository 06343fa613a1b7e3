"""What the volume's mesh costs: eight 640x480 sensor keyframes of the synthetic stream fused into a 256^3 volume over the room, the
surface pulled as an indexed triangle mesh (dvo_amd_volume_mesh), and next to it, from the same run,

  extract            dvo_amd_volume_extract on the same volume: the same crossings as a bag of points
  host round trip    timed once: the records downloaded, and tests/volume_mesh_ref.py's vectorised numpy restatement on a sub-box
                     of 64 z-layers around the layer of the median vertex, scaled by voxels to the whole volume (the scaled
                     figure is an estimate: the surface is not spread evenly over the layers; the sub-box's vertices are reported)

  device_ms   between two events on the library's internal stream around the call's own launches (dvo_amd_debug_volume_timing)
  call_ms     host clock around the synchronous call, the copies of the results to the host included

Medians of --samples timed calls after a warm-up, the two interleaved call by call, with [min, max].  Both are timed with their
capacity known: one call of the entry.  bytes: what the mesh must move at least -- plane a once per pass over the cells and twice
per pass over the voxels (8 B/voxel, three passes of the five), 28 B per vertex with its normal, 12 B per triangle -- and the
fraction of the HBM peak (8.0 TB/s) that device_ms implies.  One process, one GPU.  Writes profiles/volume_mesh.json.
Usage: python scripts/volume_mesh_bench.py [--samples 7] [--size 256] [--out PATH]"""
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
SUB_LAYERS = 64


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_mesh.json"))
    a = ap.parse_args()

    import volume_mesh_ref as mref
    import volume_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("volume_mesh_bench.py needs a HIP device (no CPU fallback)")
    K = tuple(float(k) for k in synth.intrinsics_for(W, H))
    poses = [synth.se3_exp(4 * synth.XI_STEP_STREAM * t) for t in range(N_KF)]
    pyr = []
    for t, T in enumerate(poses):
        grey, raw_z = synth.sensor_frame(W, H, T, frame_id=t)
        I, Z = synth.raw_to_float(grey, raw_z)
        pyr.append(capi.RgbdImagePyramid(I, Z, K, LEVELS))
    n = a.size
    voxel = EXTENT / n
    opt = dict(nx=n, ny=n, nz=n, voxel=voxel, origin=ORIGIN, trunc=max(3.0 * voxel, 0.03), near_z=0.4, far_z=5.0,
               weight=capi.VOLUME_WEIGHT_SENSOR)
    vol = capi.SurfaceVolume(opt)
    vol.integrate(pyr, poses)
    capi.volume_timing(True)
    xyz, rgb, normals, tri, counts = vol.mesh()
    points = vol.extract()[2]["points"]
    assert counts["triangles"] // 2 + counts["open_edges"] == points

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3, capi.volume_timing(True)["ms"]

    variants = {"mesh": lambda: vol.mesh(capacity=(counts["vertices"], counts["triangles"])),
                "mesh_without_normals": lambda: vol.mesh(normals=False, capacity=(counts["vertices"], counts["triangles"])),
                "extract": lambda: vol.extract(capacity=points)}
    samples = {k: [] for k in variants}
    for rep in range(a.samples + 1):  # (the first round is the warm-up)
        for name, fn in variants.items():
            s = timed(fn)
            if rep:
                samples[name].append(s)
    n_vox = n ** 3
    bytes_of = {"mesh": 3 * 8 * n_vox + 28 * counts["vertices"] + 12 * counts["triangles"],
                "mesh_without_normals": 3 * 8 * n_vox + 16 * counts["vertices"] + 12 * counts["triangles"],
                "extract": 16 * n_vox + 16 * points}
    result = {"build_id": capi.build_id(), "width": W, "height": H, "keyframes": N_KF, "samples": a.samples, "size": n, "voxel": voxel,
              "counts": counts, "extract_points": points}
    for name, s in samples.items():
        call, dev = [c for c, _ in s], [d for _, d in s]
        result[name] = {"call_ms": spread(call), "device_ms": spread(dev), "bytes_at_least": bytes_of[name],
                        "hbm_fraction": round(bytes_of[name] / (float(np.median(dev)) * 1e-3) / HBM_PEAK, 4)}
    # the host path, once: all records down, the numpy restatement on a sub-box, scaled
    t0 = time.perf_counter()
    d = vol.download()
    t_down = (time.perf_counter() - t0) * 1e3
    layers = min(SUB_LAYERS, n)
    # ... around the layer that holds the median vertex, so that the sub-box has a surface to mesh
    mid = int(np.median((xyz[:, 2].astype(np.float64) - ORIGIN[2]) / voxel)) if len(xyz) else n // 2
    z0 = int(np.clip(mid - layers // 2, 0, n - layers))
    rec = np.ascontiguousarray(np.stack([d[f][z0:z0 + layers] for f in ("w_sum", "sd_sum", "iw_sum", "i_sum")], axis=-1)).view(np.uint32)
    sub = dict(opt, nz=layers, origin=(ORIGIN[0], ORIGIN[1], ORIGIN[2] + z0 * voxel))
    t0 = time.perf_counter()
    sub_counts = mref.mesh(ref.Options(**sub), rec)[4]
    t_sub = (time.perf_counter() - t0) * 1e3
    result["host_round_trip_ms_once"] = {"download": round(t_down, 1), "numpy_mesh_sub_box": round(t_sub, 1), "sub_box_layers": layers,
                                         "sub_box_vertices": sub_counts["vertices"],
                                         "numpy_mesh_scaled_to_the_volume": round(t_sub * n / layers, 1)}
    print(json.dumps(result))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
