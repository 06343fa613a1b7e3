"""Many small pose graphs: N sequential dvo_amd_optimize_graph calls (dense, the only way before the batch entry) against one
dvo_amd_optimize_graphs_batch call over the same N local maps (tests/test_pose_graph_batch.py::local_maps: a fixed keyframe,
15 frames, odometry + keyframe edges, noise and drift), Levenberg, 50 iterations.

Wall clock around the whole C calls (upload, kernels, download; the ctypes arrays are packed before the clock starts and the
poses are reset before every repetition), after one warm-up call of each kind per N.  Reports per N: ms per call set, graphs/s,
the ratio baseline / batch, the iterations run per graph; medians of --reps repetitions with min and max.
Usage: python scripts/graph_batch_timing.py [--reps 7] [--sizes 1,8,64,512] [--out profiles/graph_batch.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dvo_slam_amd import capi, graph  # noqa: E402
from test_pose_graph_batch import _items, local_maps  # noqa: E402


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="1,8,64,512")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_batch.json"))
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    k = 15
    maps = local_maps(n_frames=k * max(sizes) + 1, k=k)[:max(sizes)]
    assert len(maps) == max(sizes)
    L = graph._lib()
    trk = capi.DenseTracker()
    opt = graph.default_options("levenberg")
    opt.max_iterations = 50
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rows = []
    for n in sizes:
        items, keep = _items(maps[:n])
        pristine = [kp[0].copy() for kp in keep]
        st = graph.CGraphStats()

        def reset():
            for kp, P in zip(keep, pristine):
                kp[0][...] = P

        def single():
            its = []
            t0 = time.perf_counter()
            for i in range(n):
                P, fixed, ce, chi2, weight = keep[i]
                rc = L.dvo_amd_optimize_graph(trk._h, items[i].n_vertices, P.ctypes.data_as(dp), fixed.ctypes.data_as(ip),
                                              items[i].n_edges, ce, C.byref(opt), chi2.ctypes.data_as(dp),
                                              weight.ctypes.data_as(dp), 0, None, C.byref(st))
                assert rc == 0, rc
                its.append(st.iterations)
            return (time.perf_counter() - t0) * 1e3, its

        def batch():
            t0 = time.perf_counter()
            rc = L.dvo_amd_optimize_graphs_batch(trk._h, n, items, C.byref(opt))
            ms = (time.perf_counter() - t0) * 1e3
            assert rc == 0, rc
            return ms, [items[i].stats.iterations for i in range(n)]

        t_single, t_batch = [], []
        for rep in range(a.reps + 1):  # the first of each kind is the warm-up (the workspaces grow there)
            reset()
            ms, its_single = single()
            if rep:
                t_single.append(ms)
            reset()
            ms, its_batch = batch()
            if rep:
                t_batch.append(ms)
        s, b = stats(t_single), stats(t_batch)
        row = {"graphs": n, "free_vertices": int(items[0].stats.n_free), "edges": int(items[0].n_edges), "reps": a.reps,
               "sequential_single_calls": dict(s, graphs_per_s=n / s["median_ms"] * 1e3,
                                               iterations_mean=float(np.mean(its_single))),
               "one_batch_call": dict(b, graphs_per_s=n / b["median_ms"] * 1e3, iterations_mean=float(np.mean(its_batch))),
               "ratio_single_over_batch": s["median_ms"] / b["median_ms"],
               "ranges_overlap": bool(s["min_ms"] <= b["max_ms"])}
        rows.append(row)
        print(f"N={n:4d}: sequential {s['median_ms']:9.2f} ms [{s['min_ms']:.2f}, {s['max_ms']:.2f}]  batch "
              f"{b['median_ms']:8.2f} ms [{b['min_ms']:.2f}, {b['max_ms']:.2f}]  ratio {row['ratio_single_over_batch']:.1f}  "
              f"iterations/graph {np.mean(its_single):.1f} vs {np.mean(its_batch):.1f}", flush=True)
    out = {"what": "N local maps (15 free vertices, 29 edges), Levenberg, 50 iterations max: N sequential "
                   "dvo_amd_optimize_graph (dense) calls vs one dvo_amd_optimize_graphs_batch call; wall clock of the C calls",
           "device": trk.device_name() if hasattr(trk, "device_name") else "gfx950", "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
