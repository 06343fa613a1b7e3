"""Time of the pose-graph optimizer (dvo_amd_optimize_graph) on synthetic ring-plus-chords graphs of m = 100, 573 and 1024 free
vertices (n = 6m unknowns).

For every size one line: ms of a linearisation (linearise + assemble) and of a factorization (damped copy + blocked Cholesky),
both from hipEvents inside the call (dvo_amd_debug_graph_timing), ms per iteration of a 10-iteration Levenberg-Marquardt call
(host clock around the whole call / iterations), and the fp64 rate of the factorization counted as n^3 / 3 flops.  Medians over
--reps calls in one process.  Every size runs in a child process of its own under `timeout`.
Usage: python scripts/pose_graph_timing.py [--sizes 100,573,1024] [--reps 5] [--timeout 600]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def one_size(m: int, reps: int) -> dict:
    from dvo_slam_amd import capi, graph
    import pose_graph_restatement as R

    g, _ = R.ring_graph(m + 1, n_chords=max(4, m // 25), star=8, seed=m, noise=1e-3, drift=0.01)
    pg = graph.PoseGraph()
    for P, f in zip(g.poses, g.fixed):
        pg.add_vertex(P, fixed=f)
    for f, t, Z, O in g.edges:
        pg.add_edge(f, t, Z, O)
    trk = capi.DenseTracker()
    iters = 10
    pg.optimize(trk, "levenberg", iterations=iters, update=False)  # warm-up: code objects, workspace
    lin, fac, per_it = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = pg.optimize(trk, "levenberg", iterations=iters, update=False)
        dt = (time.perf_counter() - t0) * 1e3
        a, b, n_pad, _ = graph.debug_timing(trk)
        lin.append(a)
        fac.append(b)
        per_it.append(dt / max(res.n_iterations, 1))
    n = 6 * res.n_free
    fac_ms = float(np.median(fac))
    return dict(m=res.n_free, n=n, n_padded=n_pad, edges=len(g.edges), linearise_ms=float(np.median(lin)), factorize_ms=fac_ms,
                iteration_ms=float(np.median(per_it)), iterations=res.n_iterations,
                factorize_gflops=(n_pad ** 3 / 3.0) / (fac_ms * 1e-3) / 1e9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,573,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(one_size(a.child, a.reps)))
        return
    rc = 0
    for m in [int(s) for s in a.sizes.split(",")]:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", str(m),
               "--reps", str(a.reps)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            print(f"m={m}: exit {res.returncode}\n{res.stderr[-2000:]}")
            rc = res.returncode
            break  # nothing more on the GPU after a failure
        r = json.loads(res.stdout.strip().splitlines()[-1])
        print(f"m={r['m']:5d} n={r['n']:5d} (padded {r['n_padded']}) edges={r['edges']:5d}: linearise {r['linearise_ms']:.3f} ms, "
              f"factorize {r['factorize_ms']:.3f} ms ({r['factorize_gflops']:.1f} GFLOP/s fp64, n_padded^3/3), "
              f"iteration {r['iteration_ms']:.3f} ms (Levenberg, {r['iterations']} iterations)")
    sys.exit(rc)


if __name__ == "__main__":
    main()
