"""Time of the pose-graph optimizer (dvo_amd_optimize_graph) per solver on synthetic graphs.

Graphs: "ring" = the ring-plus-chords graph of the dense tests with m free vertices; "slam" = the reference's dense final graph
(one vertex per frame, odometry + keyframe edges, keyframe-keyframe constraints and loop closures, tests/slam_graph.py) of F
frames (m = F - 1 free vertices).  Size specs: ring573, ring1024, slam3000, ... (a bare number means ring).

For every (size, solver) one line: ms of the first linearisation (linearise + assemble) and of the first factorization, both from
hipEvents inside the call; for the sparse solver also the host ms of its symbolic phase, the ms of the substitutions after the
first factorization, and the fronts / levels / widest front / factor MB of the symbolic phase; ms per iteration of a
10-iteration Levenberg-Marquardt call (host clock around the whole call / iterations); and a GFLOP/s figure: the dense path
counts n_padded^3 / 3, the sparse path the symbolic phase's flop count of its numeric factorization.  Medians over --reps
calls in one process after a warm-up call.  Every (size, solver) runs in a child process of its own under `timeout`.
Usage: python scripts/pose_graph_timing.py [--sizes ring573,ring1024,slam1000,slam3000,slam5000] [--solver dense,sparse]
       [--reps 5] [--timeout 600]
The dense solver takes at most 1024 free vertices: larger sizes are skipped for it."""
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


def make_graph(spec: str):
    import pose_graph_restatement as R
    import slam_graph

    kind = spec.rstrip("0123456789") or "ring"
    size = int(spec[len(kind):] if spec[0].isalpha() else spec)
    if kind == "ring":
        g, _ = R.ring_graph(size + 1, n_chords=max(4, size // 25), star=8, seed=size, noise=1e-3, drift=0.01)
    elif kind == "slam":
        g, _, _ = slam_graph.slam_graph(size, seed=size, noise=1e-3, drift=0.01)
    else:
        raise ValueError(spec)
    return g


def one_size(spec: str, solver: str, reps: int) -> dict:
    from dvo_slam_amd import capi, graph

    g = make_graph(spec)
    pg = graph.PoseGraph()
    for P, f in zip(g.poses, g.fixed):
        pg.add_vertex(P, fixed=f)
    for f, t, Z, O in g.edges:
        pg.add_edge(f, t, Z, O)
    trk = capi.DenseTracker()
    iters = 10
    pg.optimize(trk, "levenberg", iterations=iters, update=False, solver=solver)  # warm-up: code objects, workspace
    rows, per_it = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = pg.optimize(trk, "levenberg", iterations=iters, update=False, solver=solver)
        dt = (time.perf_counter() - t0) * 1e3
        if solver == "sparse":
            rows.append(graph.debug_sparse_timing(trk))
        else:
            a, b, n_pad, _ = graph.debug_timing(trk)
            rows.append({"linearise_ms": a, "factorize_ms": b, "n_padded": n_pad})
        per_it.append(dt / max(res.n_iterations, 1))
    n = 6 * res.n_free
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    out = dict(spec=spec, solver=solver, m=res.n_free, n=n, edges=len(g.edges), iteration_ms=float(np.median(per_it)),
               iterations=res.n_iterations, **med)
    flops = med["flops"] if solver == "sparse" else med["n_padded"] ** 3 / 3.0
    out["factorize_gflops"] = flops / (med["factorize_ms"] * 1e-3) / 1e9
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="ring573,ring1024,slam1000,slam3000,slam5000")
    ap.add_argument("--solver", default="dense,sparse")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        spec, solver = a.child.split(":")
        print(json.dumps(one_size(spec, solver, a.reps)))
        return
    rc = 0
    for spec in a.sizes.split(","):
        for solver in a.solver.split(","):
            if solver == "dense" and len(make_graph(spec).free) > 1024:
                continue
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child",
                   f"{spec}:{solver}", "--reps", str(a.reps)]
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode != 0:
                print(f"{spec} {solver}: exit {res.returncode}\n{res.stderr[-2000:]}")
                sys.exit(res.returncode)  # nothing more on the GPU after a failure
            r = json.loads(res.stdout.strip().splitlines()[-1])
            line = (f"{spec:>9s} {solver:6s} m={r['m']:5d} edges={r['edges']:5d}: linearise {r['linearise_ms']:.3f} ms, "
                    f"factorize {r['factorize_ms']:.3f} ms ({r['factorize_gflops']:.1f} GFLOP/s fp64), ")
            if solver == "sparse":
                line += (f"solve {r['solve_ms']:.3f} ms, symbolic {r['symbolic_ms']:.2f} ms (host), fronts {r['fronts']:.0f} / "
                         f"levels {r['levels']:.0f} / widest {r['widest']:.0f}, factor {r['factor_doubles'] * 8 / 1e6:.1f} MB, ")
            else:
                line += f"n_padded {r['n_padded']:.0f}, "
            line += f"iteration {r['iteration_ms']:.3f} ms (Levenberg, {r['iterations']} iterations)"
            print(line, flush=True)
            print("JSON " + json.dumps(r), flush=True)
    sys.exit(rc)


if __name__ == "__main__":
    main()
