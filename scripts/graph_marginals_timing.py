"""Time of the marginal covariances (dvo_amd_graph_marginals) against one factorization and against unit solves.

Per graph (the specs of scripts/pose_graph_timing.py: ring573, ring1024, slam1000, slam3000, slam5000) and solver, medians of
--reps calls with their ranges, host clock around the C call alone (the arrays are packed once, outside the clock):
  (a)  all_diagonals_ms      every vertex's diagonal block through the new path: the whole call (symbolic phase, linearise,
                             factorize, selected inversion, gather, copy back)
       stats_only_ms         the same call with n_blocks = 0 (everything but the gather and the copy back)
       first_system_ms       dvo_amd_debug_graph_system[_sparse] on the same graph: the same call without the selected inversion;
                             selected_inversion_ms = stats_only_ms - first_system_ms
  (b)  factorize_ms          one factorization of the same graph on the same build, from the hipEvents inside an optimize call
                             (dvo_amd_debug_graph_sparse_timing / _graph_timing)
  (c)  unit_solves_ms        the same diagonals the only way the kernels had before allow: 6 m unit solves through the existing
                             substitution.  Sparse solver only: measured on >= 64 block columns (requests between far-apart
                             vertices, which take the solve path: 6 solves per column) as the call's time over stats_only_ms, and
                             scaled by m / columns.
Every (spec, solver) runs in a child process of its own under `timeout`.
Usage: python scripts/graph_marginals_timing.py [--sizes ...] [--solver dense,sparse] [--reps 5] [--out profiles/graph_marginals.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def _summary(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def one_size(spec: str, solver: str, reps: int) -> dict:
    from pose_graph_timing import make_graph

    from dvo_slam_amd import capi, graph

    g = make_graph(spec)
    pg = graph.PoseGraph()
    for P, f in zip(g.poses, g.fixed):
        pg.add_vertex(P, fixed=f)
    for f, t, Z, O in g.edges:
        pg.add_edge(f, t, Z, O)
    trk = capi.DenseTracker()
    L = graph._lib()
    live, nv, ne, P, fixed, ce = pg._pack()
    o = graph.default_options("dogleg")
    o.solver = graph.SOLVERS[solver]
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    st = graph.CGraphMarginalStats()

    def call(pairs):
        pr = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        a, b = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        out = np.zeros(36 * max(len(pr), 1))
        ms = []
        for i in range(reps + 1):  # the first call warms up: code objects, workspace
            t0 = time.perf_counter()
            rc = L.dvo_amd_graph_marginals(trk._h, nv, P.ctypes.data_as(dp), fixed.ctypes.data_as(ip), ne, ce, C.byref(o),
                                           len(pr), a.ctypes.data_as(ip), b.ctypes.data_as(ip), out.ctypes.data_as(dp),
                                           C.byref(st))
            dt = (time.perf_counter() - t0) * 1e3
            capi._check(rc, "dvo_amd_graph_marginals")
            assert st.factorized == 1
            if i:
                ms.append(dt)
        return ms

    m = len(g.free)
    res = dict(spec=spec, solver=solver, m=m, n=6 * m, edges=len(g.edges), reps=reps)
    res["all_diagonals_ms"] = _summary(call([(v, v) for v in range(nv)]))
    assert st.solved_columns == 0
    res["stats_only_ms"] = _summary(call([]))
    probe = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        (pg.debug_system_sparse if solver == "sparse" else pg.debug_system)(trk, 5.0)
        if i:
            probe.append((time.perf_counter() - t0) * 1e3)
    res["first_system_ms_with_python_packing"] = _summary(probe)
    fac = []
    for i in range(reps + 1):
        pg.optimize(trk, "levenberg", iterations=1, update=False, solver=solver)
        if i:
            fac.append(graph.debug_sparse_timing(trk)["factorize_ms"] if solver == "sparse" else graph.debug_timing(trk)[1])
    res["factorize_ms"] = _summary(fac)
    if solver == "sparse":
        free = g.free
        step = max(1, (m // 2) // 64)
        far = [(free[i], free[i + m // 2]) for i in range(0, m // 2, step)][:64]
        ms = call(far)
        cols = st.solved_columns
        res["unit_solve_columns_measured"] = cols
        if cols:
            base = res["stats_only_ms"]["median"]
            res["unit_solves_ms"] = {k: (v - base) * m / cols for k, v in _summary(ms).items()}
            res["unit_solves_note"] = f"measured on {cols} block columns ({6 * cols} solves), scaled by m / {cols}"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="ring573,ring1024,slam1000,slam3000,slam5000")
    ap.add_argument("--solver", default="dense,sparse")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_marginals.json"))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        spec, solver = a.child.split(":")
        print(json.dumps(one_size(spec, solver, a.reps)))
        return
    from pose_graph_timing import make_graph

    rows = []
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
            rows.append(r)
            line = (f"{spec:>9s} {solver:6s} m={r['m']:5d}: all diagonals {r['all_diagonals_ms']['median']:.2f} ms "
                    f"[{r['all_diagonals_ms']['min']:.2f}, {r['all_diagonals_ms']['max']:.2f}], stats only "
                    f"{r['stats_only_ms']['median']:.2f} ms, factorize {r['factorize_ms']['median']:.3f} ms")
            if "unit_solves_ms" in r:
                u = r["unit_solves_ms"]
                line += f", 6m unit solves {u['median']:.0f} ms [{u['min']:.0f}, {u['max']:.0f}] ({r['unit_solves_note']})"
            print(line, flush=True)
    with open(a.out, "w") as f:
        json.dump({"what": "scripts/graph_marginals_timing.py", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
