"""What the place index costs at 640x480 with four levels (level 3: 80x60, dim 4800), next to what a user could do before it
existed, from one run:

  add_64_one_call / add_64_calls   dvo_amd_place_index_add of 64 pyramids in one call (one launch) and in 64 calls, into a new index
  host_describe_64                 the route it replaces: 64 level planes downloaded, the numpy descriptor (tests/place_ref.py)
  query_1xN (N = 1024, 4096)       dvo_amd_place_query of one row against the whole index, k = 5
  all_pairs_4096                   dvo_amd_place_query of every row against the whole index, k = 5
  host_query_1xN / host_all_pairs  an int32 numpy matmul over descriptors already on the host, the score and the order by lexsort;
                                   all pairs is timed on --host-rows query rows and scaled to N (said so in the report)

The index of N rows holds the 64 pyramids N / 64 times.  call_ms is the host clock around the synchronous call; device_ms is the
time between two events around the call's kernel launches (dvo_amd_debug_place_timing): dots_device_ms brackets k_place_dots alone
(through dvo_amd_place_scores), query_device_ms k_place_dots and k_place_topk.  Medians of --samples timed calls after a warm-up,
with [min, max].  fraction_of_hbm_peak: the N * dim bytes a 1 x N query must read over dots_device_ms over 8 TB/s -- the index of
a repeated query sits in the last-level cache, so this is a rate, not a statement about HBM traffic.  fraction_of_int8_peak:
2 * N * N * dim operations over dots_device_ms over 5e15 op/s (dense int8: twice the BF16 rate per clock).
--tile 1|2|4 fixes the workgroup tile of k_place_dots (DVO_AMD_PLACE_TILE) and --quick leaves out add and the host routes: the job
that compares tiles.  One process, one GPU.  Writes profiles/place_index.json (or --out).
Usage: python scripts/place_index_bench.py [--samples 7] [--host-rows 64] [--tile T] [--quick] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, LEVELS, LEVEL = 640, 480, 4, 3
BASE, SIZES, ALL_PAIRS, K = 64, (1024, 4096), 4096, 5
HBM_PEAK, INT8_PEAK = 8e12, 5e15  # bytes / s, op / s


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def clocked(fn, samples):
    fn()
    times = []
    for _ in range(samples):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--host-rows", type=int, default=64)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_index.json"))
    a = ap.parse_args()
    if a.tile:
        os.environ["DVO_AMD_PLACE_TILE"] = str(a.tile)  # (read once, when the first dot products are launched)

    import place_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("place_index_bench.py needs a HIP device (no CPU fallback)")
    Kc = synth.intrinsics_for(W, H)
    poses = [synth.se3_exp(t * synth.XI_STEP_STREAM) for t in range(BASE)]
    pyr = [capi.RgbdImagePyramid(*synth.raw_to_float(*synth.sensor_frame(W, H, poses[t], frame_id=t)), Kc, LEVELS) for t in range(BASE)]
    report = {"image": [W, H], "levels": LEVELS, "level": LEVEL, "k": K, "samples": a.samples, "tile": a.tile or "by the number of queries",
              "what": "call_ms: host clock around the synchronous call; *_device_ms: between two events around the call's kernel "
                      "launches; medians with [min, max]; one process"}

    def describe_host():
        return ref.describe([p.plane(LEVEL, 0) for p in pyr])

    X64, nn64 = describe_host()
    dim = X64.shape[1]
    report["dim"] = dim
    check = capi.PlaceIndex(level=LEVEL)
    check.add(pyr)
    rows, norms = check.descriptors()
    assert np.array_equal(rows, X64) and np.array_equal(norms, nn64)  # the two routes give the same descriptors

    if not a.quick:
        def one_call():
            capi.PlaceIndex(level=LEVEL).add(pyr)

        def many_calls():
            index = capi.PlaceIndex(level=LEVEL)
            for p in pyr:
                index.add([p])

        report["add"] = {"add_64_one_call_ms": spread(clocked(one_call, a.samples)), "add_64_calls_ms": spread(clocked(many_calls, a.samples)),
                         "host_describe_64_ms": spread(clocked(describe_host, 3), 2)}

    report["queries"] = {}
    capi.place_timing(True)
    try:
        for n in sorted(set(SIZES) | {ALL_PAIRS}):
            index = capi.PlaceIndex(level=LEVEL)
            for _ in range(n // BASE):
                index.add(pyr)
            X, nn = np.tile(X64, (n // BASE, 1)), np.tile(nn64, n // BASE)
            r = np.array([ref.inv_norm(v) for v in nn])
            got = index.query([n - 1], k=K)
            assert np.array_equal(got[0], ref.query(X, nn, [n - 1], K)[0])
            shapes = [("query_1xN", [n - 1])] + ([("all_pairs", list(range(n)))] if n == ALL_PAIRS else [])
            for name, ids in shapes:
                dots_ms, query_ms, call_ms = [], [], []
                index.scores(ids), index.query(ids, k=K)  # warm-up: code objects loaded, scratch grown
                for _ in range(a.samples):
                    index.scores(ids)
                    dots_ms.append(capi.place_timing(True))
                    t0 = time.perf_counter()
                    index.query(ids, k=K)
                    call_ms.append((time.perf_counter() - t0) * 1e3)
                    query_ms.append(capi.place_timing(True))
                entry = {"n": n, "n_queries": len(ids), "dots_device_ms": spread(dots_ms), "query_device_ms": spread(query_ms),
                         "call_ms": spread(call_ms)}
                d = entry["dots_device_ms"]["median"] * 1e-3
                if len(ids) == 1:
                    entry["bytes_read"] = n * dim
                    entry["fraction_of_hbm_peak"] = round(n * dim / d / HBM_PEAK, 4)
                else:
                    entry["operations"] = 2 * n * n * dim
                    entry["fraction_of_int8_peak"] = round(2 * n * n * dim / d / INT8_PEAK, 4)
                if not a.quick:
                    X32 = X.astype(np.int32)
                    rows_timed = min(len(ids), a.host_rows)

                    def host_query():
                        D = X32[ids[:rows_timed]] @ X32.T
                        return [ref.query_row(D[i], r[q], r, q, K) for i, q in enumerate(ids[:rows_timed])]

                    host = spread(clocked(host_query, 3), 2)
                    scale = len(ids) / rows_timed
                    entry["host_ms"] = {k: round(v * scale, 2) for k, v in host.items()}
                    entry["host_rows_timed"] = rows_timed  # (fewer than n_queries: host_ms is the timed rows' time scaled up)
                    entry["host_over_call"] = round(entry["host_ms"]["median"] / entry["call_ms"]["median"], 1)
                report["queries"][f"{name}_{n}"] = entry
            del index
    finally:
        capi.place_timing(False)
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
