"""What a point budget costs and buys on the 640x480, four-level workload of bench.py (keyframe 0 against the first current
frames of the synthetic workload, default thresholds, default tracker configuration).  For the full selection and for a few
budget masks -- TOPK at 1/2, 1/4, 1/8 of level 0's candidates (capi.level_budgets), GRID with cells of 2 and 4 -- side by side
from one run:

  create_ms      host clock around dvo_amd_mask_create_budget (the call ends in its one synchronisation), median of --samples
                 calls, the variants interleaved call by call; for GRID also with cells of 8, 9, 16, 64 and 640 (create only)
  match_ms       host clock around a single match() behind the mask with the selection already cached (the second and later
                 matches of a keyframe), median over --samples calls cycling through the current frames, variants interleaved
  pairs_per_s    dvo_amd_match_many_masked over --batch pairs of the keyframe with the current frames, every pair behind the
                 mask; median of --rounds timed rounds after two warm-up rounds, variants interleaved round by round
  pose_error     synth.pose_error against the synthetic ground truth of the batch's distinct pairs: mean and maximum; next to
                 it the residual passes a match took, averaged over those pairs

Nothing here is a kernel time: every figure includes launch overhead and the host side of the call, which is what a caller
pays.  One process, one GPU; other work may share the host, so the spread (min .. max) is reported next to every median.
Writes profiles/budget_selection.json.
Usage: python scripts/budget_selection_bench.py [--samples 100] [--batch 1152] [--rounds 7] [--frames 16] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, LEVELS = 640, 480, 4


def spread(xs, scale=1.0, digits=4):
    xs = np.asarray(xs, dtype=np.float64) * scale
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--batch", type=int, default=1152)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "budget_selection.json"))
    a = ap.parse_args()

    import bench
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("budget_selection_bench.py needs a HIP device (no CPU fallback)")
    K = synth.intrinsics_for(W, H)
    ref_frame = bench.workload_ref_frame(synth, W, H, 0, 0)
    cur_frames = [bench.workload_cur_frame(synth, W, H, 0, i) for i in range(a.frames)]
    truth = [bench.workload_cur_pose(synth, i) for i in range(a.frames)]
    ref = capi.RgbdImagePyramid(ref_frame[0], ref_frame[1], K, LEVELS)
    curs = [capi.RgbdImagePyramid(f[0], f[1], K, LEVELS) for f in cur_frames]
    cfg = capi.Config(FirstLevel=LEVELS - 1, LastLevel=0)
    thresholds = (cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold)
    trk = capi.DenseTracker(cfg)

    candidates = capi.SelectionMask.from_budget(ref, capi.BUDGET_TOPK, thresholds=thresholds).info()["kept"]
    makers = {"full": None}
    for name, part in (("topk_1/2", 2), ("topk_1/4", 4), ("topk_1/8", 8)):
        budgets = capi.level_budgets(candidates[0] // part, LEVELS)
        makers[name] = lambda b=budgets: capi.SelectionMask.from_budget(ref, capi.BUDGET_TOPK, budget=b, thresholds=thresholds)
    for name, cell in (("grid_2", 2), ("grid_4", 4)):
        makers[name] = lambda c=cell: capi.SelectionMask.from_budget(ref, capi.BUDGET_GRID, cell=c, thresholds=thresholds)
    variants = list(makers)
    masks = {v: (makers[v]() if makers[v] else None) for v in variants}

    # ---- the time of the create call; GRID's also where its kernel changes form (a lane per cell up to 8, a block per cell
    # above) and for large cells, up to one cell per level -- masks nobody tracks behind here
    for cell in (8, 9, 16, 64, 640):
        makers[f"grid_{cell}_create_only"] = lambda c=cell: capi.SelectionMask.from_budget(ref, capi.BUDGET_GRID, cell=c, thresholds=thresholds)
    create = {v: [] for v in makers if makers[v]}
    for v in create:  # warm-up: code objects loaded
        makers[v]()
    for _ in range(a.samples):
        for v in create:
            t0 = time.perf_counter()
            m = makers[v]()
            create[v].append(time.perf_counter() - t0)
            del m

    # ---- a single match() behind the mask, selection cached
    single = {v: [] for v in variants}
    for v in variants:  # warm-up: builds the keyframe's selection behind the mask
        for c in curs[:2]:
            trk.match(ref, c, mask=masks[v])
    for s in range(a.samples):
        c = curs[s % len(curs)]
        for v in variants:
            t0 = time.perf_counter()
            trk.match(ref, c, mask=masks[v])
            single[v].append(time.perf_counter() - t0)

    # ---- match_many_masked throughput and the pose error of its results
    B = a.batch
    refs, curb = [ref] * B, [curs[i % len(curs)] for i in range(B)]
    many, errors, passes, valid_points = {v: [] for v in variants}, {}, {}, {}
    for r in range(2 + a.rounds):
        for v in variants:
            ms = None if masks[v] is None else [masks[v]] * B
            t0 = time.perf_counter()
            raw = trk.match_batch(refs, curb, stats=False, masks=ms, raw=True)  # (raw: no per-pair Python objects in the window)
            dt = time.perf_counter() - t0
            if r >= 2:
                many[v].append(B / dt)
            if r == 0:
                out = [capi.Result(raw[i], None) for i in range(min(B, len(curs)))]
                assert not any(o.isNaN() for o in out), v
                errors[v] = [synth.pose_error(truth[i], o.Transformation) for i, o in enumerate(out)]
                passes[v] = float(np.mean([o.n_residual_passes for o in out]))
    for v in variants:
        valid_points[v] = [ref.select(l, thresholds[0], thresholds[1], mask=masks[v])[0] for l in range(LEVELS)]

    report = {"image": [W, H], "levels": LEVELS, "selection_thresholds": list(thresholds), "samples": a.samples, "batch": B,
              "rounds": a.rounds, "current_frames": a.frames,
              "what": "host-clock figures around synchronous calls, one process; see the script's docstring for each column",
              "candidates_per_level": candidates, "variants": {}}
    for v in variants:
        report["variants"][v] = {
            "selected_per_level": valid_points[v],
            "create_ms": spread(create[v], 1e3) if v in create else None,
            "match_ms": spread(single[v], 1e3),
            "pairs_per_s": spread(many[v], 1.0, 1),
            "pose_error": {"mean": float(np.mean(errors[v])), "max": float(np.max(errors[v]))},
            "residual_passes_per_match": round(passes[v], 2),
        }
    report["create_only_ms"] = {v[:-len("_create_only")]: spread(create[v], 1e3) for v in create if v.endswith("_create_only")}
    full = report["variants"]["full"]
    for v in variants:
        e = report["variants"][v]
        e["match_ms_over_full"] = round(e["match_ms"]["median"] / full["match_ms"]["median"], 4)
        e["pairs_per_s_over_full"] = round(e["pairs_per_s"]["median"] / full["pairs_per_s"]["median"], 4)
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
