"""What scoring pose hypotheses costs on the 640x480, four-level workload of bench.py (keyframe 0 and the first current frame of the
synthetic workload, hypotheses on a grid around the pose a match returned, the precisions of that match), two routes, from one run:

  score_poses   dvo_amd_score_poses for 512 and 4096 hypotheses at level 3 and at level 2, and dvo_amd_score_poses_many over 8 pairs
                x 4096 hypotheses at level 3 (the same pair 8 times): two launches and one synchronisation per call, whatever m is
  per_call      what the call replaces, on the same build: one dvo_amd_mask_from_residuals call per hypothesis (all levels, with
                counts).  64 of them are timed and the time is SCALED to m (x m / 64): thousands of launches are not waited for

call_ms is the host clock around the synchronous call(s).  Medians of --samples after a warm-up, with [min, max].  The two routes
are compared for equality before anything is timed: the records of the first 64 hypotheses equal the restatement
(tests/pose_score_ref.py) fed with dvo_amd_mask_from_residuals' planes at each of them, at both levels.

Recorded next to the timings, asserted nowhere: a synthetic pair whose true motion is a yaw of 15 degrees and 20 cm along x --
where dvo_amd_match from the identity ends and where it ends from the top-ranked hypothesis of a grid of +-20 degrees in steps of
5 and +-30 cm in steps of 10 scored at level 3, both as pose error against the ground truth.  That motion is a point of the grid,
so a second pair (13 degrees, 17 cm) that lies between the grid's points is recorded the same way.
One process, one GPU.  Writes profiles/pose_scoring.json.
Usage: python scripts/pose_scoring_bench.py [--samples 9] [--out PATH]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, LEVELS = 640, 480, 4
PAIRS, TIMED_CALLS = 8, 64


def spread(xs, digits=4):
    xs = np.asarray(xs, dtype=np.float64)
    return {"median": round(float(np.median(xs)), digits), "min": round(float(xs.min()), digits), "max": round(float(xs.max()), digits)}


def outcome_of(ref, evaluated, plane, distance):
    """the outcome plane from a mask made with invalid_keep = 1 and its distances (tests/test_pose_scoring.py)"""
    outcome = np.full(evaluated.shape, ref.UNEVALUATED, np.int8)
    outcome[evaluated] = ref.OUTLIER
    outcome[evaluated & (plane == 1)] = ref.INLIER
    outcome[evaluated & (plane == 1) & np.isnan(distance)] = ref.INVALID
    return outcome


def lost_pair(capi, synth, yaw_degrees, shift):
    """a pair the tracker is lost on: pose error of a match from the identity and of one from the top-ranked hypothesis"""
    K = synth.intrinsics_for(W, H)
    xi = np.array([shift, 0.0, 0.0, 0.0, np.deg2rad(yaw_degrees), 0.0])
    (Ir, Zr), (Ic, Zc), T_gt = synth.make_pair(W, H, xi_gt=xi)
    reference, current = capi.RgbdImagePyramid(Ir, Zr, K, LEVELS), capi.RgbdImagePyramid(Ic, Zc, K, LEVELS)
    plain = capi.DenseTracker(capi.Config()).match(reference, current)
    grid = capi.pose_grid(np.eye(4), vx=(7, 0.1), wy=(9, np.deg2rad(5.0)))
    options = capi.pose_score_options(LEVELS - 1, result=plain)  # the only precision a lost tracker has: the failed alignment's
    seeded_tracker = capi.DenseTracker(capi.Config(UseInitialEstimate=True))
    scores = seeded_tracker.score_poses(reference, current, grid, options)
    order = capi.rank_poses(scores, 3)
    seeded = seeded_tracker.match(reference, current, T_init=grid[order[0]])
    truth = np.linalg.inv(T_gt)  # reference -> current
    return {"true_motion": f"yaw {yaw_degrees} degrees, {shift} m along x", "hypotheses": len(grid), "level": LEVELS - 1,
            "top3": [int(j) for j in order], "top3_total": [int(scores["total"][j]) for j in order],
            "top_hypothesis_error": float(synth.pose_error(truth, grid[order[0]])),
            "identity_error": float(synth.pose_error(truth, np.eye(4))),
            "match_from_identity_error": None if plain.isNaN() else float(synth.pose_error(T_gt, plain.Transformation)),
            "match_from_identity_is_nan": bool(plain.isNaN()),
            "match_from_top_hypothesis_error": None if seeded.isNaN() else float(synth.pose_error(T_gt, seeded.Transformation)),
            "match_from_top_hypothesis_is_nan": bool(seeded.isNaN())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_scoring.json"))
    a = ap.parse_args()

    import bench
    import pose_score_ref as ps
    import residual_mask_ref as ref
    from dvo_slam_amd import capi, synth

    if capi.lib().dvo_amd_device_count() < 1:
        raise SystemExit("pose_scoring_bench.py needs a HIP device (no CPU fallback)")
    K = synth.intrinsics_for(W, H)
    f0, f1 = bench.workload_ref_frame(synth, W, H, 0, 0), bench.workload_cur_frame(synth, W, H, 0, 0)
    kf, cur = capi.RgbdImagePyramid(f0[0], f0[1], K, LEVELS), capi.RgbdImagePyramid(f1[0], f1[1], K, LEVELS)
    trk = capi.DenseTracker(capi.Config(FirstLevel=LEVELS - 1, LastLevel=0))
    result = trk.match(kf, cur)
    estimate = capi.rigid_inverse(result.Transformation)
    # 17^3 = 4913 hypotheses around the estimate (1 cm along x, half a degree about y and z); the first 4096 / 512 are used
    grid = capi.pose_grid(estimate, vx=(17, 0.01), wy=(17, np.deg2rad(0.5)), wz=(17, np.deg2rad(0.5)))
    ropt = capi.residual_mask_options(result, LEVELS, invalid_keep=1)
    sopt = {l: capi.pose_score_options(l, precision=list(ropt.precision[l])) for l in (2, 3)}

    # ---- the two routes agree
    for l in (2, 3):
        evaluated = ref.evaluated_ref(*(kf.plane(l, k) for k in (1, 4, 5)))
        got = ps.as_ints(trk.score_poses(kf, cur, grid[:TIMED_CALLS], sopt[l]))
        for j in range(TIMED_CALLS):
            mask, counts, distance = capi.SelectionMask.from_residuals(trk, kf, cur, T=grid[j], options=ropt, counts=True, distance=True)
            want = ps.score_ref(outcome_of(ref, evaluated, mask.download(l), distance[l]), distance[l])
            assert got[j] == want, (l, j, got[j], want)
            assert all(got[j][k] == int(counts[l][k]) for k in ("evaluated", "invalid", "inlier", "outlier"))

    def score(m, l):
        return lambda: trk.score_poses(kf, cur, grid[:m], sopt[l])

    def many():
        return trk.score_poses_many([kf] * PAIRS, [cur] * PAIRS, [grid[:4096]] * PAIRS, [sopt[3]] * PAIRS)

    def per_call():
        for j in range(TIMED_CALLS):
            capi.SelectionMask.from_residuals(trk, kf, cur, T=grid[j], options=ropt, counts=True)

    routes = {"score_512_level3": score(512, 3), "score_4096_level3": score(4096, 3), "score_512_level2": score(512, 2),
              "score_4096_level2": score(4096, 2), "score_many_8x4096_level3": many, "from_residuals_64_calls": per_call}
    ms = {k: [] for k in routes}
    for fn in routes.values():  # warm-up: code objects loaded, pools and areas grown
        fn()
        fn()
    for _ in range(a.samples):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    report = {"image": [W, H], "levels": LEVELS, "samples": a.samples, "pixels": {l: (W >> l) * (H >> l) for l in (2, 3)},
              "tile": capi.POSE_SCORE_TILE,
              "what": "call_ms: host clock around the synchronous call(s); routes interleaved; one process; the per-call route is "
                      "64 dvo_amd_mask_from_residuals calls, SCALED by m / 64 in per_call_scaled_ms",
              "call_ms": {k: spread(v) for k, v in ms.items()}}
    c = report["call_ms"]
    one = c["from_residuals_64_calls"]["median"] / TIMED_CALLS
    report["per_call_ms_each"] = round(one, 4)
    report["per_call_scaled_ms"] = {"m_512": round(512 * one, 2), "m_4096": round(4096 * one, 2), "8x4096": round(PAIRS * 4096 * one, 2)}
    report["ratios"] = {
        "per_call_over_score_512_level3": round(512 * one / c["score_512_level3"]["median"], 1),
        "per_call_over_score_4096_level3": round(4096 * one / c["score_4096_level3"]["median"], 1),
        "per_call_over_score_4096_level2": round(4096 * one / c["score_4096_level2"]["median"], 1),
        "per_call_over_score_many": round(PAIRS * 4096 * one / c["score_many_8x4096_level3"]["median"], 1),
        "us_per_hypothesis_level3": round(1e3 * c["score_4096_level3"]["median"] / 4096, 3),
        "us_per_hypothesis_level2": round(1e3 * c["score_4096_level2"]["median"] / 4096, 3),
        "us_per_hypothesis_many": round(1e3 * c["score_many_8x4096_level3"]["median"] / (PAIRS * 4096), 3),
    }
    # (15 degrees, 0.2 m) is a point of the grid -- the inverse of exp(xi) is exp(-xi); (13 degrees, 0.17 m) lies between its points
    report["lost_pair"] = lost_pair(capi, synth, 15.0, 0.2)
    report["lost_pair_off_grid"] = lost_pair(capi, synth, 13.0, 0.17)
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
