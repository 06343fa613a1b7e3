"""Cost of scoring a loop-closure candidate by view overlap (dvo_amd_covisibility) next to the cost of the alignments a pruned
candidate saves (stage 1 of the validator: four level-3 alignments per candidate), and what pruning does on one scenario.

Keyframes: 640x480 frames of the synthetic room along a slow sweep, N = 50 and 200.  For every N, in one process after a warm-up
cycle, medians of 7 with [min, max]:
  covisibility   all N*N ordered pairs in one call, at level 3 and at level 1: device time (hipEvents around k_covis inside the
                 call, dvo_amd_debug_covisibility_ms) and whole-call time, and both per pair
  stage 1        the validator's first stage (level 3, identity and relative-pose proposals with their cross-validation
                 inverses) for keyframe 0 against up to --stage1-candidates of the same keyframes: whole-call time per proposal
                 and per candidate
Pruning: synth.loop_closure_scenario in the sensor regime with its decoys and four keyframes that stand within the radius but look
elsewhere; for several min_overlap the candidates and stage-1 alignments it removes, and whether a constraint that survives the
two-stage validation without pruning is lost with it.
No bar is stated and no min_overlap is recommended here.  Writes profiles/covisibility.json.
Usage: python scripts/covisibility_timing.py [--sizes 50 200] [--reps 7] [--out profiles/covisibility.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dvo_slam_amd import capi, synth  # noqa: E402
from dvo_slam_amd import constraints as Cn  # noqa: E402

W, H, LEVELS = 640, 480, 4


def pose(k):
    return synth.se3_exp(np.array([0.02, -0.01, 0.015, 0.01, -0.02, 0.005]) * 0.5 * k)


def summary(v):
    return [round(float(np.median(v)), 5), round(float(np.min(v)), 5), round(float(np.max(v)), 5)]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def covisibility_rows(trk, kfs, reps):
    n = len(kfs)
    pairs = [(a, b) for a in range(n) for b in range(n)]
    rows = {}
    for level in (3, 1):
        dev, call = [], []
        for rep in range(reps + 1):  # cycle 0 warms the buffers up
            counts, ms = timed(lambda: capi.covisibility(trk, kfs, pairs, level=level))
            if rep > 0:
                call.append(ms), dev.append(capi.covisibility_ms(trk))
        over = capi.covisibility_overlap(counts)
        rows[f"level_{level}"] = {"pairs": len(pairs), "device_ms": summary(dev), "call_ms": summary(call),
                                  "device_us_per_pair": summary(np.array(dev) * 1e3 / len(pairs)),
                                  "call_us_per_pair": summary(np.array(call) * 1e3 / len(pairs)),
                                  "mean_overlap": round(float(over.mean()), 4)}
        print(f"  N = {n} level {level}: device {rows[f'level_{level}']['device_ms']} call {rows[f'level_{level}']['call_ms']} ms")
    return rows


def stage1_row(trk, kfs, n_candidates, reps):
    cands = kfs[1:1 + n_candidates]
    ms = []
    survivors = 0
    for rep in range(reps + 1):
        val = Cn.createConstraintProposalValidator(tracker=trk, min_constraint_ratio=0.0, ratio_coarse=-1e300, ratio_fine=-1e300)
        val.stages = val.stages[:1]  # no ratio rejects anything: the survivors show that every proposal was aligned
        props = Cn.proposalsForCandidates(kfs[0], cands)
        n_props = len(props)
        val.validate(props)
        survivors = len(props)
        if rep > 0:
            ms.append(val.native_ms)
    row = {"candidates": len(cands), "proposals": n_props, "alignments": 2 * n_props, "survivors": survivors, "call_ms": summary(ms),
           "ms_per_proposal": summary(np.array(ms) / n_props), "ms_per_candidate": summary(np.array(ms) / len(cands))}
    print(f"  stage 1: {row['candidates']} candidates, {row['call_ms']} ms, {row['ms_per_candidate']} ms per candidate")
    return row


def mid_gap(values):
    """a threshold in the middle of the widest gap of the observed values"""
    v = np.sort(np.asarray([x for x in values if np.isfinite(x)], dtype=np.float64))
    k = int(np.argmax(np.diff(v)))
    return float(0.5 * (v[k] + v[k + 1]))


def scenario(trk, n_candidates, overlaps):
    """synth.loop_closure_scenario in the sensor regime with its three decoys, plus four keyframes that stand within the radius
    but see little or nothing of the query keyframe's surfaces: turned by 90, 135 and 180 degrees about y, and 0.9 m to the side"""
    K = synth.intrinsics_for(W, H)
    key, cands = synth.loop_closure_scenario(W, H, n_candidates, sensor=True)
    for i, xi in enumerate(([0.1, 0, 0, 0, np.pi / 2, 0], [0, 0, 0.1, 0, 0.75 * np.pi, 0], [0.05, 0, 0, 0, np.pi, 0], [0.9, 0, 0, 0, 0, 0])):
        T = synth.se3_exp(xi)
        cands.append(dict(id=200 + 2 * i, frame=synth.raw_to_float(*synth.sensor_frame(W, H, T, synth.SEED, 60 + i)), pose_true=T, pose=T))

    def make(e):
        p = capi.RgbdImagePyramid(e["frame"][0], e["frame"][1], K, LEVELS)
        nb = synth.raw_to_float(*synth.sensor_frame(W, H, synth.se3_exp(synth.XI_STEP_STREAM) @ e["pose_true"],
                                                    synth.SEED + 77 if e["id"] == 60 else synth.SEED, 200 + e["id"]))
        return Cn.Keyframe(e["id"], p, e["pose"], Cn.LogLikelihoodTrackingResultEvaluation(
            trk.match(p, capi.RgbdImagePyramid(nb[0], nb[1], K, LEVELS))))

    kfs = [make(key)] + [make(c) for c in cands]
    plain = Cn.NearestNeighborConstraintSearch(1.0).findPossibleConstraints(kfs, kfs[0])
    # the coarse threshold: in the widest gap of the ratios stage 1 observes when nothing is rejected by a ratio
    val = Cn.createConstraintProposalValidator(tracker=trk, min_constraint_ratio=0.0, ratio_coarse=-1e300, ratio_fine=-1e300)
    val.stages = val.stages[:1]
    thresholds = dict(min_constraint_ratio=0.2, ratio_fine=-1e300,
                      ratio_coarse=mid_gap([p.Votes[3].Value for p in val.validate(Cn.proposalsForCandidates(kfs[0], plain))]))

    def validate(found):
        props = Cn.proposalsForCandidates(kfs[0], found)
        val = Cn.createConstraintProposalValidator(tracker=trk, **thresholds)
        val.validate(props)
        return sorted({tuple(sorted((p.Reference.id, p.Current.id))) for p in props}), round(val.native_ms, 3)

    kept_plain, ms_plain = validate(plain)
    rows = {"keyframes": len(kfs), "thresholds": thresholds, "radius_candidates": [k.id for k in plain],
            "validated_without_pruning": kept_plain, "validate_ms_without_pruning": ms_plain, "min_overlap": {}}
    for o in overlaps:
        search = Cn.NearestNeighborConstraintSearch(1.0, o, tracker=trk)
        (found, search_ms) = timed(lambda: search.findPossibleConstraints(kfs, kfs[0]))
        kept, ms = validate(found)
        rows["min_overlap"][str(o)] = {
            "candidates": [k.id for k in found], "overlaps": [round(float(v), 4) for v in search.overlaps],
            "candidates_removed": len(plain) - len(found), "stage1_alignments_removed": 4 * (len(plain) - len(found)),
            "search_ms": round(search_ms, 3), "validate_ms": ms, "validated": kept,
            "validated_lost": [pair for pair in kept_plain if pair not in kept]}
        print(f"  min_overlap {o}: {len(found)} of {len(plain)} candidates, {len(kept)} of {len(kept_plain)} validated, "
              f"lost {rows['min_overlap'][str(o)]['validated_lost']}")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[50, 200])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--stage1-candidates", type=int, default=49)
    ap.add_argument("--scenario-candidates", type=int, default=12)
    ap.add_argument("--overlaps", type=float, nargs="+", default=[0.1, 0.3, 0.5, 0.7])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covisibility.json"))
    a = ap.parse_args()
    K = synth.intrinsics_for(W, H)
    trk = capi.DenseTracker()
    report = {"image": [W, H], "reps": a.reps, "format": "[median, min, max]", "sizes": {}}
    pyrs, kfs = [], []
    for N in sorted(a.sizes):
        for k in range(len(pyrs), N + 1):  # one frame more than keyframes: every keyframe's evaluation comes from its successor
            pyrs.append(capi.RgbdImagePyramid(*synth.render(W, H, pose(k), frame_id=k), K, LEVELS))
        for k in range(len(kfs), N):
            kfs.append(Cn.Keyframe(2 * k, pyrs[k], pose(k), Cn.LogLikelihoodTrackingResultEvaluation(trk.match(pyrs[k], pyrs[k + 1]))))
        print(f"N = {N}")
        entry = covisibility_rows(trk, kfs[:N], a.reps)
        entry["stage_1"] = stage1_row(trk, kfs[:N], min(a.stage1_candidates, N - 1), a.reps)
        report["sizes"][str(N)] = entry
    print("pruning:")
    report["pruning"] = scenario(trk, a.scenario_candidates, a.overlaps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
