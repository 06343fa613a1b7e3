"""What a masked point selection costs next to an unmasked one: the FIRST selection of a 640x480, 4-level pyramid (the one that
lives in the pyramid's slab), device time by the event bracket of dvo_amd_debug_ingest_timing around the selection's build --
descriptor upload, select + finish + prefix + compact per level, counter copy.

  unmasked   dvo_amd_pyramid_select               k_select
  ones       dvo_amd_pyramid_select_masked, an all-ones mask: the same points, so the same compaction -- the difference to
             `unmasked` is k_select_masked's one extra byte per pixel and nothing else
  cutout     ... a mask with a third of the image cut out: fewer points to compact

Every sample is a fresh pyramid (slab pool warm).  Three repeats, the variants interleaved sample by sample inside every repeat;
a repeat's figure is the median of its samples.  No bar is set: the expectation to confirm or refute is that one byte per pixel
on a kernel that streams 36 leaves the build within a few percent.
Every repeat runs in a fresh process of its own (warm-up included).
--baseline-lib PATH: a libdvo_amd.so built from the commit before masks existed; its `unmasked` figure is measured the same way,
its repeats alternating with this library's, and reported as `baseline_unmasked`.
Writes profiles/selection_mask.json.
Usage: python scripts/selection_mask_bench.py [--repeats 3] [--samples 24] [--baseline-lib PATH] [--out profiles/selection_mask.json]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, LEVELS = 640, 480, 4
SEL = (0.0, 0.0)  # DenseTracker::Config's default thresholds


def load(path):
    """the library through plain ctypes (a baseline library has no mask entries for the binding to describe)"""
    try:
        import torch  # noqa: F401  (one HIP runtime per process: torch's, when torch is installed -- as dvo_slam_amd.capi does)
    except Exception:
        pass
    L = C.CDLL(path)
    fp, vp, ip = C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int)
    L.dvo_amd_pyramid_create.argtypes = [C.c_int, fp, fp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int,
                                         C.c_double, C.POINTER(vp)]
    L.dvo_amd_pyramid_release.argtypes = [vp]
    L.dvo_amd_pyramid_release.restype = None
    L.dvo_amd_pyramid_select.argtypes = [vp, C.c_int, C.c_float, C.c_float, ip, C.POINTER(C.c_ubyte)]
    L.dvo_amd_debug_ingest_timing.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.dvo_amd_last_error.restype = C.c_char_p
    if hasattr(L, "dvo_amd_mask_create"):
        L.dvo_amd_mask_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.dvo_amd_mask_release.argtypes = [vp]
        L.dvo_amd_mask_release.restype = None
        L.dvo_amd_pyramid_select_masked.argtypes = [vp, C.c_int, C.c_float, C.c_float, vp, ip, C.POINTER(C.c_ubyte)]
    return L


def ok(L, rc, what):
    if rc != 0:
        raise SystemExit(f"{what}: status {rc} [{L.dvo_amd_last_error().decode()}]")


def measure(L, variants, repeats, samples):
    """{variant: [median ms of each repeat]}, {variant: selected pixels of level 0}"""
    from dvo_slam_amd import synth

    (I, Z), _, _ = synth.make_pair(W, H)
    I, Z = np.ascontiguousarray(I, np.float32), np.ascontiguousarray(Z, np.float32)
    K = synth.intrinsics_for(W, H)
    fpt = C.POINTER(C.c_float)
    masks = {}
    if "ones" in variants or "cutout" in variants:
        keep = {"ones": np.ones((H, W), np.uint8), "cutout": np.ones((H, W), np.uint8)}
        keep["cutout"][H // 4: (3 * H) // 4, W // 6: (5 * W) // 6] = 0
        for name in ("ones", "cutout"):
            masks[name] = C.c_void_p()
            ok(L, L.dvo_amd_mask_create(0, W, H, LEVELS, keep[name].ctypes.data, W, 0, 0, C.byref(masks[name])), "mask_create")
    ms, cnt = C.c_double(), C.c_int()
    counts = {}

    def sample(variant):
        h = C.c_void_p()
        ok(L, L.dvo_amd_pyramid_create(0, I.ctypes.data_as(fpt), Z.ctypes.data_as(fpt), W, H, W, *[float(k) for k in K], LEVELS, 0.0,
                                       C.byref(h)), "pyramid_create")
        if variant == "unmasked":
            ok(L, L.dvo_amd_pyramid_select(h, 0, SEL[0], SEL[1], C.byref(cnt), None), "select")
        else:
            ok(L, L.dvo_amd_pyramid_select_masked(h, 0, SEL[0], SEL[1], masks[variant], C.byref(cnt), None), "select_masked")
        ok(L, L.dvo_amd_debug_ingest_timing(0, 1, C.byref(ms)), "ingest_timing")
        L.dvo_amd_pyramid_release(h)
        counts[variant] = cnt.value
        return ms.value

    ok(L, L.dvo_amd_debug_ingest_timing(0, 1, C.byref(ms)), "ingest_timing")
    for _ in range(4):  # warm-up: code loaded, the slab pool holds a slab
        for v in variants:
            sample(v)
    out = {v: [] for v in variants}
    for _ in range(repeats):
        got = {v: [] for v in variants}
        for _ in range(samples):
            for v in variants:
                got[v].append(sample(v))
        for v in variants:
            out[v].append(float(np.median(got[v])))
    ok(L, L.dvo_amd_debug_ingest_timing(0, 0, C.byref(ms)), "ingest_timing")
    for m in masks.values():
        L.dvo_amd_mask_release(m)
    return out, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=24)
    ap.add_argument("--lib", default=None, help="(a repeat's own process) measure this library once and print the figures")
    ap.add_argument("--variants", default="unmasked,ones,cutout")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selection_mask.json"))
    a = ap.parse_args()
    if a.lib:
        ms, counts = measure(load(a.lib), a.variants.split(","), 1, a.samples)
        print("REPEAT " + json.dumps({"ms": {v: ms[v][0] for v in ms}, "selected": counts}))
        return
    from dvo_slam_amd import _build

    def one_repeat(lib, variants):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", lib, "--variants", variants, "--samples", str(a.samples)],
                             capture_output=True, text=True, timeout=300)
        if res.returncode != 0:
            raise SystemExit(f"the process measuring {lib} failed:\n" + res.stdout + res.stderr)
        return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("REPEAT ")][0][len("REPEAT "):])

    # every repeat of every library in a fresh process of its own (warm-up included), the two libraries alternating: whatever a
    # process's start, the clocks or the neighbours on the machine do to a figure, they do to both
    new_lib = _build.build()
    ms = {v: [] for v in ("unmasked", "ones", "cutout")}
    base, counts, base_count = [], {}, None
    for _ in range(a.repeats):
        if a.baseline_lib:
            r = one_repeat(a.baseline_lib, "unmasked")
            base.append(r["ms"]["unmasked"])
            base_count = r["selected"]["unmasked"]
        r = one_repeat(new_lib, "unmasked,ones,cutout")
        for v in ms:
            ms[v].append(r["ms"][v])
        counts = r["selected"]
    r3 = lambda xs: [round(x, 5) for x in xs]  # noqa: E731
    report = {"image": [W, H], "levels": LEVELS, "selection_thresholds": list(SEL), "repeats": a.repeats, "samples_per_repeat": a.samples,
              "what": "device ms of the first selection's build of a fresh pyramid (event bracket), median of the samples of each repeat; "
                      "every repeat in a process of its own, the libraries alternating",
              "selected_pixels_level0": counts,
              "device_ms": {v: {"repeats": r3(ms[v]), "median": round(float(np.median(ms[v])), 5)} for v in ms},
              "ratio_to_unmasked_per_repeat": {v: [round(m / u, 4) for m, u in zip(ms[v], ms["unmasked"])] for v in ("ones", "cutout")}}
    if base:
        report["baseline_unmasked"] = {"repeats": r3(base), "median": round(float(np.median(base)), 5), "selected_pixels_level0": base_count}
        report["unmasked_over_baseline_per_repeat"] = [round(u / b, 4) for u, b in zip(ms["unmasked"], base)]
        report["ones_over_baseline_per_repeat"] = [round(m / b, 4) for m, b in zip(ms["ones"], base)]
    print(json.dumps(report, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(report, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
