"""Writes tests/golden/counted_selections_parent.npz: transformation, information, log-likelihood, iterations per level and valid pixels
per level of every case of tests/counted_selection_cases.py, from single match() calls in the default reciprocal mode.

Run it on the GPU against a library built from the commit BEFORE a change that must not move a bit, given through DVO_AMD_LIB:

    DVO_AMD_LIB=/path/to/parent/libdvo_amd.so python scripts/record_counted_selections_fixture.py [OUT.npz]

tests/test_counted_selections.py then holds the working tree's library to these bits.  (The host-rcpps mode is not recorded: its
table is the recording host's, see tests/test_rcp_mode.py.)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import counted_selection_cases as cases  # noqa: E402
from dvo_slam_amd import capi, synth  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", cases.FIXTURE)
    capi.lib()
    print("library:", os.environ.get("DVO_AMD_LIB", "(the tree's own)"), "build id", capi.build_id())
    arrays = {}
    for name, result in cases.Scene(capi, synth).singles("exact").items():
        s = cases.summary(result)
        print(name, "iterations", s["iterations"], "valid", s["valid_pixels"], "loglik", s["log_likelihood"][0], "NaN" if result.isNaN() else "")
        for field in cases.FIELDS:
            arrays[f"{name}/{field}"] = s[field]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
