"""The residual pass on exactly counted point sets (tests/counted_selection_cases.py): 0, 1, 63, 64, 65, 1 023, 1 024 and 1 025
selected points on a level walked in 4-step segments -- both sides of a wave step and of a block --, and an 80x48 pair whose top
level is mostly padding.  The step loop of k_tick issues its gathers in front of the Gram stage and its reference prefetch behind
it; no arithmetic moved, so every check is equality: against results recorded from the commit before that change
(tests/golden/counted_selections_parent.npz, written by scripts/record_counted_selections_fixture.py), and of a batch against single calls
in both reciprocal modes."""
import os
import re

import numpy as np
import pytest

import counted_selection_cases as cases
import selection_mask_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", cases.FIXTURE)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_the_fixture_holds_every_case_and_field():
    with np.load(GOLDEN) as z:
        assert sorted(z.files) == sorted(f"{c}/{f}" for c in cases.case_names() for f in cases.FIELDS)
        for c in cases.case_names():
            assert z[f"{c}/transformation"].shape == (4, 4) and z[f"{c}/information"].shape == (6, 6)
            levels = cases.SMALL[2] if c.startswith("w") else 1
            assert z[f"{c}/iterations"].shape == (levels,) and z[f"{c}/valid_pixels"].shape == (levels,)
    assert os.path.getsize(GOLDEN) < 64 * 1024


@pytest.mark.parametrize("n", cases.COUNTS)
def test_count_masks_keep_exactly_n_selected_pixels_in_scan_order(n):
    rng = np.random.default_rng(3)
    selected = (rng.uniform(size=(cases.H >> 1, cases.W >> 1)) < 0.6).astype(np.uint8)
    p0, p1 = cases.count_mask_planes(selected, n)
    assert p0.shape == (cases.H, cases.W) and p0.all()
    assert int(p1.sum()) == n and not (p1 & ~selected & 1).any()
    if n > 1:  # spread over the whole selection, first and last selected pixel included
        at = np.flatnonzero(selected.ravel())
        assert p1.ravel()[at[0]] and p1.ravel()[at[-1]]


def test_k_tick_keeps_four_waves_per_simd_without_scratch():
    """The gathers stand in front of the Gram stage only because three placements keep the register allocator inside 128 VGPRs
    (DESIGN.md section 10 item 37); a compiler that lays the pass out differently brings scratch back silently.  Read from the
    built library's own metadata (scripts/kernel_resources.sh): every matrix-form k_tick has at most 128 VGPRs, no scratch and
    no spilled register."""
    import subprocess

    from dvo_slam_amd import _build

    out = subprocess.run(["bash", os.path.join(ROOT, "scripts", "kernel_resources.sh"), _build.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    rows = {}
    for line in out.splitlines():
        m = re.match(r"void dvo_amd::(k_tick(?:_small)?<[^>]*>)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s", line)
        if m:
            rows[m.group(1)] = tuple(int(v) for v in m.group(2, 4, 5))
    matrix_form = ["k_tick<1, 0>", "k_tick<1, 1>", "k_tick<1, 2>", "k_tick_small<0>", "k_tick_small<1>", "k_tick_small<2>"]
    assert sorted(rows) == sorted(matrix_form + ["k_tick<0, 0>"]), out
    for name in matrix_form:
        vgpr, scratch, spilled = rows[name]
        assert vgpr <= 128 and scratch == 0 and spilled == 0, (name, rows[name])
    assert rows["k_tick<0, 0>"][1:] == (0, 0)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene(synth):
    from dvo_slam_amd import capi

    capi.lib()
    return cases.Scene(capi, synth)


@pytest.fixture(scope="module")
def singles(scene):
    return {mode: scene.singles(mode) for mode in ("exact", "host_sse")}


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.case_names())
def test_match_equals_the_parent_commits_result_bit_for_bit(singles, case):
    got = cases.summary(singles["exact"][case])
    with np.load(GOLDEN) as z:
        for field in cases.FIELDS:
            want = z[f"{case}/{field}"]
            print(case, field, "got", got[field].ravel()[:6], "want", want.ravel()[:6])
            assert cases.same_bits(got[field], want), (case, field)


@pytest.mark.gpu
def test_the_counted_level_is_walked_in_four_step_segments(scene):
    """What makes the counts straddle a wave step and a block: the default geometry gives level 1 of 160x120 four 64-point steps
    per wave segment, so a block of four segments holds 1 024 points.  If the step table moves, the counts have to move with it."""
    counted, small = scene.trackers()
    steps, blocks, points = counted.level_geometry(scene.refs[cases.COUNTS[-1]], cases.LEVEL)
    assert steps == cases.STEPS and cases.BLOCK_POINTS == 4 * steps * 64 == 1024
    assert points >= max(cases.COUNTS) and blocks == -(-points // cases.BLOCK_POINTS) >= 2  # (the unmasked selection: several blocks)
    assert {1, cases.BLOCK_POINTS - 1, cases.BLOCK_POINTS, cases.BLOCK_POINTS + 1, 63, 64, 65} <= set(cases.COUNTS)
    top = cases.SMALL[2] - 1
    w, h = cases.SMALL[0] >> top, cases.SMALL[1] >> top
    steps, blocks, points = small.level_geometry(scene.small_ref, top)
    assert blocks == 1 and points <= w * h < 64 * 4 * steps  # less than one block: the rest of it is padding


@pytest.mark.gpu
def test_the_counted_cases_report_exactly_their_count(singles):
    """A level's ValidPixels is the selection's count (the reference's PointSelection size, odd trailing point included): exactly
    the number of points the mask left, in both modes -- a counted padding lane or a lost point shows here.  The valid
    constraints of every iteration are points that were walked: at most the count less an odd trailing point (Q3).  An alignment
    over no points at all is reported as failed."""
    for mode in ("exact", "host_sse"):
        for n in cases.COUNTS:
            r = singles[mode][f"n{n}"]
            assert len(r.Levels) == 1 and r.Levels[0]["ValidPixels"] == n, (mode, n, r.Levels[0]["ValidPixels"])
            for it in r.Levels[0]["Iterations"]:
                assert 0 <= it["ValidConstraints"] <= (n & ~1), (mode, n, it["ValidConstraints"])
        assert singles[mode]["n0"].isNaN()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["exact", "host_sse"])
@pytest.mark.parametrize("in_flight", [0, 1, 3])
def test_a_batch_equals_the_single_calls_bit_for_bit(scene, singles, mode, in_flight):
    counted, small = scene.trackers(mode)
    pairs = scene.pairs()
    refs, curs, masks = [p[1] for p in pairs[:-1]], [p[2] for p in pairs[:-1]], [p[3] for p in pairs[:-1]]
    got = counted.match_batch(refs, curs, masks=masks, in_flight=in_flight)
    for (name, *_), r in zip(pairs[:-1], got):
        assert selection_mask_cases.same_result(r, singles[mode][name]), (mode, in_flight, name)
    name, ref, cur, _, _ = pairs[-1]
    for r in small.match_batch([ref] * 3, [cur] * 3, in_flight=in_flight):
        assert selection_mask_cases.same_result(r, singles[mode][name]), (mode, in_flight, name)
