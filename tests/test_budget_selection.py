"""Point-budget selection masks (dvo_amd_mask_create_budget): TOPK and GRID masks ranked on the device from a resident pyramid.
The rules are exact -- a total order, integer counts -- so every mask comparison is equality with the numpy restatement in
budget_selection_cases.py; the alignment behind a budget mask is compared bit for bit with the alignment behind the same planes
uploaded from the host, and sanity-bounded against the ground truth."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import budget_selection_cases as budget
import selection_mask_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, LEVELS = 160, 120, 4
SW, SH, SLEVELS = 32, 30, 3  # level 1 has 15 rows: its odd trailing row has no child level
K_SMALL = (30.0, 30.0, 15.5, 14.5)
NEW_SYMBOLS = ["dvo_amd_default_budget_options", "dvo_amd_mask_create_budget"]
INVALID_ARGUMENT, NO_DEVICE, DEVICE_MISMATCH = 1, 2, 8


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_the_library_exports_the_budget_entries_and_the_binding_covers_the_headers(capi):
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
    declared = set()
    for header in ("dvo_amd.h", "dvo_amd_debug.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared |= set(re.findall(r"\b(dvo_amd_[a-z0-9_]+)\s*\(", text))
    assert sorted(capi.EXPORTS) == sorted(declared)
    assert L.dvo_amd_abi_version() == 3
    assert (capi.BUDGET_TOPK, capi.BUDGET_GRID) == (0, 1)
    assert capi.MAX_MASKED_SELECTIONS == 8 and (capi.MASK_ALL, capi.MASK_ANY) == (0, 1)
    assert capi.level_budgets(20000, 4) == [20000, 5000, 1250, 312]
    assert capi.level_budgets(1000, 4, minimum=100) == [1000, 250, 100, 100]


def test_the_default_budget_options_are_the_documented_ones(capi):
    opt = capi.BudgetOptions()
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt))
    capi.lib().dvo_amd_default_budget_options(C.byref(opt))
    assert opt.rule == capi.BUDGET_TOPK
    assert list(opt.budget) == [-1] * capi.MAX_LEVELS and list(opt.cell) == [1] * capi.MAX_LEVELS
    assert (opt.intensity_threshold, opt.depth_threshold, opt.depth_weight) == (0.0, 0.0, 0.0)
    assert opt.within is None
    capi.lib().dvo_amd_default_budget_options(None)  # a no-op


def test_null_pointers_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    opt = capi.BudgetOptions()
    L.dvo_amd_default_budget_options(C.byref(opt))
    something = C.create_string_buffer(64)  # stands for a pyramid: a NULL next to it is refused before anything is looked at
    p = C.c_void_p(C.addressof(something))
    for what, (pyr, o, with_out) in {"pyramid": (None, C.byref(opt), True), "options": (p, None, True),
                                     "out": (p, C.byref(opt), False), "all": (None, None, False)}.items():
        handle = C.c_void_p(0xDEAD)
        rc = L.dvo_amd_mask_create_budget(pyr, o, C.byref(handle) if with_out else None)
        assert rc == INVALID_ARGUMENT, (what, rc)
        if with_out:
            assert not handle.value, what
        reason = L.dvo_amd_last_error().decode()
        assert reason.startswith("dvo_amd_mask_create_budget: ") and "NULL" in reason, (what, reason)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene(capi, small_pair):
    (Ir, Zr), (Ic, Zc), Tgt, K = small_pair
    ref, cur = capi.RgbdImagePyramid(Ir, Zr, K, LEVELS), capi.RgbdImagePyramid(Ic, Zc, K, LEVELS)
    trk = capi.DenseTracker(capi.Config(FirstLevel=LEVELS - 1, LastLevel=0))
    return dict(ref=ref, cur=cur, trk=trk, Tgt=Tgt, K=K, frames=((Ir, Zr), (Ic, Zc)))


def _pyramid(capi, scene, which):
    """the frames the masks are checked on.  big: small_pair's reference with a NaN-depth square; raw: the 32x30 8-bit frame
    whose keys tie in large groups"""
    if which == "big":
        (Ir, Zr), _ = scene["frames"]
        return capi.RgbdImagePyramid(Ir, budget.nan_patch(Zr), scene["K"], LEVELS), LEVELS
    grey, depth = budget.raw_tie_frame(SW, SH)
    return capi.RgbdImagePyramid.from_raw(grey, depth, K_SMALL, SLEVELS), SLEVELS


def _planes(mask, levels):
    return [mask.download(l) for l in range(levels)]


def _raw_create(capi, pyramid, **fields):
    """dvo_amd_mask_create_budget itself with the default options and `fields` on top: (status, handle)"""
    L = capi.lib()
    opt = capi.BudgetOptions()
    L.dvo_amd_default_budget_options(C.byref(opt))
    for k, v in fields.items():
        if k in ("budget", "cell"):
            getattr(opt, k)[:] = v
        else:
            setattr(opt, k, v)
    handle = C.c_void_p(0xDEAD)
    rc = L.dvo_amd_mask_create_budget(pyramid._h, C.byref(opt), C.byref(handle))
    return rc, handle


@pytest.mark.gpu
def test_invalid_options_and_mismatched_within_masks_are_refused(capi, scene):
    L = capi.lib()
    ref = scene["ref"]
    ones, bad_cell = [1] * capi.MAX_LEVELS, [1] * capi.MAX_LEVELS
    bad_cell[LEVELS - 1] = 0
    beyond = [1] * capi.MAX_LEVELS
    beyond[LEVELS] = 0  # a level the pyramid does not have: not looked at
    nan, inf = float("nan"), float("inf")
    bad = {
        "rule 2": dict(rule=2), "rule -1": dict(rule=-1),
        "GRID with cell 0 on the last level": dict(rule=capi.BUDGET_GRID, cell=bad_cell),
        "GRID with a negative cell": dict(rule=capi.BUDGET_GRID, cell=[-3] + ones[1:]),
        "intensity threshold NaN": dict(intensity_threshold=nan), "intensity threshold inf": dict(intensity_threshold=inf),
        "depth threshold NaN": dict(depth_threshold=nan), "depth threshold -inf": dict(depth_threshold=-inf),
        "depth_weight -1": dict(depth_weight=-1.0), "depth_weight NaN": dict(depth_weight=nan), "depth_weight inf": dict(depth_weight=inf),
    }
    for what, fields in bad.items():
        rc, handle = _raw_create(capi, ref, **fields)
        assert rc == INVALID_ARGUMENT, (what, rc)
        assert not handle.value, what
        assert L.dvo_amd_last_error().decode().startswith("dvo_amd_mask_create_budget: "), what
    other_size = capi.SelectionMask.from_level0(np.ones((SH, SW), np.uint8), 1)
    shallow = capi.SelectionMask.from_level0(np.ones((H, W), np.uint8), LEVELS - 1)
    for what, within in (("size", other_size), ("levels", shallow)):
        rc, handle = _raw_create(capi, ref, within=within._h)
        assert rc == INVALID_ARGUMENT and not handle.value, (what, rc)
        assert "mask" in L.dvo_amd_last_error().decode()
    if L.dvo_amd_device_count() > 1:
        elsewhere = capi.SelectionMask.from_level0(np.ones((H, W), np.uint8), LEVELS, device=1)
        rc, handle = _raw_create(capi, ref, within=elsewhere._h)
        assert rc == DEVICE_MISMATCH and not handle.value
    # what is not looked at is not refused: TOPK with cells of 0, GRID with a cell of 0 beyond the pyramid's levels
    for fields in (dict(cell=[0] * capi.MAX_LEVELS), dict(rule=capi.BUDGET_GRID, cell=beyond)):
        rc, handle = _raw_create(capi, ref, **fields)
        assert rc == 0 and handle.value
        L.dvo_amd_mask_release(handle)


@pytest.mark.gpu
@pytest.mark.parametrize("depth_weight", [0.0, 2.5])
@pytest.mark.parametrize("which", ["big", "raw"])
def test_topk_equals_numpy(capi, scene, which, depth_weight):
    """K over 0, 1, 2, |C|-1, |C|, |C|+1, every candidate (-1), |C|/2 and a K strictly inside a group of at least 3 equal keys.
    The raw frame is built so that every level has such a group (the test fails if one has none); small_pair's float frame is
    cut inside a group wherever it has one."""
    pyr, levels = _pyramid(capi, scene, which)
    kc = [budget.keys_and_candidates(pyr, l, 0.0, 0.0, depth_weight) for l in range(levels)]
    n_cand = [int(c.sum()) for _, c in kc]
    assert all(n > 8 for n in n_cand)
    groups = [budget.tie_group(k, c, 3) for k, c in kc]
    if which == "raw":
        assert all(g is not None for g in groups), "vacuous: a level of the raw frame has no three equal keys"
    inside = []
    for l, g in enumerate(groups):
        if g is not None:
            a, b = g
            o = budget.order(*kc[l])
            keys = kc[l][0].ravel()[o]
            assert b - a >= 3 and len(set(keys[a:b].tolist())) == 1 and a < a + 1 < b  # proven: K = a + 1 cuts the group
            inside.append(a + 1)
        else:
            inside.append(n_cand[l] // 3)
    kinds = {"0": [0] * levels, "1": [1] * levels, "2": [2] * levels, "|C|-1": [n - 1 for n in n_cand], "|C|": n_cand,
             "|C|+1": [n + 1 for n in n_cand], "every": [-1] * levels, "|C|/2": [n // 2 for n in n_cand], "inside a tie": inside}
    for kind, budgets in kinds.items():
        mask = capi.SelectionMask.from_budget(pyr, capi.BUDGET_TOPK, budget=budgets, depth_weight=depth_weight)
        info = mask.info()
        assert (info["width"], info["height"], info["levels"]) == ((W, H, LEVELS) if which == "big" else (SW, SH, SLEVELS))
        for l in range(levels):
            want = budget.topk_plane(*kc[l], budgets[l])
            got = mask.download(l)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (kind, l)
            assert info["kept"][l] == (n_cand[l] if budgets[l] < 0 else min(budgets[l], n_cand[l])), (kind, l)
            assert info["kept"][l] == int(got.sum())


@pytest.mark.gpu
def test_all_ties_keep_the_first_pixels_in_scan_order(capi):
    """A linear ramp over valid depth: every interior pixel of a level shares one key, the highest of the level (the border's
    one-sided differences are half as steep).  K below the interior's size keeps the first K interior pixels in scan order."""
    I, Z = budget.ramp_frame(SW, SH)
    pyr = capi.RgbdImagePyramid(I, Z, K_SMALL, SLEVELS)
    budgets, want = [], []
    for l in range(SLEVELS):
        key, cand = budget.keys_and_candidates(pyr, l)
        h, w = key.shape
        interior = np.zeros((h, w), bool)
        interior[1:-1, 1:-1] = True
        assert cand.all()
        assert len(set(key[interior].tolist())) == 1 and key[~interior].max() < key[interior].min()
        k = int(interior.sum()) * 2 // 3
        first = np.flatnonzero(interior.ravel())[:k]
        plane = np.zeros(h * w, np.uint8)
        plane[first] = 1
        budgets.append(k), want.append(plane.reshape(h, w))
        assert np.array_equal(budget.topk_plane(key, cand, k), want[-1])  # (the restatement says the same)
    mask = capi.SelectionMask.from_budget(pyr, capi.BUDGET_TOPK, budget=budgets)
    for l in range(SLEVELS):
        assert np.array_equal(mask.download(l), want[l]), l
    assert mask.info()["kept"] == budgets
    # past the interior: all of it and the strongest border pixels
    for extra in (1, 5):
        more = [int(w_.sum()) * 3 // 2 + extra for w_ in want]
        mask = capi.SelectionMask.from_budget(pyr, capi.BUDGET_TOPK, budget=more)
        for l in range(SLEVELS):
            assert np.array_equal(mask.download(l), budget.topk_plane(*budget.keys_and_candidates(pyr, l), more[l])), (extra, l)


@pytest.mark.gpu
def test_topk_at_the_digit_edges_of_the_radix_select(capi):
    """Keys over more than 20 binades, a group that differs in the lowest mantissa bits only, and +inf.  K at every boundary of
    those groups and at the first positions of the order where the first, second and third digit change, each -1, +0, +1."""
    I, Z = budget.digit_frame(SW, SH)
    pyr = capi.RgbdImagePyramid(I, Z, K_SMALL, SLEVELS)
    key, cand = budget.keys_and_candidates(pyr, 0)
    o = budget.order(key, cand)
    k = key.ravel()[o]
    finite = k[(k < 0x7F800000) & (k > 0)]
    assert int(finite.max() >> 23) - int(finite.min() >> 23) >= 20  # binades between the weakest and the strongest gradient
    n_inf = int((k == 0x7F800000).sum())
    assert n_inf >= 1 and k[0] == 0x7F800000
    one = np.float32(1.0).view(np.uint32)
    low = np.flatnonzero((k >> 8) == (one >> 8))  # the keys that share 1.0's upper 24 bits
    assert len(low) >= 8 and len(set((k[low] & 0xFF).tolist())) >= 4 and np.array_equal(low, np.arange(low[0], low[-1] + 1))
    edges = {n_inf, int(low[0]), int(low[-1]) + 1}
    for shift in (24, 16, 8):
        changes = np.flatnonzero((k[1:] >> shift) != (k[:-1] >> shift)) + 1
        assert len(changes) >= 2
        edges.update(int(c) for c in changes[:4])
        edges.add(int(changes[-1]))
    for e in sorted(edges):
        for K in (e - 1, e, e + 1):
            if 0 <= K <= len(o):
                mask = capi.SelectionMask.from_budget(pyr, capi.BUDGET_TOPK, budget=[K, 0, 0])
                assert np.array_equal(mask.download(0), budget.topk_plane(key, cand, K)), K
                assert mask.info()["kept"] == [K, 0, 0]
    # ... and the coarser levels of this frame, whatever their keys are
    for l in (1, 2):
        kc = budget.keys_and_candidates(pyr, l)
        for K in (1, int(kc[1].sum()) // 2):
            b = [0] * SLEVELS
            b[l] = K
            assert np.array_equal(capi.SelectionMask.from_budget(pyr, capi.BUDGET_TOPK, budget=b).download(l), budget.topk_plane(*kc, K))


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [1, 2, 3, 7, 64])
@pytest.mark.parametrize("which", ["big", "raw"])
def test_grid_equals_numpy(capi, scene, which, cell):
    """Partial cells at the right and bottom edges (3, 7), one cell that holds a whole level (64 on the small levels), cells
    emptied by invalid depth, and -- on the raw frame -- cells whose strongest key is shared, where the lowest index wins."""
    pyr, levels = _pyramid(capi, scene, which)
    dw = 0.5 if which == "big" else 0.0
    mask = capi.SelectionMask.from_budget(pyr, capi.BUDGET_GRID, cell=cell, depth_weight=dw)
    info = mask.info()
    empty_cells = shared_maximum = 0
    for l in range(levels):
        key, cand = budget.keys_and_candidates(pyr, l, 0.0, 0.0, dw)
        want = budget.grid_plane(key, cand, cell)
        got = mask.download(l)
        assert np.array_equal(got, want), l
        assert info["kept"][l] == int(want.sum())
        h, w = key.shape
        for y0 in range(0, h, cell):
            for x0 in range(0, w, cell):
                c, k = cand[y0:y0 + cell, x0:x0 + cell], key[y0:y0 + cell, x0:x0 + cell]
                assert int(want[y0:y0 + cell, x0:x0 + cell].sum()) == (1 if c.any() else 0)
                empty_cells += not c.any()
                shared_maximum += bool(c.any()) and int((k[c] == k[c].max()).sum()) > 1
        if cell == 1:
            assert np.array_equal(want, cand.astype(np.uint8))
        if cell >= max(h, w):
            assert int(want.sum()) == 1
    if cell in (2, 3, 7):
        assert empty_cells > 0, "vacuous: no cell was emptied by the invalid depth"
    if which == "raw" and cell in (2, 3, 7):
        assert shared_maximum > 0, "vacuous: no cell's strongest key is shared"


@pytest.mark.gpu
def test_candidates_follow_within_nan_intensity_and_the_thresholds(capi, scene):
    (Ir, Zr), _ = scene["frames"]
    I = Ir.copy()
    I[50, 70] = np.nan
    pyr = capi.RgbdImagePyramid(I, Zr, scene["K"], LEVELS)
    rng = np.random.default_rng(29)
    planes = [(rng.uniform(size=(H >> l, W >> l)) < 0.5).astype(np.uint8) * 3 for l in range(LEVELS)]
    within = capi.SelectionMask.from_levels(planes)
    for rule, kw in ((capi.BUDGET_GRID, dict(cell=4)), (capi.BUDGET_TOPK, dict(budget=[(W * H) >> (2 * l + 3) for l in range(LEVELS)]))):
        free = capi.SelectionMask.from_budget(pyr, rule, **kw)
        held = capi.SelectionMask.from_budget(pyr, rule, within=within, **kw)
        for l in range(LEVELS):
            got = held.download(l)
            key, cand = budget.keys_and_candidates(pyr, l, within=planes[l])
            want = budget.grid_plane(key, cand, 4) if rule == capi.BUDGET_GRID else budget.topk_plane(key, cand, kw["budget"][l])
            assert np.array_equal(got, want), (rule, l)
            assert not (got & (planes[l] == 0)).any()
            assert not np.array_equal(got, free.download(l) & (planes[l] != 0)), (rule, l)  # other pixels win, not fewer of the same
    # a NaN intensity makes Ix or Iy of its four neighbours NaN.  Where their depth is valid the validity-only predicate keeps
    # them -- but a NaN saliency is no candidate, for either rule.  (The pixel itself has finite derivatives and a finite
    # saliency: by the pinned rule it is a candidate like any other, as it is for the selection's own predicate.)
    valid = cases.threshold_predicate(pyr, 0, -1.0, -1.0)
    s = budget.saliency(pyr, 0, 0.0)
    assert np.isnan(s).sum() == 4 and (valid[np.isnan(s)] == 1).sum() >= 2
    for rule, kw in ((capi.BUDGET_TOPK, {}), (capi.BUDGET_GRID, dict(cell=1))):
        every = capi.SelectionMask.from_budget(pyr, rule, thresholds=(-1.0, -1.0), **kw).download(0)
        assert np.array_equal(every, (valid != 0) & ~np.isnan(s))
    # stricter thresholds: fewer candidates, exactly the predicate's
    loose = capi.SelectionMask.from_budget(pyr, capi.BUDGET_TOPK)
    strict = capi.SelectionMask.from_budget(pyr, capi.BUDGET_TOPK, thresholds=(2.5, 0.01))
    for l in range(LEVELS):
        _, cand = budget.keys_and_candidates(pyr, l, 2.5, 0.01)
        assert np.array_equal(strict.download(l), cand.astype(np.uint8))
        assert 0 < strict.info()["kept"][l] < loose.info()["kept"][l]


@pytest.mark.gpu
def test_two_builds_of_the_same_options_give_the_same_mask(capi, scene):
    for which in ("big", "raw"):
        pyr, levels = _pyramid(capi, scene, which)
        n = [int(budget.keys_and_candidates(pyr, l)[1].sum()) for l in range(levels)]
        for rule, kw in ((capi.BUDGET_TOPK, dict(budget=[k // 3 for k in n], depth_weight=1.0)), (capi.BUDGET_GRID, dict(cell=3)),
                         (capi.BUDGET_GRID, dict(cell=64))):
            a, b = capi.SelectionMask.from_budget(pyr, rule, **kw), capi.SelectionMask.from_budget(pyr, rule, **kw)
            assert a.info() == b.info()
            assert all(np.array_equal(x, y) for x, y in zip(_planes(a, levels), _planes(b, levels)))


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["topk", "grid"])
def test_the_selection_behind_a_budget_mask_is_the_mask(capi, scene, rule):
    """Every kept pixel passes the predicate the mask was built with: selecting behind it with those thresholds, or with
    validity only, returns the mask's plane."""
    (Ir, Zr), _ = scene["frames"]
    ti, td = 1.5, 0.005
    for thresholds in ((ti, td), (-1.0, -1.0)):
        ref = capi.RgbdImagePyramid(Ir, Zr, scene["K"], LEVELS)
        n = [int(budget.keys_and_candidates(ref, l, ti, td)[1].sum()) for l in range(LEVELS)]
        kw = dict(budget=[k // 2 for k in n]) if rule == "topk" else dict(cell=3)
        mask = capi.SelectionMask.from_budget(ref, capi.BUDGET_TOPK if rule == "topk" else capi.BUDGET_GRID, thresholds=(ti, td), **kw)
        for l in range(LEVELS):
            plane = mask.download(l)
            cnt, out = ref.select(l, thresholds[0], thresholds[1], mask=mask)
            assert np.array_equal(out, plane), (thresholds, l)
            assert cnt == int(plane.sum()) and 0 < cnt < n[l]


@pytest.mark.gpu
def test_tracking_behind_a_budget_mask(capi, scene, synth):
    """TOPK at half of each level's candidates and GRID with cell 2: the match behind the budget mask is the match behind the
    same planes uploaded from the host, bit for bit, alone and inside a batch next to unmasked pairs; it is another alignment
    than the unmasked one and still finds the pose (1e-3: the sanity bound of tests/test_selection_mask.py for this pair)."""
    ref, cur, trk = scene["ref"], scene["cur"], scene["trk"]
    n = [int(budget.keys_and_candidates(ref, l)[1].sum()) for l in range(LEVELS)]
    topk = capi.SelectionMask.from_budget(ref, capi.BUDGET_TOPK, budget=[k // 2 for k in n])
    grid = capi.SelectionMask.from_budget(ref, capi.BUDGET_GRID, cell=2)
    plain = trk.match(ref, cur)
    errors = {"unmasked": synth.pose_error(scene["Tgt"], plain.Transformation)}
    singles = {}
    for name, mask in (("topk", topk), ("grid", grid)):
        uploaded = capi.SelectionMask.from_levels(_planes(mask, LEVELS))
        got, want = trk.match(ref, cur, mask=mask), trk.match(ref, cur, mask=uploaded)
        assert not got.isNaN()
        assert cases.same_result(got, want), name
        assert not cases.same_result(got, plain), name
        singles[name] = got
        errors[name] = synth.pose_error(scene["Tgt"], got.Transformation)
    for in_flight in (1, 0):
        batch = trk.match_batch([ref] * 4, [cur] * 4, masks=[None, topk, grid, None], in_flight=in_flight)
        for k, want in enumerate((plain, singles["topk"], singles["grid"], plain)):
            assert cases.same_result(batch[k], want), (in_flight, k)
    print("pose error against the ground truth: " + ", ".join(f"{k} {v:.3e}" for k, v in errors.items()))
    for name, err in errors.items():
        assert err <= 1e-3, (name, err)
