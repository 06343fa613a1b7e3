"""Selection masks (dvo_amd_mask): a device-resident mask pyramid behind the point selection, so that any predicate over the
reference pixels can run -- a cut-out region, a segmentation, a region of interest.  The mask enters in the select kernel and
nowhere else, so every check but one sanity bound is equality: against numpy for the mask pyramid and the selection, against
dvo_amd_match_selection (the oracle-checked path) for the alignment."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import selection_mask_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, LEVELS = 160, 120, 4
NEW_SYMBOLS = ["dvo_amd_mask_create", "dvo_amd_mask_create_levels", "dvo_amd_mask_retain", "dvo_amd_mask_release",
               "dvo_amd_mask_info", "dvo_amd_mask_download", "dvo_amd_pyramid_select_masked", "dvo_amd_match_masked",
               "dvo_amd_match_many_masked"]
INVALID_ARGUMENT, NO_DEVICE, CAPACITY = 1, 2, 7


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_the_library_exports_the_mask_entries_and_the_binding_covers_the_headers(capi):
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
    assert capi.MAX_MASKED_SELECTIONS == 8 and (capi.MASK_ALL, capi.MASK_ANY) == (0, 1)


def _create(L, w, h, levels, mask0, stride, rule, out=True):
    handle = C.c_void_p()
    rc = L.dvo_amd_mask_create(0, w, h, levels, mask0, stride, 0, rule, C.byref(handle) if out else None)
    return rc, handle


def _create_levels(L, w, h, levels, planes, strides, out=True):
    handle = C.c_void_p()
    rc = L.dvo_amd_mask_create_levels(0, w, h, levels, planes, strides, 0, C.byref(handle) if out else None)
    return rc, handle


def test_bad_mask_requests_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    keep = [np.ones((H >> l, W >> l), np.uint8) for l in range(LEVELS)]
    p0 = keep[0].ctypes.data
    planes = (C.c_void_p * LEVELS)(*[k.ctypes.data for k in keep])
    strides = (C.c_int * LEVELS)(*[W >> l for l in range(LEVELS)])
    holed = (C.c_void_p * LEVELS)(*[k.ctypes.data for k in keep])
    holed[2] = None
    short = (C.c_int * LEVELS)(*[W >> l for l in range(LEVELS)])
    short[1] = (W >> 1) - 1
    bad = {
        "create: out is NULL": lambda: _create(L, W, H, LEVELS, p0, W, 0, out=False),
        "create: mask0 is NULL": lambda: _create(L, W, H, LEVELS, None, W, 0),
        "create: a width that is no multiple of 4": lambda: _create(L, 158, H, 1, p0, W, 0),
        "create: too small": lambda: _create(L, 4, 1, 1, p0, W, 0),
        "create: level 4 of 160x120 is 10 wide": lambda: _create(L, W, H, 5, p0, W, 0),
        "create: stride < width": lambda: _create(L, W, H, LEVELS, p0, W - 1, 0),
        "create: levels 0": lambda: _create(L, W, H, 0, p0, W, 0),
        "create: levels 9": lambda: _create(L, 4096, 4096, capi.MAX_LEVELS + 1, p0, 4096, 0),
        "create: rule 2": lambda: _create(L, W, H, LEVELS, p0, W, 2),
        "create: rule -1": lambda: _create(L, W, H, LEVELS, p0, W, -1),
        "create_levels: out is NULL": lambda: _create_levels(L, W, H, LEVELS, planes, strides, out=False),
        "create_levels: planes is NULL": lambda: _create_levels(L, W, H, LEVELS, None, strides),
        "create_levels: strides is NULL": lambda: _create_levels(L, W, H, LEVELS, planes, None),
        "create_levels: planes[2] is NULL": lambda: _create_levels(L, W, H, LEVELS, holed, strides),
        "create_levels: strides[1] < the width of level 1": lambda: _create_levels(L, W, H, LEVELS, planes, short),
        "create_levels: level 4 of 160x120 is 10 wide": lambda: _create_levels(L, W, H, 5, planes, strides),
        "create_levels: levels 0": lambda: _create_levels(L, W, H, 0, planes, strides),
    }
    for what, call in bad.items():
        rc, handle = call()
        assert rc == INVALID_ARGUMENT, (what, rc)  # (not NO_DEVICE: the argument checks come first)
        assert not handle.value, what
        reason = L.dvo_amd_last_error().decode()
        assert reason.startswith("dvo_amd_mask_create") and len(reason) > len("dvo_amd_mask_create_levels: "), (what, reason)
    # a valid request goes on to the device: without one it is refused as such, with one it succeeds
    for rc, handle in (_create(L, W, H, LEVELS, p0, W, capi.MASK_ANY), _create_levels(L, W, H, LEVELS, planes, strides)):
        if L.dvo_amd_device_count() > 0:
            assert rc == 0 and handle.value
            L.dvo_amd_mask_release(handle)
        else:
            assert rc == NO_DEVICE and not handle.value
    # info / download of nothing
    assert L.dvo_amd_mask_info(None, None, None, None, None) == INVALID_ARGUMENT
    assert L.dvo_amd_mask_download(None, 0, None) == INVALID_ARGUMENT
    L.dvo_amd_mask_retain(None), L.dvo_amd_mask_release(None)  # no-ops, like the other handles'


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene(capi, small_pair):
    """small_pair as pyramids, a tracker over all four levels with the default thresholds, and the case-4 mask"""
    (Ir, Zr), (Ic, Zc), Tgt, K = small_pair
    ref, cur = capi.RgbdImagePyramid(Ir, Zr, K, LEVELS), capi.RgbdImagePyramid(Ic, Zc, K, LEVELS)
    trk = capi.DenseTracker(capi.Config(FirstLevel=LEVELS - 1, LastLevel=0))
    m0 = cases.level0_mask(W, H)
    return dict(ref=ref, cur=cur, trk=trk, Tgt=Tgt, K=K, frames=((Ir, Zr), (Ic, Zc)), m0=m0, unmasked=trk.match(ref, cur))


def _fresh_reference(capi, scene):
    (Ir, Zr), _ = scene["frames"]
    return capi.RgbdImagePyramid(Ir, Zr, scene["K"], LEVELS)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["all", "any"])
@pytest.mark.parametrize("size", [(W, H, LEVELS), (32, 30, 3)])
def test_mask_pyramid_equals_the_numpy_block_reduction(capi, rule, size):
    """(32, 30, 3): level 1 has 15 rows, so its odd trailing row has no parent in level 2"""
    w, h, levels = size
    m0 = cases.level0_mask(w, h)
    want = cases.mask_pyramid(m0, levels, rule == "any")
    mask = capi.SelectionMask.from_level0(m0, levels, capi.MASK_ANY if rule == "any" else capi.MASK_ALL)
    info = mask.info()
    assert (info["width"], info["height"], info["levels"]) == (w, h, levels)
    for l in range(levels):
        got = mask.download(l)
        assert got.shape == want[l].shape and got.dtype == np.uint8
        assert np.array_equal(got, want[l]), (rule, l)
    assert info["kept"] == [int(p.sum()) for p in want]
    assert 0 < info["kept"][levels - 1] < want[levels - 1].size


@pytest.mark.gpu
def test_given_levels_come_back_normalised_and_a_device_source_gives_the_same_planes(capi):
    import torch

    rng = np.random.default_rng(11)
    planes = [(rng.integers(0, 4, size=(H >> l, W >> l)) * rng.integers(1, 64, size=(H >> l, W >> l))).astype(np.uint8) for l in range(LEVELS)]
    mask = capi.SelectionMask.from_levels(planes)
    for l in range(LEVELS):
        assert np.array_equal(mask.download(l), (planes[l] != 0).astype(np.uint8))
    assert mask.info()["kept"] == [int((p != 0).sum()) for p in planes]
    # level 0 from device memory, with a row stride wider than the image, against the same bytes from the host
    m0 = cases.level0_mask(W, H)
    padded = np.zeros((H, W + 24), np.uint8)
    padded[:, :W] = m0
    d = torch.from_numpy(padded).cuda()
    torch.cuda.synchronize()
    for rule in (capi.MASK_ALL, capi.MASK_ANY):
        host = capi.SelectionMask.from_level0(m0, LEVELS, rule)
        dev = capi.SelectionMask.from_level0_device(d.data_ptr(), W, H, LEVELS, rule, stride=W + 24)
        assert dev.info() == host.info()
        for l in range(LEVELS):
            assert np.array_equal(dev.download(l), host.download(l))


@pytest.mark.gpu
@pytest.mark.parametrize("thresholds", [(0.0, 0.0), (-1.0, -1.0)])
def test_masked_selection_is_the_mask_and_the_unmasked_selection(capi, scene, thresholds):
    """Every level: output mask == mask[l] & select()'s output mask, count == its sum.  The Q3 rule (an odd trailing point is
    counted and marked but never walked) needs a level with an odd count: if the case-4 mask gives none for this threshold pair,
    one more selected pixel of level 0 is dropped, which makes level 0's count odd."""
    ref, (ti, td) = _fresh_reference(capi, scene), thresholds
    unmasked = [ref.select(l, ti, td) for l in range(LEVELS)]
    for cnt, out in unmasked:
        assert cnt == int(out.sum())
    m0 = (scene["m0"] != 0).astype(np.uint8)

    def expected(m0):
        return [mp & u[1] for mp, u in zip(cases.mask_pyramid(m0, LEVELS, False), unmasked)]

    if not any(int(e.sum()) & 1 for e in expected(m0)):
        y, x = np.argwhere(expected(m0)[0])[0]
        m0[y, x] = 0
    want = expected(m0)
    assert any(int(e.sum()) & 1 for e in want)
    mask = capi.SelectionMask.from_level0(m0, LEVELS, capi.MASK_ALL)
    for l in range(LEVELS):
        cnt, out = ref.select(l, ti, td, mask=mask)
        assert np.array_equal(out, want[l]), l
        assert cnt == int(want[l].sum())
        assert 0 < cnt < unmasked[l][0]


def _match_selection(capi, trk, ref, cur, ti, td):
    """dvo_amd_match_selection itself, the entry the oracle tests pin"""
    res, its = trk._alloc_results(1)
    rc = capi.lib().dvo_amd_match_selection(trk._h, ref._h, ti, td, cur._h, None, C.byref(res[0]))
    assert rc == 0, rc
    return capi.Result(res[0], its[0])


@pytest.mark.gpu
def test_a_mask_that_says_what_a_threshold_says_gives_the_threshold_match_bit_for_bit(capi, scene):
    """The predicate of a pair stricter than the configuration's, evaluated in numpy from the downloaded planes, uploaded level
    by level: tracking behind it with thresholds (-1, -1) is dvo_amd_match_selection with that pair -- same points, same order,
    same sums.  Which points are kept, and in which order, shows here."""
    ref, cur, trk = scene["ref"], scene["cur"], scene["trk"]
    ti, td = 2.5, 0.01
    planes = [cases.threshold_predicate(ref, l, ti, td) for l in range(LEVELS)]
    for l in range(LEVELS):
        assert 0 < planes[l].sum() < cases.threshold_predicate(ref, l, 0.0, 0.0).sum()  # stricter, and not empty
    mask = capi.SelectionMask.from_levels(planes)
    want = _match_selection(capi, trk, ref, cur, ti, td)
    got = trk.match(ref, cur, mask=mask, thresholds=(-1.0, -1.0))
    assert not want.isNaN()
    assert cases.same_result(got, want)
    assert not cases.same_result(want, scene["unmasked"])  # (the stricter pair is a different alignment)
    cfg = trk.configuration()  # the thresholds of the call did not stick
    assert cases.same_result(trk.match(ref, cur), scene["unmasked"]) and (cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold) == (0.0, 0.0)


@pytest.mark.gpu
def test_neutral_masks_change_nothing_alone_or_in_a_batch(capi, scene):
    ref, cur, trk = scene["ref"], scene["cur"], scene["trk"]
    ones = capi.SelectionMask.from_level0(np.ones((H, W), np.uint8), LEVELS)
    m = capi.SelectionMask.from_level0(scene["m0"], LEVELS, capi.MASK_ALL)
    plain = scene["unmasked"]
    assert cases.same_result(trk.match(ref, cur, mask=ones), plain)
    masked = trk.match(ref, cur, mask=m)
    assert not masked.isNaN() and not cases.same_result(masked, plain)
    singles = [plain, masked, plain, plain]
    for in_flight in (1, 0):
        batch = trk.match_batch([ref] * 4, [cur] * 4, masks=[None, m, None, ones], in_flight=in_flight)
        for k in range(4):
            assert cases.same_result(batch[k], singles[k]), (in_flight, k)
    assert all(cases.same_result(r, plain) for r in trk.match_batch([ref] * 2, [cur] * 2, masks=None))


@pytest.mark.gpu
def test_what_is_masked_out_cannot_influence_the_result(capi, scene, synth):
    """A rectangle of the reference replaced by noise (one NaN depth included), the mask (rule ALL) dropping it dilated by
    2^(levels-1) = 8 pixels: the 2x2 means of three coarser levels and the +-1 central differences of a kept pixel never reach into
    the rectangle, so the masked matches of the clean and of the corrupted reference are the same bits.  Unmasked they differ.
    The masked clean match still finds the pose: within 1e-3 of the ground truth (a sanity bound on the number of points left)."""
    (Ir, Zr), _ = scene["frames"]
    cur, trk = scene["cur"], scene["trk"]
    x0, x1, y0, y1, margin = 64, 96, 40, 64, 1 << (LEVELS - 1)
    assert all(v % 8 == 0 for v in (x0, x1, y0, y1))
    rng = np.random.default_rng(23)
    Ib, Zb = Ir.copy(), Zr.copy()
    Ib[y0:y1, x0:x1] = rng.uniform(0.0, 255.0, size=(y1 - y0, x1 - x0)).astype(np.float32)
    Zb[y0:y1, x0:x1] = rng.uniform(0.4, 4.0, size=(y1 - y0, x1 - x0)).astype(np.float32)
    Zb[(y0 + y1) // 2, (x0 + x1) // 2] = np.nan
    clean = _fresh_reference(capi, scene)
    corrupted = capi.RgbdImagePyramid(Ib, Zb, scene["K"], LEVELS)
    keep = np.ones((H, W), np.uint8)
    keep[y0 - margin:y1 + margin, x0 - margin:x1 + margin] = 0
    mask = capi.SelectionMask.from_level0(keep, LEVELS, capi.MASK_ALL)
    a, b = trk.match(clean, cur, mask=mask), trk.match(corrupted, cur, mask=mask)
    assert not a.isNaN()
    assert cases.same_result(a, b)
    assert not cases.same_result(trk.match(corrupted, cur), scene["unmasked"])
    err_plain, err_masked = synth.pose_error(scene["Tgt"], scene["unmasked"].Transformation), synth.pose_error(scene["Tgt"], a.Transformation)
    print(f"pose error against the ground truth: unmasked {err_plain:.3e}, masked {err_masked:.3e}")
    assert err_plain <= 1e-3
    assert err_masked <= 1e-3


@pytest.mark.gpu
def test_a_masked_selection_is_built_once_and_is_keyed_by_the_masks_serial(capi, scene):
    """The second select with one mask finds the selection in the cache: the bracket of dvo_amd_debug_ingest_timing (every
    selection build runs inside it) does not move.  The key is the mask's serial, not its address: after a mask is released, a
    new mask with other content -- wherever the allocator puts it -- selects by its own content, never the released one's
    selection; and the released mask's selection is still the pyramid's, the cached unmasked and masked results stay what they were."""
    ref = _fresh_reference(capi, scene)
    unmasked = [ref.select(l)[1] for l in range(LEVELS)]
    a0 = (scene["m0"] != 0).astype(np.uint8)
    b0 = np.ones((H, W), np.uint8)
    b0[:, : W // 2] = 0
    want_a = [mp & u for mp, u in zip(cases.mask_pyramid(a0, LEVELS, False), unmasked)]
    want_b = [mp & u for mp, u in zip(cases.mask_pyramid(b0, LEVELS, False), unmasked)]
    capi.ingest_timing(True)
    try:
        a = capi.SelectionMask.from_level0(a0, LEVELS)
        before = capi.ingest_timing(True)
        first = ref.select(1, mask=a)
        built = capi.ingest_timing(True)
        assert built > 0.0
        moved = [built != before]
        again = [ref.select(l, mask=a) for l in range(LEVELS)]
        assert capi.ingest_timing(True) == built  # all four levels came from the one build
        assert first[0] == again[1][0] and np.array_equal(first[1], again[1][1])
        assert all(np.array_equal(again[l][1], want_a[l]) for l in range(LEVELS))
        del a  # released: the device planes of the mask are gone
        b = capi.SelectionMask.from_level0(b0, LEVELS)
        got_b = [ref.select(l, mask=b) for l in range(LEVELS)]
        moved.append(capi.ingest_timing(True) != built)
        assert all(np.array_equal(got_b[l][1], want_b[l]) for l in range(LEVELS))
        assert any(moved)  # (two builds: two device times equal to the last bit would hide one move, not two)
        a2 = capi.SelectionMask.from_level0(a0, LEVELS)  # the same content again is a new mask: a new entry, the same selection
        assert all(np.array_equal(ref.select(l, mask=a2)[1], want_a[l]) for l in range(LEVELS))
        assert all(np.array_equal(ref.select(l)[1], unmasked[l]) for l in range(LEVELS))
    finally:
        capi.ingest_timing(False)


@pytest.mark.gpu
def test_a_selection_outlives_its_mask_inside_the_queue(capi, scene):
    """The queue retains a pair's mask from submission until the pair's selection is resolved, and the selection holds planes of
    its own: masks that nobody but the call holds, in a batch wider than the residency, give the results of masks that live on."""
    ref, cur, trk = scene["ref"], scene["cur"], scene["trk"]
    refs = [_fresh_reference(capi, scene) for _ in range(3)]
    keep = capi.SelectionMask.from_level0(scene["m0"], LEVELS)
    want = trk.match(ref, cur, mask=keep)
    got = trk.match_batch(refs, [cur] * 3, masks=[capi.SelectionMask.from_level0(scene["m0"], LEVELS) for _ in range(3)], in_flight=1)
    assert all(cases.same_result(r, want) for r in got)
    # ... and the selections are still the pyramids': matching again with yet another mask of that content builds a new entry
    # next to them, with the same result
    assert cases.same_result(trk.match(refs[0], cur, mask=capi.SelectionMask.from_level0(scene["m0"], LEVELS)), want)


@pytest.mark.gpu
def test_a_ninth_masked_selection_is_refused_and_mismatched_masks_are_invalid(capi, scene):
    w, h = 16, 8
    rng = np.random.default_rng(5)
    I = rng.uniform(0.0, 255.0, size=(h, w)).astype(np.float32)
    Z = rng.uniform(1.0, 2.0, size=(h, w)).astype(np.float32)
    p = capi.RgbdImagePyramid(I, Z, (20.0, 20.0, 8.0, 4.0), 1)
    _, unmasked = p.select(0)
    assert unmasked.sum() > w * h // 2
    masks, outs = [], []
    for k in range(capi.MAX_MASKED_SELECTIONS):
        m0 = np.ones((h, w), np.uint8)
        m0[k % h, : 1 + k] = 0
        masks.append(capi.SelectionMask.from_level0(m0, 1))
        cnt, out = p.select(0, mask=masks[-1])
        assert np.array_equal(out, m0 & unmasked) and cnt == int(out.sum())
        outs.append(out)
    ninth = capi.SelectionMask.from_level0(np.ones((h, w), np.uint8), 1)
    with pytest.raises(capi.DvoAmdError) as e:
        p.select(0, mask=ninth)
    assert e.value.status == CAPACITY
    for m, out in zip(masks, outs):  # the eight before it select what they selected; unmasked selections are not limited
        assert np.array_equal(p.select(0, mask=m)[1], out)
    for ti in (1.0, 2.0, 3.0):
        assert p.select(0, ti, 0.5)[0] <= int(unmasked.sum())
    # other thresholds behind a cached mask are a further masked selection: refused as well, the pyramid stays as it was
    with pytest.raises(capi.DvoAmdError) as e:
        p.select(0, 1.0, 0.5, mask=masks[0])
    assert e.value.status == CAPACITY
    # a mask of another size, and one with fewer levels than the pyramid
    ref, cur, trk = scene["ref"], scene["cur"], scene["trk"]
    shallow = capi.SelectionMask.from_level0(np.ones((H, W), np.uint8), LEVELS - 2)
    for wrong in (ninth, shallow):
        with pytest.raises(capi.DvoAmdError) as e:
            ref.select(0, mask=wrong)
        assert e.value.status == INVALID_ARGUMENT and "mask" in str(e.value)
        with pytest.raises(capi.DvoAmdError) as e:
            trk.match(ref, cur, mask=wrong)
        assert e.value.status == INVALID_ARGUMENT
        with pytest.raises(capi.DvoAmdError) as e:
            trk.match_batch([ref, ref], [cur, cur], masks=[None, wrong])
        assert e.value.status == INVALID_ARGUMENT
    assert cases.same_result(trk.match(ref, cur), scene["unmasked"])  # a refused call left the tracker usable
