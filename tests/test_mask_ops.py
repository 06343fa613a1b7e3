"""Mask operations on the device (include/dvo_amd.h, "Mask operations"): dvo_amd_mask_combine, dvo_amd_mask_morph, dvo_amd_mask_warp
and dvo_amd_mask_warp_many.  The rules are pinned in the header and restated in tests/mask_ops_ref.py; every comparison in this file
is equality -- of byte planes, of integer counts, of tracking results bit for bit.  There is no tolerance anywhere.
CPU: the restatement against its pixel loop and its algebra, the warp's convention on a case whose arithmetic is exact, the
argument checks that need no device.  GPU: the library against the restatement on the planes downloaded from the pyramids."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_ops_ref as ref  # noqa: E402
import selection_mask_cases as cases  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_mask_warp_options", "dvo_amd_mask_combine", "dvo_amd_mask_morph", "dvo_amd_mask_warp",
               "dvo_amd_mask_warp_many"]
INVALID, NO_DEVICE, MISMATCH = 1, 2, 8
SIZES = {"80x48": (80, 48, 3), "72x50": (72, 50, 2), "64x32": (64, 32, 3)}
OPS = {"and": ref.AND, "or": ref.OR, "andnot": ref.ANDNOT, "not": ref.NOT}
KEEPS = [(1, 1), (1, 0), (0, 1), (0, 0)]  # (unseen_keep, inconsistent_keep)
# the kernel's tile (dvo_mask_ops.cpp): a block owns 64 columns x 64 rows, a wave 16 of the rows
TILE_X, TILE_Y, WAVE_Y = 64, 64, 16


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


# ---- CPU: the restatement -------------------------------------------------------------------------------------------------------

def _random_masks():
    rng = np.random.default_rng(5)
    sizes = [(8, 6), (9, 7), (13, 9), (16, 12), (20, 15)]
    for k in range(40):
        w, h = sizes[k % 5]
        yield k, (rng.uniform(size=(h, w)) < (0.1, 0.5, 0.9, 0.97)[k % 4]).astype(np.uint8) * (1, 255, 7)[k % 3]


def test_morph_restatement_matches_the_pixel_loop():
    for k, m in _random_masks():
        for r in (0, 1, 2, max(m.shape), max(m.shape) + 3):
            for op in (ref.DILATE, ref.ERODE):
                assert np.array_equal(ref.morph_ref(m, op, r), ref.morph_brute(m, op, r)), (k, r, op)


def test_morph_algebra_of_the_clipped_window():
    for k, m in _random_masks():
        b = (m != 0).astype(np.uint8)
        assert np.array_equal(ref.morph_ref(m, ref.DILATE, 0), b) and np.array_equal(ref.morph_ref(m, ref.ERODE, 0), b)
        for r in (1, 2, 5, 30):
            d, e = ref.morph_ref(m, ref.DILATE, r), ref.morph_ref(m, ref.ERODE, r)
            assert np.array_equal(e, 1 - ref.morph_ref(1 - b, ref.DILATE, r)), (k, r)   # pixels outside the plane have no vote
            assert (e <= b).all() and (b <= d).all(), (k, r)
        big = max(m.shape)
        assert (ref.morph_ref(m, ref.DILATE, big) == (1 if b.any() else 0)).all()          # saturated
        assert (ref.morph_ref(m, ref.ERODE, big) == (1 if b.all() else 0)).all()


def test_level_radii(capi):
    assert capi.level_radii(0, 4) == [0, 0, 0, 0]
    assert capi.level_radii(1, 4) == [1, 1, 1, 1]
    assert capi.level_radii(3, 4) == [3, 2, 1, 1]
    assert capi.level_radii(8, 4) == [8, 4, 2, 1]
    assert capi.level_radii(7, 3) == [7, 4, 2]
    assert capi.level_radii(64, 3) == [64, 32, 16]
    for r0 in range(0, 70):
        assert capi.level_radii(r0, 5) == ref.level_radii(r0, 5) == [-(-r0 // (1 << l)) for l in range(5)]


def test_warp_convention_on_an_exact_case():
    """A fronto-parallel plane at z = 2, fx = fy = 64, integer principal point, T = a translation of 3 * 2 / 64 along x: every
    product is exact.  T maps target points into the source frame, so target pixel u looks up source pixel u + 3: the mask comes
    out shifted by exactly 3 pixels towards smaller u.  The transposed or the inverted convention shifts it the other way."""
    w, h = 24, 10
    K = (64.0, 64.0, 11.0, 4.0)
    Z = np.full((h, w), 2.0, F)
    T = np.eye(4)
    T[0, 3] = 3 * 2 / 64
    ms = np.zeros((h, w), np.uint8)
    ms[2:7, 9:15] = 1
    ms[8, 23] = 1
    out, counts = ref.warp_ref(ms, (Z, K), (Z, K), T, dict(unseen_keep=0))
    want = np.zeros_like(ms)
    want[:, :w - 3] = ms[:, 3:]
    assert np.array_equal(out, want)
    assert want[2:7, 6:12].all() and want[8, 20] == 1 and want.sum() == ms.sum()
    assert counts == dict(valid=w * h, behind=0, outside=3 * h, no_depth=0, consistent=(w - 3) * h, occluded=0, seen_through=0,
                          dropped_by_source=(w - 3) * h - int(ms.sum()))
    other, _ = ref.warp_ref(ms, (Z, K), (Z, K), np.linalg.inv(T), dict(unseen_keep=0))
    back = np.zeros_like(ms)
    back[:, 3:] = ms[:, :w - 3]
    assert np.array_equal(other, back) and not np.array_equal(other, out)
    # unseen_keep decides the three columns that look past the source's edge; the verdicts that arrive are the source's
    kept, _ = ref.warp_ref(ms, (Z, K), (Z, K), T, dict(unseen_keep=1))
    assert np.array_equal(kept[:, :w - 3], want[:, :w - 3]) and kept[:, w - 3:].all()


def scene_a(synth, w, h):
    """source (at the identity) and target (at exp(4 xi)) with a patch brought 40 % nearer in each, and the source's mask:
    ((Is, Zs), (It, Zt), T, mask0).  T = pose_source^-1 pose_target maps target points into the source frame."""
    T = synth.se3_exp(4 * synth.XI_GT_PAIR)
    Is, Zs = synth.render(w, h, np.eye(4), frame_id=0, nan_fraction=0.05)
    It, Zt = synth.render(w, h, T, frame_id=1, nan_fraction=0.05)
    Zs, Zt = Zs.copy(), Zt.copy()
    Zs[h // 4:h // 2, w // 8:w // 3] *= F(0.6)
    Zt[h // 2:(3 * h) // 4, w // 2:(3 * w) // 4] *= F(0.6)
    mask0 = np.ones((h, w), np.uint8)
    mask0[h // 5:(3 * h) // 5, w // 4:(2 * w) // 3] = 0
    return (Is, Zs), (It, Zt), T, mask0


def _assert_every_outcome_but_behind(counts, what):
    for name in ("outside", "no_depth", "consistent", "occluded", "seen_through", "dropped_by_source"):
        assert counts[name] > 0, (what, name, counts)
    assert counts["behind"] == 0, (what, counts)


@pytest.mark.parametrize("name", sorted(SIZES))
def test_scene_a_produces_every_outcome_but_behind(synth, name):
    """on frames rendered at the size of every level (the device's levels are checked again on the GPU before they are compared)"""
    w, h, levels = SIZES[name]
    for l in range(levels):
        wl, hl = w >> l, h >> l
        (_, Zs), (_, Zt), T, mask0 = scene_a(synth, wl, hl)
        K = synth.intrinsics_for(wl, hl)
        _, counts = ref.warp_ref(mask0, (Zt, K), (Zs, K), T)
        _assert_every_outcome_but_behind(counts, (name, l))
        assert counts["valid"] == int(np.isfinite(Zt).sum()) == sum(counts[k] for k in ref.WARP_COUNTS[1:7])


# ---- CPU: the library's host side -----------------------------------------------------------------------------------------------

def test_the_library_exports_the_entries_and_the_binding_covers_the_headers(capi):
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
    assert (capi.MASK_AND, capi.MASK_OR, capi.MASK_ANDNOT, capi.MASK_NOT) == (ref.AND, ref.OR, ref.ANDNOT, ref.NOT) == (0, 1, 2, 3)
    assert (capi.MASK_DILATE, capi.MASK_ERODE, capi.MASK_MAX_RADIUS) == (ref.DILATE, ref.ERODE, ref.MAX_RADIUS) == (0, 1, 64)
    assert capi.MASK_WARP_COUNTS == ref.WARP_COUNTS and capi.MASK_WARP_DTYPE.itemsize == 64


def test_the_default_warp_options_are_the_documented_ones(capi):
    opt = capi.MaskWarpOptions()
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt))
    capi.lib().dvo_amd_default_mask_warp_options(C.byref(opt))
    assert (opt.near_z, opt.depth_sigmas, opt.unseen_keep, opt.inconsistent_keep) == (F(0.1), 20.0, 1, 1)
    assert C.sizeof(opt) == 16
    capi.lib().dvo_amd_default_mask_warp_options(None)  # a no-op


def _refused(L, entry, rc, handle, what):
    assert rc == INVALID, (entry, what, rc)
    assert not handle.value, (entry, what)
    reason = L.dvo_amd_last_error().decode()
    assert reason.startswith(entry + ": ") and "NULL" in reason, (entry, what, reason)


def test_null_pointers_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    something = C.create_string_buffer(4096)  # stands for a mask or a pyramid: a NULL next to it is refused before it is looked at
    p = C.c_void_p(C.addressof(something))
    radius = (C.c_int * capi.MAX_LEVELS)()
    opt = capi.mask_warp_options()
    T = (C.c_double * 16)(*np.eye(4).ravel())
    one = (C.c_void_p * 1)(p)
    null_in = (C.c_void_p * 1)(None)
    cnt = (C.c_longlong * 64)()

    def out():
        return C.c_void_p(0xDEAD)

    h = out()
    _refused(L, "dvo_amd_mask_combine", L.dvo_amd_mask_combine(None, p, capi.MASK_AND, C.byref(h)), h, "a")
    h = out()
    _refused(L, "dvo_amd_mask_combine", L.dvo_amd_mask_combine(p, None, capi.MASK_OR, C.byref(h)), h, "b")
    assert L.dvo_amd_mask_combine(p, p, capi.MASK_AND, None) == INVALID
    h = out()
    assert L.dvo_amd_mask_combine(p, p, capi.MASK_NOT, C.byref(h)) == INVALID and not h.value   # b given for NOT
    h = out()
    assert L.dvo_amd_mask_combine(p, p, 4, C.byref(h)) == INVALID and not h.value               # no such op
    for what, (m, r, with_out) in {"mask": (None, radius, True), "radius": (p, None, True), "out": (p, radius, False)}.items():
        h = out()
        rc = L.dvo_amd_mask_morph(m, capi.MASK_DILATE, r, C.byref(h) if with_out else None)
        if with_out:
            _refused(L, "dvo_amd_mask_morph", rc, h, what)
        assert rc == INVALID, what
    for what, args in {"mask": (None, p, p, T, C.byref(opt)), "source": (p, None, p, T, C.byref(opt)), "target": (p, p, None, T, C.byref(opt)),
                       "T": (p, p, p, None, C.byref(opt)), "options": (p, p, p, T, None)}.items():
        h = out()
        _refused(L, "dvo_amd_mask_warp", L.dvo_amd_mask_warp(*args, C.byref(h), cnt), h, what)
    assert L.dvo_amd_mask_warp(p, p, p, T, C.byref(opt), None, cnt) == INVALID
    for what, args in {"masks": (1, None, one, one, T, C.byref(opt)), "sources": (1, one, None, one, T, C.byref(opt)),
                       "targets": (1, one, one, None, T, C.byref(opt)), "T": (1, one, one, one, None, C.byref(opt)),
                       "options": (1, one, one, one, T, None), "masks[0]": (1, null_in, one, one, T, C.byref(opt)),
                       "sources[0]": (1, one, null_in, one, T, C.byref(opt)), "targets[0]": (1, one, one, null_in, T, C.byref(opt))}.items():
        outs = (C.c_void_p * 1)(0xDEAD)
        rc = L.dvo_amd_mask_warp_many(*args, outs, cnt)
        assert rc == INVALID and not outs[0], (what, rc)
        assert "NULL" in L.dvo_amd_last_error().decode(), what
    assert L.dvo_amd_mask_warp_many(1, one, one, one, T, C.byref(opt), None, cnt) == INVALID
    outs = (C.c_void_p * 1)(0xDEAD)
    assert L.dvo_amd_mask_warp_many(-1, one, one, one, T, C.byref(opt), outs, cnt) == INVALID
    # options and transformations are looked at before any object is
    for field, value in (("near_z", 0.0), ("near_z", float("nan")), ("near_z", float("inf")), ("depth_sigmas", -1.0),
                         ("depth_sigmas", float("nan"))):
        bad = capi.mask_warp_options(**{field: value})
        outs = (C.c_void_p * 1)(0xDEAD)
        assert L.dvo_amd_mask_warp_many(0, one, one, one, T, C.byref(bad), outs, cnt) == INVALID, (field, value)
    if L.dvo_amd_device_count() == 0:
        # nothing left to refuse: the device is looked for.  The zeroed buffer reads as a mask without levels.
        h = out()
        assert L.dvo_amd_mask_combine(p, p, capi.MASK_AND, C.byref(h)) == NO_DEVICE and not h.value
        h = out()
        assert L.dvo_amd_mask_combine(p, None, capi.MASK_NOT, C.byref(h)) == NO_DEVICE and not h.value
        h = out()
        assert L.dvo_amd_mask_morph(p, capi.MASK_ERODE, radius, C.byref(h)) == NO_DEVICE and not h.value
        outs = (C.c_void_p * 1)(0xDEAD)
        assert L.dvo_amd_mask_warp_many(0, one, one, one, T, C.byref(opt), outs, cnt) == NO_DEVICE


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


def _planes(mask):
    return [mask.download(l) for l in range(mask.info()["levels"])]


def _same(mask, want, what):
    """the mask's planes and kept counts are the restated ones"""
    info = mask.info()
    assert info["levels"] == len(want), what
    for l, p in enumerate(want):
        got = mask.download(l)
        assert got.shape == p.shape and np.array_equal(got, p), (what, l)
    assert info["kept"] == [int(p.sum()) for p in want], what


def _status(capi, call):
    with pytest.raises(capi.DvoAmdError) as err:
        call()
    return err.value.status


def _random_level0(w, h, seed, p=0.5):
    rng = np.random.default_rng(seed)
    return (rng.uniform(size=(h, w)) < p).astype(np.uint8) * rng.choice(np.array([1, 2, 128, 255], np.uint8), size=(h, w))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIZES))
def test_combine_equals_numpy(gpu, name):
    w, h, levels = SIZES[name]
    a0, b0 = cases.level0_mask(w, h), _random_level0(w, h, 3)
    assert a0.max() > 1 and b0.max() > 1  # keep bytes other than 1
    for rule in (gpu.MASK_ALL, gpu.MASK_ANY):
        A, B = gpu.SelectionMask.from_level0(a0, levels, rule), gpu.SelectionMask.from_level0(b0, levels, rule)
        pa, pb = cases.mask_pyramid(a0, levels, rule == gpu.MASK_ANY), cases.mask_pyramid(b0, levels, rule == gpu.MASK_ANY)
        _same(A & B, [ref.combine_ref(x, y, ref.AND) for x, y in zip(pa, pb)], (name, rule, "and"))
        _same(A | B, [ref.combine_ref(x, y, ref.OR) for x, y in zip(pa, pb)], (name, rule, "or"))
        _same(A.andnot(B), [ref.combine_ref(x, y, ref.ANDNOT) for x, y in zip(pa, pb)], (name, rule, "andnot"))
        _same(B.andnot(A), [ref.combine_ref(y, x, ref.ANDNOT) for x, y in zip(pa, pb)], (name, rule, "andnot, swapped"))
        _same(~A, [ref.combine_ref(x, None, ref.NOT) for x in pa], (name, rule, "not"))
        _same(A & ~A, [np.zeros_like(x) for x in pa], (name, rule, "empty"))
        _same(A | ~A, [np.ones_like(x) for x in pa], (name, rule, "full"))
        _same(A, pa, "the inputs are only read")
    # every level given on its own, with keep bytes other than 1
    la = [_random_level0(w >> l, h >> l, 10 + l, 0.7) for l in range(levels)]
    lb = [_random_level0(w >> l, h >> l, 20 + l, 0.3) for l in range(levels)]
    A, B = gpu.SelectionMask.from_levels(la), gpu.SelectionMask.from_levels(lb)
    for op_name, op in OPS.items():
        got = ~A if op == ref.NOT else {ref.AND: A & B, ref.OR: A | B, ref.ANDNOT: A.andnot(B)}[op]
        _same(got, [ref.combine_ref(x, None if op == ref.NOT else y, op) for x, y in zip(la, lb)], (name, "levels", op_name))


@pytest.mark.gpu
def test_combine_refuses_masks_that_do_not_match(gpu):
    L = gpu.lib()
    a = gpu.SelectionMask.from_level0(np.ones((48, 80), np.uint8), 3)
    shallow = gpu.SelectionMask.from_level0(np.ones((48, 80), np.uint8), 2)
    other = gpu.SelectionMask.from_level0(np.ones((32, 64), np.uint8), 3)
    for what, b in (("levels", shallow), ("size", other)):
        for x, y in ((a, b), (b, a)):
            h = C.c_void_p(0xDEAD)
            assert L.dvo_amd_mask_combine(x._h, y._h, gpu.MASK_AND, C.byref(h)) == INVALID and not h.value, what
            assert L.dvo_amd_last_error().decode().startswith("dvo_amd_mask_combine: "), what
    assert _status(gpu, lambda: a & shallow) == INVALID
    h = C.c_void_p(0xDEAD)
    assert L.dvo_amd_mask_combine(a._h, a._h, gpu.MASK_NOT, C.byref(h)) == INVALID and not h.value
    assert L.dvo_amd_mask_combine(a._h, None, gpu.MASK_AND, C.byref(h)) == INVALID and not h.value
    assert L.dvo_amd_mask_combine(a._h, a._h, 7, C.byref(h)) == INVALID and not h.value
    if L.dvo_amd_device_count() > 1:
        elsewhere = gpu.SelectionMask.from_level0(np.ones((48, 80), np.uint8), 3, device=1)
        assert L.dvo_amd_mask_combine(a._h, elsewhere._h, gpu.MASK_AND, C.byref(h)) == MISMATCH and not h.value


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIZES))
def test_morph_equals_numpy(gpu, name):
    w, h, levels = SIZES[name]
    planes = cases.mask_pyramid(cases.level0_mask(w, h), levels, False)
    planes[-1] = _random_level0(w >> (levels - 1), h >> (levels - 1), 4, 0.2)  # (levels given on their own: any content)
    M = gpu.SelectionMask.from_levels(planes)
    norm = [(p != 0).astype(np.uint8) for p in planes]
    for r0 in (0, 1, 2, 7, 64):
        radii = gpu.level_radii(r0, levels)
        for op, morph in ((ref.DILATE, M.dilate), (ref.ERODE, M.erode)):
            _same(morph(r0), [ref.morph_ref(p, op, r) for p, r in zip(norm, radii)], (name, r0, op))
    _same(M.dilate(0), norm, "radius 0 copies")
    # (64 saturates the small levels: every level of these frames but level 0 of 80x48 and 72x50 lies within 64 of any pixel)
    assert all((ref.morph_ref(p, ref.DILATE, r) == 1).all() for p, r in list(zip(norm, gpu.level_radii(64, levels)))[1:])
    per_level = [2, 0, 5][:levels]
    _same(M.dilate(per_level), [ref.morph_ref(p, ref.DILATE, r) for p, r in zip(norm, per_level)], (name, "per level"))
    _same(M.erode(per_level[::-1]), [ref.morph_ref(p, ref.ERODE, r) for p, r in zip(norm, per_level[::-1])], (name, "per level"))
    _same(M, norm, "the input is only read")


def _tile_border_mask(w, h, kept):
    """isolated pixels (kept on a dropped plane, or dropped on a kept one) at the four corners, on the last row and the last
    column, and on both sides of every border between the kernel's tiles (columns at multiples of 64, rows at multiples of 16)"""
    m = np.zeros((h, w), np.uint8)
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h - 1, w // 3), (h // 3, w - 1)]
    for i, bx in enumerate(range(TILE_X, w, TILE_X)):
        spots += [((11 + 29 * i) % h, bx - 1), ((40 + 29 * i) % h, bx)]
    for i, by in enumerate(range(WAVE_Y, h, WAVE_Y)):
        spots += [(by - 1, (17 + 23 * i) % w), (by, (30 + 23 * i) % w)]
    for y, x in spots:
        m[y, x] = 1
    return m if kept else 1 - m


@pytest.mark.gpu
def test_morph_across_the_kernel_tiles(gpu):
    """208x208, not the 208x80 of a first sketch: a block's tile is 64x64 and its halo the radius, up to 64 on each side, so only a
    plane of more than 192 rows and columns holds a tile, its whole halo and pixels beyond both"""
    w = h = 208
    assert w > TILE_X + 2 * ref.MAX_RADIUS and h > TILE_Y + 2 * ref.MAX_RADIUS
    levels = 3
    for kept in (True, False):
        planes = [_tile_border_mask(w >> l, h >> l, kept) for l in range(levels)]
        M = gpu.SelectionMask.from_levels(planes)
        for radii in ([1, 1, 1], [7, 3, 2], [64, 63, 33], [0, 64, 1]):
            for op, morph in ((ref.DILATE, M.dilate), (ref.ERODE, M.erode)):
                _same(morph(radii), [ref.morph_ref(p, op, r) for p, r in zip(planes, radii)], (kept, radii, op))


@pytest.mark.gpu
def test_morph_refuses_radii_outside_the_range(gpu):
    L = gpu.lib()
    M = gpu.SelectionMask.from_level0(np.ones((48, 80), np.uint8), 3)
    for radii, ok in (([-1, 0, 0], False), ([0, 0, 65], False), ([65, 0, 0], False), ([0, 0, 0, -1, 65], True), ([64, 64, 64], True)):
        arr = (C.c_int * 8)(*radii)
        for op in (gpu.MASK_DILATE, gpu.MASK_ERODE):
            h = C.c_void_p(0xDEAD)
            rc = L.dvo_amd_mask_morph(M._h, op, arr, C.byref(h))
            if ok:  # entries beyond the mask's levels are not read
                assert rc == 0 and h.value, radii
                L.dvo_amd_mask_release(h)
            else:
                assert rc == INVALID and not h.value, radii
                assert L.dvo_amd_last_error().decode().startswith("dvo_amd_mask_morph: "), radii
    assert _status(gpu, lambda: M.dilate(-1)) == INVALID and _status(gpu, lambda: M.erode(65)) == INVALID
    h = C.c_void_p(0xDEAD)
    assert L.dvo_amd_mask_morph(M._h, 2, (C.c_int * 8)(), C.byref(h)) == INVALID and not h.value


class WarpScene:
    """scene A at one size: the pyramids, the source's mask, and what the library reads -- the depth plane and the intrinsics of
    every level, downloaded"""

    def __init__(self, capi, synth, name):
        self.w, self.h, self.levels = SIZES[name]
        (Is, Zs), (It, Zt), self.T, self.mask0 = scene_a(synth, self.w, self.h)
        K = synth.intrinsics_for(self.w, self.h)
        self.source = capi.RgbdImagePyramid(Is, Zs, K, self.levels)
        self.target = capi.RgbdImagePyramid(It, Zt, K, self.levels)
        self.mask = capi.SelectionMask.from_level0(self.mask0, self.levels)
        self.mask_planes = cases.mask_pyramid(self.mask0, self.levels, False)
        self.ps = [(self.source.plane(l, 1), tuple(self.source.level_info(l)[2])) for l in range(self.levels)]
        self.pt = [(self.target.plane(l, 1), tuple(self.target.level_info(l)[2])) for l in range(self.levels)]
        self._ref = {}

    def ref(self, **opt):
        """the restated (planes, counts) of every level (computed once per option set, shared)"""
        key = tuple(sorted(opt.items()))
        if key not in self._ref:
            self._ref[key] = [ref.warp_ref(self.mask_planes[l], self.pt[l], self.ps[l], self.T, opt) for l in range(self.levels)]
        return self._ref[key]


@pytest.fixture(scope="module")
def warp_scenes(gpu, synth):
    return {name: WarpScene(gpu, synth, name) for name in SIZES}


def _counts(records):
    return [{k: int(r[k]) for k in ref.WARP_COUNTS} for r in records]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIZES))
def test_warp_equals_the_restatement_on_every_level(gpu, warp_scenes, name):
    from dvo_slam_amd import constraints as Cn

    s = warp_scenes[name]
    for l, (_, counts) in enumerate(s.ref()):
        _assert_every_outcome_but_behind(counts, (name, l))  # ... on the real level planes, before anything is compared
    tracker = gpu.DenseTracker()
    keyframes = [Cn.Keyframe(0, s.target, s.T, None), Cn.Keyframe(2, s.source, np.eye(4), None)]
    for unseen, inconsistent in KEEPS:
        for extra in (dict(), dict(near_z=2.5, depth_sigmas=0.5)):
            opt = dict(unseen_keep=unseen, inconsistent_keep=inconsistent, **extra)
            want = s.ref(**opt)
            got, counts = s.mask.warp(s.source, s.target, s.T, counts=True, **opt)
            _same(got, [p for p, _ in want], (name, opt))
            assert _counts(counts) == [c for _, c in want], (name, opt)
            for l in range(s.levels):
                covis = gpu.covisibility(tracker, keyframes, [(0, 1)], level=l, **extra)[0]
                assert [int(covis[k]) for k in ref.WARP_COUNTS[:7]] == [int(counts[l][k]) for k in ref.WARP_COUNTS[:7]], (name, opt, l)
    planes = {k: [p for p, _ in s.ref(unseen_keep=k[0], inconsistent_keep=k[1])] for k in KEEPS}
    assert all(not np.array_equal(planes[KEEPS[0]][0], planes[k][0]) for k in KEEPS[1:])  # each switch decides some pixel
    assert s.mask.warp(s.source, s.target, s.T).info()["kept"] == [int(p.sum()) for p in planes[(1, 1)]]  # counts=False: the mask alone


@pytest.mark.gpu
def test_warp_behind_and_far_away(gpu, warp_scenes, synth):
    s = warp_scenes["80x48"]
    # scene B: a half turn about y -- every pixel with depth lands behind the source camera
    turn = synth.se3_exp([0, 0, 0, 0, np.pi, 0])
    for unseen in (0, 1):
        got, counts = s.mask.warp(s.source, s.target, turn, counts=True, unseen_keep=unseen, inconsistent_keep=1 - unseen)
        want = [ref.warp_ref(s.mask_planes[l], s.pt[l], s.ps[l], turn, dict(unseen_keep=unseen, inconsistent_keep=1 - unseen))
                for l in range(s.levels)]
        assert _counts(counts) == [c for _, c in want]
        for l, c in enumerate(_counts(counts)):
            assert c["behind"] == c["valid"] == int(np.isfinite(s.pt[l][0]).sum()) > 0
            assert (got.download(l) == unseen).all()
    # a translation of 1e30 across the view, or backwards along it: the projections are far beyond any int (the range is tested
    # in float), or the point is behind
    for axis, sign in ((0, 1.0), (0, -1.0), (1, 1.0), (1, -1.0), (2, -1.0)):
        far = np.eye(4)
        far[axis, 3] = sign * 1e30
        got, counts = s.mask.warp(s.source, s.target, far, counts=True, unseen_keep=0)
        want = [ref.warp_ref(s.mask_planes[l], s.pt[l], s.ps[l], far, dict(unseen_keep=0)) for l in range(s.levels)]
        assert _counts(counts) == [c for _, c in want], (axis, sign)
        for l, c in enumerate(_counts(counts)):
            assert c["valid"] > 0 and (c["behind"] if axis == 2 else c["outside"]) == c["valid"], (axis, sign, l)
            assert not got.download(l).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIZES))
def test_the_identity_warp_returns_the_mask_where_there_is_depth(gpu, warp_scenes, name):
    s = warp_scenes[name]
    got, counts = s.mask.warp(s.source, s.source, np.eye(4), counts=True, unseen_keep=0)
    for l in range(s.levels):
        has_depth = np.isfinite(s.ps[l][0])
        assert np.array_equal(got.download(l), s.mask_planes[l] * has_depth), l
        c = _counts(counts)[l]
        assert c["consistent"] == c["valid"] == int(has_depth.sum())
        assert c["dropped_by_source"] == int((has_depth & (s.mask_planes[l] == 0)).sum())


@pytest.mark.gpu
def test_warp_between_frames_of_different_sizes(gpu, warp_scenes):
    """the target's own rays and size, the source's size and intrinsics; the target's level count"""
    a, b = warp_scenes["80x48"], warp_scenes["72x50"]
    got, counts = a.mask.warp(a.source, b.target, b.T, counts=True, inconsistent_keep=0)   # 3-level source, 2-level target
    want = [ref.warp_ref(a.mask_planes[l], b.pt[l], a.ps[l], b.T, dict(inconsistent_keep=0)) for l in range(b.levels)]
    _same(got, [p for p, _ in want], "80x48 -> 72x50")
    assert got.info()["width"] == 72 and got.info()["height"] == 50 and got.info()["levels"] == 2
    assert _counts(counts) == [c for _, c in want] and sum(c["consistent"] for _, c in want) > 1000
    c = warp_scenes["64x32"]
    got, counts = c.mask.warp(c.source, a.target, a.T, counts=True)                         # both of 3 levels
    want = [ref.warp_ref(c.mask_planes[l], a.pt[l], c.ps[l], a.T) for l in range(3)]
    _same(got, [p for p, _ in want], "64x32 -> 80x48")
    assert _counts(counts) == [c for _, c in want]


@pytest.mark.gpu
def test_warp_many_equals_single_calls(gpu, warp_scenes, synth):
    a, b, c = warp_scenes["80x48"], warp_scenes["72x50"], warp_scenes["64x32"]
    other = gpu.SelectionMask.from_level0(cases.level0_mask(80, 48), 3, gpu.MASK_ANY)
    pairs = [(a.mask, a.source, a.target, a.T), (b.mask, b.source, b.target, b.T), (other, a.source, a.target, np.eye(4)),
             (c.mask, c.source, a.target, a.T), (a.mask, a.source, b.target, synth.se3_exp(2 * synth.XI_GT_PAIR))]
    opt = dict(inconsistent_keep=0)
    single = [m.warp(s, t, T, counts=True, **opt) for m, s, t, T in pairs]
    for order in (list(range(5)), [4, 2, 0, 3, 1], list(range(5))):
        masks, counts = gpu.SelectionMask.warp_many(*[[pairs[k][i] for k in order] for i in range(4)], counts=True, **opt)
        assert len(masks) == len(counts) == 5
        for at, k in enumerate(order):
            _same(masks[at], _planes(single[k][0]), (order, k))
            assert masks[at].info() == single[k][0].info()
            assert _counts(counts[at]) == _counts(single[k][1]), (order, k)
    assert gpu.SelectionMask.warp_many([], [], [], []) == []


@pytest.mark.gpu
def test_warp_refuses_what_does_not_fit(gpu, warp_scenes):
    L = gpu.lib()
    a, b = warp_scenes["80x48"], warp_scenes["72x50"]

    def raw(mask, source, target, T, **options):
        opt = gpu.mask_warp_options(**options)
        h = C.c_void_p(0xDEAD)
        Tc = np.ascontiguousarray(np.asarray(T, np.float64).T)
        rc = L.dvo_amd_mask_warp(mask._h, source._h, target._h, Tc.ctypes.data_as(C.POINTER(C.c_double)), C.byref(opt), C.byref(h), None)
        assert rc == 0 or not h.value
        if rc == 0:
            L.dvo_amd_mask_release(h)
        return rc

    assert raw(a.mask, a.source, a.target, a.T) == 0                                   # (counts may be NULL)
    assert raw(b.mask, b.source, a.target, a.T) == INVALID                             # a target with more levels than the source
    assert "levels" in L.dvo_amd_last_error().decode()
    assert raw(b.mask, a.source, a.target, a.T) == INVALID                             # a mask of another size than the source
    shallow = gpu.SelectionMask.from_level0(a.mask0, 2)
    assert raw(shallow, a.source, a.target, a.T) == INVALID                            # ... or with fewer levels
    for bad in (np.nan, np.inf, -np.inf):
        for at in ((0, 0), (1, 3), (3, 3), (3, 0)):
            T = np.array(a.T)
            T[at] = bad
            assert raw(a.mask, a.source, a.target, T) == INVALID, (bad, at)
    for options in (dict(near_z=0.0), dict(near_z=-1.0), dict(near_z=np.nan), dict(near_z=np.inf), dict(depth_sigmas=-0.5),
                    dict(depth_sigmas=np.nan), dict(depth_sigmas=np.inf)):
        assert raw(a.mask, a.source, a.target, a.T, **options) == INVALID, options
        assert L.dvo_amd_last_error().decode().startswith("dvo_amd_mask_warp: "), options
    assert raw(a.mask, a.source, a.target, a.T, depth_sigmas=0.0) == 0
    assert _status(gpu, lambda: b.mask.warp(b.source, a.target, a.T)) == INVALID
    # one bad pair refuses the whole call, and every output stays NULL
    assert _status(gpu, lambda: gpu.SelectionMask.warp_many([a.mask, b.mask], [a.source, a.source], [a.target, a.target], [a.T, a.T])) == INVALID


@pytest.fixture(scope="module")
def chain(gpu, synth):
    """three frames of a short stream at 160x120 and the tracker the chain of examples/mask_ops_example.c runs with"""
    w, h, levels = 160, 120, 4
    K = synth.intrinsics_for(w, h)
    frames = [synth.render(w, h, synth.se3_exp(0.5 * k * synth.XI_GT_PAIR), frame_id=k) for k in range(3)]
    pyramids = [gpu.RgbdImagePyramid(I, Z, K, levels) for I, Z in frames]
    cfg = gpu.Config(FirstLevel=levels - 1, LastLevel=0)
    return dict(w=w, h=h, levels=levels, K=K, frames=frames, pyramids=pyramids, tracker=gpu.DenseTracker(cfg), cfg=cfg)


def rectangle(w, h):
    """the region of interest of the examples: the middle of the keyframe"""
    m = np.zeros((h, w), np.uint8)
    m[h // 4:(3 * h) // 4, w // 4:(3 * w) // 4] = 1
    return m


@pytest.mark.gpu
def test_the_results_are_ordinary_masks(gpu, chain):
    """a rectangle on the keyframe, warped to the next frame with the pose a match returned, eroded by 1, ANDed with a GRID
    budget: the match behind it is the match behind the restated planes uploaded from the host, bit for bit"""
    kf, f1, f2 = chain["pyramids"]
    trk, levels = chain["tracker"], chain["levels"]
    thresholds = (chain["cfg"].IntensityDerivativeThreshold, chain["cfg"].DepthDerivativeThreshold)
    T1 = trk.match(kf, f1).Transformation
    rect0 = rectangle(chain["w"], chain["h"])
    rect = gpu.SelectionMask.from_level0(rect0, levels)
    budget = gpu.SelectionMask.from_budget(f1, gpu.BUDGET_GRID, cell=3, thresholds=thresholds)
    warped = rect.warp(kf, f1, T1)
    combined = warped.erode(1) & budget
    # the restatement, from the planes the library reads
    rect_planes = cases.mask_pyramid(rect0, levels, False)
    radii = ref.level_radii(1, levels)
    want = []
    for l in range(levels):
        pt, ps = (f1.plane(l, 1), tuple(f1.level_info(l)[2])), (kf.plane(l, 1), tuple(kf.level_info(l)[2]))
        w_l, _ = ref.warp_ref(rect_planes[l], pt, ps, T1)
        want.append(ref.combine_ref(ref.morph_ref(w_l, ref.ERODE, radii[l]), budget.download(l), ref.AND))
    assert all(0 < int(p.sum()) < int(budget.download(l).sum()) for l, p in enumerate(want))
    _same(combined, want, "chain")
    kept = combined.info()["kept"]
    del rect, budget, warped  # the inputs may go before the result is used
    got = trk.match(f1, f2, mask=combined)
    uploaded = gpu.SelectionMask.from_levels(want)
    assert cases.same_result(got, trk.match(f1, f2, mask=uploaded))
    assert not got.isNaN() and not cases.same_result(got, trk.match(f1, f2))
    assert combined.info()["kept"] == kept == [int(p.sum()) for p in want]


@pytest.mark.gpu
def test_device_time_is_reported_when_asked_for(gpu, warp_scenes):
    s = warp_scenes["80x48"]
    gpu.mask_ops_timing(True)
    try:
        for call in (lambda: s.mask & s.mask, lambda: s.mask.dilate(2), lambda: s.mask.warp(s.source, s.target, s.T)):
            call()
            assert 0.0 < gpu.mask_ops_timing(True) < 1000.0
    finally:
        gpu.mask_ops_timing(False)
