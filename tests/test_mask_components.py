"""Connected components of masks and depth on the device (include/dvo_amd.h, "Mask components"): dvo_amd_mask_filter_components,
dvo_amd_mask_filter_components_many and dvo_amd_mask_components.  The rules are pinned in the header and restated in
tests/mask_components_ref.py; every comparison in this file is equality -- of byte planes, int32 label planes, integer records and
counts, of tracking results bit for bit.  There is no tolerance anywhere.
CPU: the restatement against scipy.ndimage.label and against a pixel loop, its algebra, the depth rule on the sensor frames, the
host check of the union-find (tests/host/components_host_check.cpp, built with the address and undefined-behaviour sanitizers), the
argument checks that need no device.  GPU: the library against the restatement on the planes downloaded from the pyramids."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_components_ref as ref  # noqa: E402
import mask_ops_ref as ops_ref  # noqa: E402
import selection_mask_cases as cases  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_component_options", "dvo_amd_mask_filter_components", "dvo_amd_mask_filter_components_many",
               "dvo_amd_mask_components", "dvo_amd_debug_components_timing"]
INVALID, NO_DEVICE, MISMATCH = 1, 2, 8
SIZES = {"80x48": (80, 48, 3), "72x50": (72, 50, 2), "136x72": (136, 72, 2), "200x136": (200, 136, 1)}
# the kernel's tile (dvo_components.cpp): a block owns 64 columns x 64 rows and labels them in LDS (a thread 16 rows of a column).
# Level 0 of every size above is no multiple of it; 136x72 and 200x136 span at least three tiles across and two down.
TILE = 64


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


# ---- patterns -------------------------------------------------------------------------------------------------------------------

def _random(w, h, p, seed):
    return (np.random.default_rng(seed).uniform(size=(h, w)) < p).astype(np.uint8)


def _corners(w, h):
    m = np.zeros((h, w), np.uint8)
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = 1
    return m


def _checkerboard(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((x + y) % 2 == 0).astype(np.uint8)


def _spiral(w, h):
    """a one-pixel-wide path that winds inwards, a one-pixel gap between its turns"""
    m = np.zeros((h, w), np.uint8)
    x0, y0, x1, y1 = 0, 0, w - 1, h - 1
    m[0, :] = 1
    while x1 - x0 >= 2 and y1 - y0 >= 2:
        m[y0:y1 + 1, x1] = 1                    # down the right side
        m[y1, x0:x1 + 1] = 1                    # along the bottom
        if y1 - (y0 + 2) < 0:
            break
        m[y0 + 2:y1 + 1, x0] = 1                # up the left side, to two rows below the top
        x1 -= 2
        if x1 - x0 < 2:
            break
        m[y0 + 2, x0:x1 + 1] = 1                # the next turn's top
        x0, y0, y1 = x0 + 2, y0 + 2, y1 - 2
    return m


def _serpentine(w, h):
    """every other row, joined alternately at the right and at the left end: one path through the whole plane"""
    m = np.zeros((h, w), np.uint8)
    m[0::2, :] = 1
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def _comb(w, h):
    """teeth that join only in the last row"""
    m = np.zeros((h, w), np.uint8)
    m[:, 0::2] = 1
    m[h - 1, :] = 1
    return m


def _u_shape(w, h):
    """two arms in different tiles that join in a third: their provisional roots merge late"""
    m = np.zeros((h, w), np.uint8)
    m[1:h - 1, 3] = 1
    m[1:h - 1, w - 4] = 1
    m[h - 2, 3:w - 3] = 1
    return m


def _late_roots(w, h):
    """components whose smallest index lies in the last tile they touch: an anti-diagonal staircase that starts at the top right and
    ends at the bottom left, and a hook whose stem stands at the right edge and whose foot runs left along the bottom"""
    m = np.zeros((h, w), np.uint8)
    n = min(w - 6, h - 4)
    for k in range(n):
        m[k, w - 6 - k] = 1
        m[k, w - 7 - k] = 1      # (4-connected as well)
    m[2:h, w - 1] = 1
    m[h - 1, w // 2:w] = 1
    return m


def _frame(w, h):
    m = np.zeros((h, w), np.uint8)
    m[0, :] = m[h - 1, :] = 1
    m[:, 0] = m[:, w - 1] = 1
    return m


def _blocks(w, h):
    """3 x 3 blocks on a pitch of 5: many components of equal area, for the ties of keep_largest; one larger and one smaller one"""
    m = np.zeros((h, w), np.uint8)
    for y in range(1, h - 3, 5):
        for x in range(1, w - 3, 5):
            m[y:y + 3, x:x + 3] = 1
    m[1:4, 1:9] = 1      # the first two blocks joined: the largest
    m[h - 1, w - 1] = 1  # a single pixel
    return m


PATTERNS = {
    "zeros": lambda w, h: np.zeros((h, w), np.uint8),
    "ones": lambda w, h: np.ones((h, w), np.uint8),
    "corners": _corners,
    "checkerboard": _checkerboard,
    "random 0.3": lambda w, h: _random(w, h, 0.3, 11),
    "random 0.5": lambda w, h: _random(w, h, 0.5, 12),
    "random 0.6": lambda w, h: _random(w, h, 0.6, 13),
    "random 0.9": lambda w, h: _random(w, h, 0.9, 14),
    "spiral": _spiral,
    "serpentine": _serpentine,
    "comb": _comb,
    "u": _u_shape,
    "late roots": _late_roots,
    "frame": _frame,
    "blocks": _blocks,
}


def _levels_of(pattern, w, h, levels):
    """the pattern drawn on every level at that level's size, with keep bytes other than 1 on level 0"""
    planes = [PATTERNS[pattern](w >> l, h >> l) for l in range(levels)]
    planes[0] = planes[0] * np.uint8(255)
    return planes


# ---- CPU: the restatement -------------------------------------------------------------------------------------------------------

def _canonical_from_scipy(mask, connectivity):
    from scipy import ndimage

    numbered, n = ndimage.label(mask != 0, structure=np.ones((3, 3), int) if connectivity == 8 else None)
    out = np.zeros(mask.shape, np.int32)
    flat = numbered.ravel()
    for k in range(1, n + 1):
        where = np.flatnonzero(flat == k)
        out.ravel()[where] = where[0] + 1
    return out, n


def test_the_restatement_equals_scipy_ndimage_label_without_depth():
    rng = np.random.default_rng(7)
    for k in range(40):
        m = (rng.uniform(size=(37, 52)) < (0.3, 0.4, 0.5, 0.6, 0.7, 0.8)[k % 6]).astype(np.uint8) * (1, 255, 7)[k % 3]
        for connectivity in (4, 8):
            want, n = _canonical_from_scipy(m, connectivity)
            got, cut = ref.label(m, None, connectivity)
            assert np.array_equal(got, want) and cut == 0, (k, connectivity)
            recs = ref.records(got)
            assert len(recs) == n and int(recs["area"].sum()) == int((m != 0).sum())
    for name, make in PATTERNS.items():
        m = make(52, 37)
        for connectivity in (4, 8):
            assert np.array_equal(ref.label(m, None, connectivity)[0], _canonical_from_scipy(m, connectivity)[0]), (name, connectivity)


def test_the_patterns_are_what_they_are_meant_to_be():
    for w, h in ((52, 37), (200, 136), (136, 72), (40, 24)):
        n8 = {name: len(ref.records(ref.label(make(w, h), None, 8)[0])) for name, make in PATTERNS.items()}
        n4 = {name: len(ref.records(ref.label(make(w, h), None, 4)[0])) for name, make in PATTERNS.items()}
        assert n8["zeros"] == 0 and n8["ones"] == 1 and n8["corners"] == n4["corners"] == 4
        assert n8["checkerboard"] == 1 and n4["checkerboard"] == int(_checkerboard(w, h).sum())
        for one in ("spiral", "serpentine", "comb", "u", "frame"):
            assert n8[one] == n4[one] == 1, (one, w, h)
        assert n8["late roots"] == n4["late roots"] == 2
        # thin: a path, not a filled plane
        assert _spiral(w, h).sum() < 0.62 * w * h and _serpentine(w, h).sum() < 0.6 * w * h
        areas = ref.records(ref.label(_blocks(w, h), None, 8)[0])["area"]
        assert (areas == 9).sum() >= 8 and areas.max() == 24 and areas.min() == 1


def _depth_cases():
    rng = np.random.default_rng(9)
    for k in range(30):
        w, h = ((20, 15), (13, 9), (8, 6))[k % 3]
        Z = (F(1.0) + F(0.05) * rng.integers(0, 4, size=(h, w)).astype(F) + rng.uniform(0, 0.02, size=(h, w)).astype(F)).astype(F)
        Z[rng.uniform(size=(h, w)) < 0.1] = np.nan
        m = None if k % 2 else (rng.uniform(size=(h, w)) < 0.8).astype(np.uint8)
        yield k, m, Z, dict(connectivity=(4, 8)[k % 2], max_step=(0.0, 0.01)[k % 2], depth_sigmas=(10.0, 3.0, 0.0)[k % 3])


def test_the_restatement_equals_a_pixel_loop_with_depth():
    some_cut = some_merged = 0
    for k, m, Z, opt in _depth_cases():
        got, cut = ref.label(m, Z, **opt)
        want, cut_loop = ref.label_loop(m, Z, **opt)
        assert np.array_equal(got, want) and cut == cut_loop, k
        assert np.array_equal(got > 0, ref.foreground(m, Z))
        some_cut += cut > 0
        some_merged += len(ref.records(got)) < int((got > 0).sum())
    assert some_cut > 10 and some_merged > 10


def test_algebra_of_the_filter():
    rng = np.random.default_rng(3)
    for k in range(12):
        m = (rng.uniform(size=(37, 52)) < (0.45, 0.6, 0.75)[k % 3]).astype(np.uint8)
        fg = (m != 0).astype(np.uint8)
        for connectivity in (4, 8):
            out, counts = ref.filter_components(m, connectivity=connectivity)
            assert np.array_equal(out, fg) and counts["kept_pixels"] == counts["foreground"] == int(fg.sum())
            assert counts["kept_components"] == counts["components"] and counts["edges_cut"] == 0
            for a in (1, 2, 5, 40):
                big, _ = ref.filter_components(m, connectivity=connectivity, min_area=a)
                small, _ = ref.filter_components(m, connectivity=connectivity, max_area=a - 1)
                assert not (big & small).any() and np.array_equal(big | small, fg), (k, a)
            labels, _ = ref.label(m, None, connectivity)
            for r in (1, 2):
                eroded = ops_ref.morph_ref(m, ops_ref.ERODE, r)
                rec, _ = ref.filter_components(m, seeds=eroded, connectivity=connectivity)
                assert (rec <= fg).all() and (eroded <= rec).all()
                kept_labels = np.unique(labels[rec != 0])
                assert np.array_equal(rec != 0, np.isin(labels, kept_labels) & (labels > 0))  # whole components of m
            recs = ref.records(labels)
            for largest in (1, 3, 8):
                out, counts = ref.filter_components(m, connectivity=connectivity, keep_largest=largest)
                assert counts["kept_components"] == min(largest, len(recs))
                order = sorted(recs, key=lambda c: (-int(c["area"]), int(c["root"])))[:largest]
                assert counts["kept_pixels"] == sum(int(c["area"]) for c in order)
                assert all(out.ravel()[int(c["root"])] for c in order)
        # 4-connected components refine 8-connected ones
        l4, l8 = ref.label(m, None, 4)[0], ref.label(m, None, 8)[0]
        assert len(np.unique(np.stack([l4.ravel(), l8.ravel()]), axis=1).T) == len(np.unique(l4))
    # ties go to the lower root
    blocks = _blocks(52, 37)
    recs = ref.records(ref.label(blocks, None, 8)[0])
    out, counts = ref.filter_components(blocks, keep_largest=3)
    nines = [int(c["root"]) for c in recs if c["area"] == 9]
    assert counts["kept_components"] == 3 and counts["kept_pixels"] == 24 + 9 + 9 and counts["largest_area"] == 24
    assert out.ravel()[nines[0]] and out.ravel()[nines[1]] and not out.ravel()[nines[2]]


@pytest.mark.parametrize("size,valid", [((160, 120), 18724), ((80, 60), 4713)])
def test_the_depth_rule_on_the_sensor_frames(synth, size, valid):
    """with the defaults the smooth room is one component that covers every valid pixel; a 3 x 3 block pasted 40 % nearer is a
    component of its own, and min_area = 10 drops it and nothing else"""
    w, h = size
    _, Z = synth.raw_to_float(*synth.sensor_frame(w, h))
    labels, _ = ref.label(None, Z)
    recs = ref.records(labels)
    assert len(recs) == 1 and int(recs["area"][0]) == valid == int(np.isfinite(Z).sum())
    pasted = Z.copy()
    pasted[30:33, 40:43] *= F(0.6)
    assert np.isfinite(pasted[30:33, 40:43]).all()
    recs = ref.records(ref.label(None, pasted)[0])
    assert [int(a) for a in recs["area"]] == [valid - 9, 9]
    assert (int(recs["x0"][1]), int(recs["y0"][1]), int(recs["x1"][1]), int(recs["y1"][1])) == (40, 30, 42, 32)
    out, counts = ref.filter_components(None, pasted, min_area=10)
    want = np.isfinite(pasted).astype(np.uint8)
    want[30:33, 40:43] = 0
    assert np.array_equal(out, want)
    _, cut = ref.label_loop(None, pasted[20:40, 30:50])
    assert ref.label(None, pasted[20:40, 30:50])[1] == cut > 0
    assert counts["edges_cut"] == ref.label(None, pasted)[1] >= cut and counts["components"] == 2 and counts["kept_components"] == 1


def test_level_areas(capi):
    assert capi.level_areas(0, 3) == [1, 1, 1]
    assert capi.level_areas(10, 4) == [10, 3, 1, 1]
    assert capi.level_areas(144, 4) == [144, 36, 9, 3]
    for a0 in range(0, 300, 7):
        assert capi.level_areas(a0, 5) == ref.level_areas(a0, 5) == [max(1, int(np.ceil(a0 / 4 ** l))) for l in range(5)]


def test_the_union_find_passes_its_host_check(tmp_path):
    """find, union, the 16-bit minimum, the edge rule and the ranking key as the kernels compile them, run on the host in many
    shuffled orders and from several threads at once, under the address and undefined-behaviour sanitizers"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "components_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-pthread", "-I", os.path.join(ROOT, "dvo_slam_amd", "csrc"), os.path.join(ROOT, "tests", "host", "components_host_check.cpp"),
            "-o", exe]
    # the sanitizer runtimes linked into the program itself, so that it runs in whatever environment the suite runs in; a compiler
    # without the static runtimes links them dynamically, and the stand-alone program is then told not to insist on coming first
    # among the libraries of its process
    env = dict(os.environ)
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], None):
        build = subprocess.run(base + (static or []), capture_output=True, text=True, timeout=300)
        if build.returncode == 0:
            break
    assert build.returncode == 0, build.stderr[-3000:]
    if static is None:
        env["ASAN_OPTIONS"] = ":".join(filter(None, [env.get("ASAN_OPTIONS"), "verify_asan_link_order=0"]))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and run.stdout.startswith("components_host_check: ok"), run.stdout + run.stderr[-3000:]
    assert not run.stderr.strip(), run.stderr[-3000:]


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
    assert set(NEW_SYMBOLS) <= declared and sorted(capi.EXPORTS) == sorted(declared)
    assert L.dvo_amd_abi_version() == 3
    assert capi.COMPONENT_COUNTS == ref.COUNTS and capi.COMPONENT_COUNTS_DTYPE.itemsize == 48
    assert capi.COMPONENT_DTYPE == ref.RECORD_DTYPE and capi.COMPONENT_DTYPE.itemsize == 28
    assert capi.COMPONENTS_MAX_LARGEST == ref.MAX_LARGEST == 8


def test_the_default_options_are_the_documented_ones(capi):
    opt = capi.ComponentOptions()
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt))
    capi.lib().dvo_amd_default_component_options(C.byref(opt))
    assert (opt.connectivity, opt.max_step, opt.depth_sigmas, opt.keep_largest) == (8, 0.0, 10.0, 0)
    assert list(opt.min_area) == [0] * capi.MAX_LEVELS and list(opt.max_area) == [-1] * capi.MAX_LEVELS
    assert C.sizeof(opt) == 4 * (3 + 2 * capi.MAX_LEVELS + 1)
    capi.lib().dvo_amd_default_component_options(None)  # a no-op
    assert ref.DEFAULTS == dict(connectivity=8, max_step=0.0, depth_sigmas=10.0, min_area=0, max_area=-1, keep_largest=0)
    opt = capi.component_options(connectivity=4, min_area=[3, 2], max_area=9, keep_largest=2, max_step=0.5, depth_sigmas=6)
    assert (opt.connectivity, opt.max_step, opt.depth_sigmas, opt.keep_largest) == (4, 0.5, 6.0, 2)
    assert list(opt.min_area)[:3] == [3, 2, 0] and list(opt.max_area) == [9] * capi.MAX_LEVELS
    with pytest.raises(TypeError):
        capi.component_options(radius=1)


class _FakeMask(C.Structure):
    """what the argument checks read of a mask: enough of one to be refused or passed on without a device.  The layout is the
    library's own object, so the test builds none: it takes a real handle's place only where the check fails before any field is
    read (NULL checks, the options)."""
    _fields_ = [("bytes", C.c_char * 4096)]


def test_argument_errors_are_reported_without_a_device(capi):
    L = capi.lib()
    something = _FakeMask()  # stands for a mask or a pyramid where the refusal comes before the object is looked at
    p = C.c_void_p(C.addressof(something))
    good = capi.component_options()
    cnt = (C.c_longlong * 64)()
    n = C.c_int(77)

    def refused(rc, handle, entry, words):
        assert rc == INVALID, (entry, words, rc)
        assert handle is None or not handle.value, (entry, words)
        reason = L.dvo_amd_last_error().decode()
        assert reason.startswith(entry + ": ") and any(w in reason for w in words), (entry, words, reason)

    entry = "dvo_amd_mask_filter_components"
    h = C.c_void_p(0xDEAD)
    refused(L.dvo_amd_mask_filter_components(None, None, None, C.byref(good), C.byref(h), cnt), h, entry, ["both NULL"])
    h = C.c_void_p(0xDEAD)
    refused(L.dvo_amd_mask_filter_components(None, None, p, C.byref(good), C.byref(h), cnt), h, entry, ["both NULL"])
    h = C.c_void_p(0xDEAD)
    refused(L.dvo_amd_mask_filter_components(p, None, None, None, C.byref(h), cnt), h, entry, ["NULL"])
    assert L.dvo_amd_mask_filter_components(p, None, None, C.byref(good), None, cnt) == INVALID
    bad_options = [(dict(connectivity=6), "connectivity"), (dict(connectivity=0), "connectivity"), (dict(max_step=-0.1), "max_step"),
                   (dict(max_step=np.nan), "max_step"), (dict(max_step=np.inf), "max_step"), (dict(depth_sigmas=-1.0), "depth_sigmas"),
                   (dict(depth_sigmas=np.nan), "depth_sigmas"), (dict(depth_sigmas=np.inf), "depth_sigmas"),
                   (dict(keep_largest=-1), "keep_largest"), (dict(keep_largest=9), "keep_largest")]
    one, null_in = (C.c_void_p * 1)(p), (C.c_void_p * 1)(None)
    for fields, word in bad_options:
        bad = capi.component_options(**fields)
        h = C.c_void_p(0xDEAD)
        refused(L.dvo_amd_mask_filter_components(p, None, None, C.byref(bad), C.byref(h), cnt), h, entry, [word])
        outs = (C.c_void_p * 1)(0xDEAD)
        assert L.dvo_amd_mask_filter_components_many(1, one, None, None, C.byref(bad), outs, cnt) == INVALID and not outs[0], fields
        assert L.dvo_amd_last_error().decode().startswith("dvo_amd_mask_filter_components_many: "), fields
        n.value = 77
        refused(L.dvo_amd_mask_components(p, None, None, C.byref(bad), 0, None, None, 0, C.byref(n)), None, "dvo_amd_mask_components", [word])
        assert n.value == 0
    many = "dvo_amd_mask_filter_components_many"
    for what, args in {"masks and depths": (1, None, None, None, C.byref(good)), "options": (1, one, None, None, None),
                       "masks[0] and depths[0]": (1, null_in, null_in, None, C.byref(good)),
                       "masks[0], no depths": (1, null_in, None, one, C.byref(good))}.items():
        outs = (C.c_void_p * 1)(0xDEAD)
        rc = L.dvo_amd_mask_filter_components_many(*args, outs, cnt)
        assert rc == INVALID and not outs[0], (what, rc)
        assert L.dvo_amd_last_error().decode().startswith(many + ": ") and "NULL" in L.dvo_amd_last_error().decode(), what
    assert L.dvo_amd_mask_filter_components_many(1, one, None, None, C.byref(good), None, cnt) == INVALID
    outs = (C.c_void_p * 1)(0xDEAD)
    assert L.dvo_amd_mask_filter_components_many(-1, one, None, None, C.byref(good), outs, cnt) == INVALID
    # the inspection entry
    comp = "dvo_amd_mask_components"
    assert L.dvo_amd_mask_components(p, None, None, C.byref(good), 0, None, None, 0, None) == INVALID
    refused(L.dvo_amd_mask_components(None, None, None, C.byref(good), 0, None, None, 0, C.byref(n)), None, comp, ["both NULL"])
    refused(L.dvo_amd_mask_components(p, None, None, None, 0, None, None, 0, C.byref(n)), None, comp, ["NULL"])
    refused(L.dvo_amd_mask_components(p, None, None, C.byref(good), 0, None, None, -1, C.byref(n)), None, comp, ["capacity"])
    refused(L.dvo_amd_mask_components(p, None, None, C.byref(good), 0, None, None, 3, C.byref(n)), None, comp, ["NULL"])
    # a zeroed buffer reads as a mask without levels: every level is outside it, and min_area is checked on no level
    refused(L.dvo_amd_mask_components(p, None, None, C.byref(good), 0, None, None, 0, C.byref(n)), None, comp, ["level"])
    refused(L.dvo_amd_mask_components(p, None, None, C.byref(good), -1, None, None, 0, C.byref(n)), None, comp, ["level"])
    assert L.dvo_amd_debug_components_timing(-1, 0, None) == INVALID
    if L.dvo_amd_device_count() == 0:
        # nothing left to refuse: the device is looked for
        h = C.c_void_p(0xDEAD)
        assert L.dvo_amd_mask_filter_components(p, None, None, C.byref(good), C.byref(h), cnt) == NO_DEVICE and not h.value
        outs = (C.c_void_p * 1)(0xDEAD)
        assert L.dvo_amd_mask_filter_components_many(0, one, None, None, C.byref(good), outs, cnt) == NO_DEVICE
        assert L.dvo_amd_debug_components_timing(0, 1, None) == NO_DEVICE
        with pytest.raises(capi.DvoAmdError) as e:
            capi.components_timing(True)
        assert e.value.status == NO_DEVICE


class _MaskHead(C.Structure):
    """the fields the argument checks read of a mask (dvo_internal.h: refs, device, w, h, levels), followed by zeros"""
    _fields_ = [("refs", C.c_int), ("device", C.c_int), ("w", C.c_int), ("h", C.c_int), ("levels", C.c_int), ("rest", C.c_char * 4096)]


class _PyramidHead(C.Structure):
    """... and of a pyramid: refs, device, n_levels, the timestamp, and the size that opens level 0's record"""
    _fields_ = [("refs", C.c_int), ("device", C.c_int), ("n_levels", C.c_int), ("timestamp", C.c_double), ("w0", C.c_int),
                ("h0", C.c_int), ("rest", C.c_char * 8192)]


def test_inputs_that_do_not_fit_are_refused_without_a_device(capi):
    """the checks read a mask's and a pyramid's size and level count and nothing else of them: stand-ins that hold just those are
    refused with the sizes in the reason (which also shows that the stand-ins are read as meant)"""
    L = capi.lib()
    good = capi.component_options()
    cnt = (C.c_longlong * 64)()
    n = C.c_int()

    def mask(w, h, levels, device=0):
        return _MaskHead(refs=1, device=device, w=w, h=h, levels=levels)

    def pyramid(w, h, levels, device=0):
        return _PyramidHead(refs=1, device=device, n_levels=levels, w0=w, h0=h)

    def filter_rc(m, d, s, opt=good):
        h = C.c_void_p(0xDEAD)
        rc = L.dvo_amd_mask_filter_components(C.byref(m) if m else None, C.byref(d) if d else None, C.byref(s) if s else None, C.byref(opt),
                                              C.byref(h), cnt)
        assert not h.value
        return rc, L.dvo_amd_last_error().decode()

    a = mask(80, 48, 3)
    for what, (m, d, s), words in (("seeds of another size", (a, None, mask(64, 32, 3)), "80x48 but seeds is 64x32"),
                                   ("seeds with fewer levels", (a, None, mask(80, 48, 2)), "3 levels but seeds has 2"),
                                   ("depth of another size", (a, pyramid(64, 32, 3), None), "80x48 but depth is 64x32"),
                                   ("depth with fewer levels", (a, pyramid(80, 48, 2), None), "3 levels but depth has 2"),
                                   ("seeds that do not fit the depth", (None, pyramid(80, 48, 3), mask(72, 50, 3)), "80x48 but seeds is 72x50"),
                                   ("seeds with fewer levels than the depth", (None, pyramid(80, 48, 3), mask(80, 48, 1)), "3 levels but seeds has 1")):
        rc, reason = filter_rc(m, d, s)
        assert rc == INVALID and reason.startswith("dvo_amd_mask_filter_components: ") and words in reason, (what, rc, reason)
    rc, reason = filter_rc(a, None, None, capi.component_options(min_area=[0, 0, -1]))
    assert rc == INVALID and "min_area[2]" in reason, reason
    # inside the arrays of the many-form, with the item named
    outs = (C.c_void_p * 2)(0xDEAD, 0xDEAD)
    masks = (C.c_void_p * 2)(C.addressof(a), C.addressof(a))
    bad_seeds = mask(80, 48, 2)
    seeds = (C.c_void_p * 2)(None, C.addressof(bad_seeds))
    assert L.dvo_amd_mask_filter_components_many(2, masks, None, seeds, C.byref(good), outs, cnt) == INVALID and not outs[0] and not outs[1]
    assert "item 1: " in L.dvo_amd_last_error().decode()
    # the inspection entry reads only the edge rule, and validates the rest as the filter does
    negative = capi.component_options(min_area=[0, 0, -1])
    assert L.dvo_amd_mask_components(C.byref(a), None, None, C.byref(negative), 0, None, None, 0, C.byref(n)) == INVALID
    assert "min_area[2]" in L.dvo_amd_last_error().decode()
    # the inspection entry: the level
    for level in (-1, 3, 100):
        assert L.dvo_amd_mask_components(C.byref(a), None, None, C.byref(good), level, None, None, 0, C.byref(n)) == INVALID, level
        assert "level" in L.dvo_amd_last_error().decode()
    # objects on different devices: after every INVALID_ARGUMENT, before the device is looked for
    rc, _ = filter_rc(a, None, mask(80, 48, 3, device=1))
    assert rc == MISMATCH
    rc, _ = filter_rc(a, pyramid(80, 48, 3, device=1), None)
    assert rc == MISMATCH
    rc, _ = filter_rc(a, pyramid(80, 48, 3, device=1), mask(64, 32, 3))
    assert rc == INVALID
    if L.dvo_amd_device_count() == 0:
        # what fits goes on to look for the device: more levels than the mask has, a negative min_area beyond the item's levels
        rc, _ = filter_rc(mask(80, 48, 2), pyramid(80, 48, 3), a, capi.component_options(min_area=[0, 0, -1]))
        assert rc == NO_DEVICE
        assert L.dvo_amd_mask_components(C.byref(a), None, None, C.byref(good), 2, None, None, 0, C.byref(n)) == NO_DEVICE


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


def _status(capi, call):
    with pytest.raises(capi.DvoAmdError) as err:
        call()
    return err.value.status


def _counts_dict(record):
    return {name: int(record[name]) for name in ref.COUNTS}


def _same_filter(got, want_planes, want_counts, what):
    """the mask's planes, its kept counts and the counts record are the restated ones"""
    mask, counts = got
    info = mask.info()
    assert info["levels"] == len(want_planes), what
    for l, p in enumerate(want_planes):
        plane = mask.download(l)
        assert plane.shape == p.shape and np.array_equal(plane, p), (what, l)
        assert _counts_dict(counts[l]) == want_counts[l], (what, l, _counts_dict(counts[l]), want_counts[l])
    assert info["kept"] == [int(p.sum()) for p in want_planes], what


def _same_components(got, mask_plane, depth_plane, seeds_plane, what, **rule):
    labels, records = got
    want_labels, _ = ref.label(mask_plane, depth_plane, **rule)
    assert labels.dtype == np.int32 and labels.shape == want_labels.shape and np.array_equal(labels, want_labels), what
    want = ref.records(want_labels, seeds_plane)
    assert records.dtype == ref.RECORD_DTYPE and np.array_equal(records, want), what


FILTERS = [dict(), dict(min_area=[4, 2, 1]), dict(max_area=[12, 5, 2]), dict(min_area=[3, 2, 2], max_area=[40, 30, 20]),
           dict(keep_largest=1), dict(keep_largest=3), dict(keep_largest=8), dict(keep_largest=3, min_area=2, max_area=30)]


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(SIZES))
def test_patterns_equal_the_restatement(gpu, name, connectivity):
    """every pattern on every level: the label plane and the records of the inspection entry; the masks, kept[l] and the counts of
    the filter under area bands, seeds and keep_largest"""
    w, h, levels = SIZES[name]
    assert w % TILE and h % TILE
    seeds_planes = [_random(w >> l, h >> l, 0.02, 40 + l) for l in range(levels)]
    seeds = gpu.SelectionMask.from_levels(seeds_planes)
    for pattern in PATTERNS:
        planes = _levels_of(pattern, w, h, levels)
        M = gpu.SelectionMask.from_levels(planes)
        what = (name, connectivity, pattern)
        for l in range(levels):
            _same_components(M.components(l, connectivity=connectivity), planes[l], None, None, what + (l,), connectivity=connectivity)
        _same_components(M.components(levels - 1, seeds=seeds, connectivity=connectivity), planes[-1], None, seeds_planes[-1],
                         what + ("seeded",), connectivity=connectivity)
        for fields in FILTERS:
            want = ref.filter_levels(planes, connectivity=connectivity, **fields)
            _same_filter(M.filter_components(counts=True, connectivity=connectivity, **fields), *want, what + (str(fields),))
        # seeds: a sparse random seed mask; the same with an area band; seeds that keep only background pixels
        want = ref.filter_levels(planes, seeds=seeds_planes, connectivity=connectivity)
        _same_filter(M.filter_components(seeds=seeds, counts=True, connectivity=connectivity), *want, what + ("seeds",))
        want = ref.filter_levels(planes, seeds=seeds_planes, connectivity=connectivity, min_area=2, keep_largest=3)
        _same_filter(M.filter_components(seeds=seeds, counts=True, connectivity=connectivity, min_area=2, keep_largest=3), *want,
                     what + ("seeds, band, largest",))
        background = [(p == 0).astype(np.uint8) for p in planes]
        got = M.filter_components(seeds=gpu.SelectionMask.from_levels(background), counts=True, connectivity=connectivity)
        want = ref.filter_levels(planes, seeds=background, connectivity=connectivity)
        assert all(not p.any() for p in want[0])
        _same_filter(got, *want, what + ("background seeds",))
        # the input is only read, and the defaults return the foreground
        for l in range(levels):
            assert np.array_equal(M.download(l), (planes[l] != 0).astype(np.uint8)), what
        if connectivity == 8:
            plain = M.filter_components()
            assert [np.array_equal(plain.download(l), (planes[l] != 0)) for l in range(levels)] == [True] * levels, what
            rec = M.reconstruct(seeds)
            assert np.array_equal(rec.download(0), ref.filter_components(planes[0], seeds=seeds_planes[0])[0]), what


@pytest.mark.gpu
def test_keep_largest_breaks_ties_by_the_lower_root(gpu):
    w, h, levels = SIZES["136x72"]
    planes = _levels_of("blocks", w, h, levels)
    M = gpu.SelectionMask.from_levels(planes)
    for largest in (1, 3, 8):
        mask, counts = M.filter_components(counts=True, keep_largest=largest)
        out = mask.download(0)
        recs = ref.records(ref.label(planes[0])[0])
        nines = [int(c["root"]) for c in recs if c["area"] == 9]
        assert len(nines) > 8
        assert int(counts[0]["kept_components"]) == largest and int(counts[0]["kept_pixels"]) == 24 + 9 * (largest - 1)
        assert [bool(out.ravel()[r]) for r in nines] == [k < largest - 1 for k in range(len(nines))]
    assert _status(gpu, lambda: M.filter_components(keep_largest=9)) == INVALID


def _sensor_depth(synth, w, h):
    _, Z = synth.raw_to_float(*synth.sensor_frame(w, h))
    return Z


@pytest.fixture(scope="module")
def blobs(gpu, synth):
    """the 160 x 120 sensor frame with blobs of area 1, 9 and 144 pasted 40 % nearer, as a pyramid of three levels"""
    w, h, levels = 160, 120, 3
    I, Z = synth.raw_to_float(*synth.sensor_frame(w, h))
    Z = Z.copy()
    Z[20, 20] *= F(0.6)
    Z[30:33, 40:43] *= F(0.6)
    big = Z[58:70, 60:72]       # across the tile seams at x = 64 and y = 64; the frame's few missing pixels there are given a depth
    big[np.isnan(big)] = F(np.nanmean(big))
    big *= F(0.6)
    assert np.isfinite(Z[20, 20]) and np.isfinite(Z[30:33, 40:43]).all() and np.isfinite(Z[58:70, 60:72]).all()
    pyramid = gpu.RgbdImagePyramid(I, Z, synth.intrinsics_for(w, h), levels)
    return dict(w=w, h=h, levels=levels, Z=Z, pyramid=pyramid, depth=[pyramid.plane(l, 1) for l in range(levels)])


@pytest.mark.gpu
@pytest.mark.parametrize("connectivity", [4, 8])
def test_depth_blobs_on_the_sensor_frame(gpu, blobs, connectivity):
    P, depth, levels = blobs["pyramid"], blobs["depth"], blobs["levels"]
    assert np.array_equal(depth[0], blobs["Z"], equal_nan=True)
    labels, records = P.depth_components(level=0, connectivity=connectivity)
    assert sorted(int(a) for a in records["area"])[:3] == [1, 9, 144] and len(records) == 4
    for l in range(levels):
        _same_components(P.depth_components(level=l, connectivity=connectivity), None, depth[l], None, ("blobs", l), connectivity=connectivity)
    for fields in (dict(), dict(min_area=gpu.level_areas(10, levels)), dict(min_area=2, max_area=gpu.level_areas(144, levels)),
                   dict(keep_largest=1), dict(keep_largest=3, max_area=200), dict(depth_sigmas=3.0), dict(depth_sigmas=0.0, max_step=0.002),
                   dict(depth_sigmas=6.0, max_step=0.01, min_area=5)):
        want = ref.filter_levels(None, depth, connectivity=connectivity, **fields)
        _same_filter(P.depth_components(counts=True, connectivity=connectivity, **fields), *want, ("blobs", str(fields)))
    despeckled, counts = P.depth_components(counts=True, connectivity=connectivity, min_area=gpu.level_areas(10, levels))
    want0 = np.isfinite(depth[0]).astype(np.uint8)
    want0[20, 20] = 0
    want0[30:33, 40:43] = 0
    assert np.array_equal(despeckled.download(0), want0) and int(counts[0]["edges_cut"]) > 0
    # a mask on top of the depth, seeds on the depth alone
    m_planes = [_random(blobs["w"] >> l, blobs["h"] >> l, 0.9, 60 + l) for l in range(levels)]
    M = gpu.SelectionMask.from_levels(m_planes)
    want = ref.filter_levels(m_planes, depth, connectivity=connectivity, min_area=3)
    _same_filter(M.filter_components(depth=P, counts=True, connectivity=connectivity, min_area=3), *want, "mask and depth")
    _same_components(M.components(1, depth=P, connectivity=connectivity), m_planes[1], depth[1], None, "mask and depth", connectivity=connectivity)
    seed_planes = [np.zeros_like(p) for p in m_planes]
    for l in range(levels):
        seed_planes[l][(64 >> l), (66 >> l)] = 1   # inside the large blob
    S = gpu.SelectionMask.from_levels(seed_planes)
    want = ref.filter_levels(None, depth, seeds=seed_planes, connectivity=connectivity)
    got = P.depth_components(seeds=S, counts=True, connectivity=connectivity)
    _same_filter(got, *want, "the surface a seed lies on")
    assert int(got[1][0]["kept_pixels"]) == 144


def _staircase(w, h, step_x):
    """three bands of rows, each a plane at 1 m on the left of column step_x and a plane further away on its right: by exactly the
    tolerance, by one ulp of the depth less, by one ulp more.  max_step is chosen so that the tolerance at 1 m is 2^-5 exactly (the
    difference of two depths in [1, 2) is exact, a multiple of 2^-23)."""
    sigmas = F(10.0)
    c = sigmas * (F(0.0012) + F(0.0019) * ((F(1.0) - F(0.4)) * (F(1.0) - F(0.4))))
    max_step = F(F(2.0 ** -5) - c)
    for _ in range(8):  # (the rounded difference may miss by an ulp: walk to it)
        tol = F(max_step + c)
        if tol == F(2.0 ** -5):
            break
        max_step = np.nextafter(max_step, F(1.0) if tol < F(2.0 ** -5) else F(0.0), dtype=F)
    assert F(max_step + c) == F(2.0 ** -5) and max_step > 0
    at = F(1.0) + F(2.0 ** -5)
    far = [at, np.nextafter(at, F(0.0), dtype=F), np.nextafter(at, F(2.0), dtype=F)]
    Z = np.full((h, w), np.nan, F)
    band = h // 3
    for k in range(3):
        Z[k * band:(k + 1) * band - 1, :step_x] = F(1.0)
        Z[k * band:(k + 1) * band - 1, step_x:] = far[k]
        assert (F(far[k] - F(1.0)) <= F(2.0 ** -5)) == (k < 2)
    return Z, float(max_step), float(sigmas)


@pytest.mark.gpu
@pytest.mark.parametrize("name,step_x", [("136x72", 64), ("72x50", 37)])
def test_a_depth_step_exactly_at_the_tolerance(gpu, synth, name, step_x):
    """at the tolerance and one ulp below it the two planes are one surface, one ulp above they are two -- at a tile seam and inside
    a tile, on both connectivities"""
    w, h, _ = SIZES[name]
    Z, max_step, sigmas = _staircase(w, h, step_x)
    P = gpu.RgbdImagePyramid(np.zeros((h, w), F), Z, synth.intrinsics_for(w, h), 1)
    assert np.array_equal(P.plane(0, 1), Z, equal_nan=True)
    band = h // 3
    for connectivity in (4, 8):
        rule = dict(connectivity=connectivity, max_step=max_step, depth_sigmas=sigmas)
        labels, records = P.depth_components(level=0, **rule)
        _same_components((labels, records), None, Z, None, (name, connectivity), **rule)
        assert len(records) == 4
        assert labels[0, 0] == labels[0, w - 1] and labels[band, 0] == labels[band, w - 1] and labels[2 * band, 0] != labels[2 * band, w - 1]
        mask, counts = P.depth_components(counts=True, **rule)
        want = ref.filter_levels(None, [Z], **rule)
        _same_filter((mask, counts), *want, (name, connectivity))
        assert int(counts[0]["edges_cut"]) == (band - 1) * (1 if connectivity == 4 else 3) - (0 if connectivity == 4 else 2)


@pytest.mark.gpu
def test_nan_pixels_inside_a_component(gpu, synth):
    w, h, levels = SIZES["80x48"]
    rng = np.random.default_rng(17)
    I, Z = synth.render(w, h, nan_fraction=0.0, hole=False)
    Z = Z.copy()
    Z[rng.uniform(size=(h, w)) < 0.15] = np.nan
    Z[10:14, :] = np.nan      # a bar of missing depth across the frame
    Z[10:14, 30] = Z[9, 30]   # ... with a one-pixel bridge
    P = gpu.RgbdImagePyramid(I, Z, synth.intrinsics_for(w, h), levels)
    depth = [P.plane(l, 1) for l in range(levels)]
    ones = gpu.SelectionMask.from_levels([np.ones((h >> l, w >> l), np.uint8) for l in range(levels)])
    for connectivity in (4, 8):
        for l in range(levels):
            _same_components(P.depth_components(level=l, connectivity=connectivity), None, depth[l], None, ("nan", connectivity, l),
                             connectivity=connectivity)
        want = ref.filter_levels(None, depth, connectivity=connectivity, min_area=4)
        _same_filter(P.depth_components(counts=True, connectivity=connectivity, min_area=4), *want, ("nan", connectivity))
        # an all-ones mask changes nothing
        _same_filter(ones.filter_components(depth=P, counts=True, connectivity=connectivity, min_area=4), *want, ("nan, ones", connectivity))
    labels, _ = P.depth_components(level=0, connectivity=4)
    assert (labels[np.isnan(depth[0])] == 0).all() and (labels[np.isfinite(depth[0])] > 0).all()


@pytest.fixture(scope="module")
def mixed_items(gpu, synth):
    """eight items of mixed sizes and level counts: masks alone, depth alone, both, with and without seeds"""
    items = []
    names = ["80x48", "72x50", "136x72", "200x136", "72x50", "80x48", "136x72", "80x48"]
    for k, name in enumerate(names):
        w, h, levels = SIZES[name]
        pattern = list(PATTERNS)[(3 * k + 4) % len(PATTERNS)]
        deeper = 1 if k == 7 else 0   # the last item's pyramid has a level more than its mask
        levels -= deeper
        m_planes = _levels_of(pattern, w, h, levels) if k % 4 != 1 else None
        P = None
        if k % 2 == 1 or k == 6:
            I, Z = synth.render(w, h, frame_id=k, nan_fraction=0.05)
            Z = Z.copy()
            Z[h // 4:h // 2, w // 8:w // 3] *= F(0.6)
            P = gpu.RgbdImagePyramid(I, Z, synth.intrinsics_for(w, h), levels + deeper)
        s_planes = [_random(w >> l, h >> l, 0.03, 70 + k + l) for l in range(levels)] if k % 3 == 0 else None
        items.append(dict(name=name, levels=levels, m_planes=m_planes, pyramid=P, s_planes=s_planes,
                          mask=None if m_planes is None else gpu.SelectionMask.from_levels(m_planes),
                          seeds=None if s_planes is None else gpu.SelectionMask.from_levels(s_planes)))
    return items


def _bits(result):
    masks, counts = result
    return [[m.download(l).tobytes() for l in range(m.info()["levels"])] + [m.info()["kept"], c.tobytes()] for m, c in zip(masks, counts)]


@pytest.mark.gpu
@pytest.mark.parametrize("fields", [dict(connectivity=4, min_area=[3, 2, 1]), dict(connectivity=8, keep_largest=3, max_area=500)])
def test_many_items_in_one_call_equal_their_single_calls(gpu, mixed_items, fields):
    masks = [i["mask"] for i in mixed_items]
    depths = [i["pyramid"] for i in mixed_items]
    seeds = [i["seeds"] for i in mixed_items]
    assert any(m is None for m in masks) and any(d is None for d in depths) and any(s is None for s in seeds)
    assert len({(i["name"], i["levels"]) for i in mixed_items}) == 5
    together = gpu.SelectionMask.filter_components_many(masks, depths, seeds, counts=True, **fields)
    again = gpu.SelectionMask.filter_components_many(masks, depths, seeds, counts=True, **fields)
    assert _bits(together) == _bits(again)   # two runs of the same call are bit-identical
    for k, item in enumerate(mixed_items):
        if item["mask"] is not None:
            single = item["mask"].filter_components(depth=item["pyramid"], seeds=item["seeds"], counts=True, **fields)
        else:
            single = item["pyramid"].depth_components(seeds=item["seeds"], counts=True, **fields)
        assert _bits(([single[0]], [single[1]])) == _bits(([together[0][k]], [together[1][k]])), k
        depth = None if item["pyramid"] is None else [item["pyramid"].plane(l, 1) for l in range(item["levels"])]
        want = ref.filter_levels(item["m_planes"], depth, item["s_planes"], **fields)
        _same_filter((together[0][k], together[1][k]), *want, ("many", k))
    # NULL arrays for depths and seeds
    only_masks = [i for i in mixed_items if i["mask"] is not None]
    plain = gpu.SelectionMask.filter_components_many([i["mask"] for i in only_masks], counts=True, **fields)
    for k, item in enumerate(only_masks):
        _same_filter((plain[0][k], plain[1][k]), *ref.filter_levels(item["m_planes"], **fields), ("masks only", k))
    assert gpu.SelectionMask.filter_components_many([]) == []


@pytest.mark.gpu
def test_arguments_that_do_not_fit_are_refused(gpu, synth, mixed_items):
    L = gpu.lib()
    a = gpu.SelectionMask.from_level0(np.ones((48, 80), np.uint8), 3)
    shallow = gpu.SelectionMask.from_level0(np.ones((48, 80), np.uint8), 2)
    other = gpu.SelectionMask.from_level0(np.ones((32, 64), np.uint8), 3)
    I, Z = synth.render(80, 48)
    deep, flat = gpu.RgbdImagePyramid(I, Z, synth.intrinsics_for(80, 48), 3), gpu.RgbdImagePyramid(I, Z, synth.intrinsics_for(80, 48), 2)
    I2, Z2 = synth.render(64, 32)
    elsewhere = gpu.RgbdImagePyramid(I2, Z2, synth.intrinsics_for(64, 32), 3)
    for what, call in {"seeds with fewer levels": lambda: a.filter_components(seeds=shallow),
                       "seeds of another size": lambda: a.filter_components(seeds=other),
                       "depth with fewer levels": lambda: a.filter_components(depth=flat),
                       "depth of another size": lambda: a.filter_components(depth=elsewhere),
                       "seeds that do not fit the depth": lambda: deep.depth_components(seeds=other),
                       "a negative min_area on a level the item has": lambda: a.filter_components(min_area=[0, 0, -1]),
                       "a level outside the mask": lambda: a.components(3),
                       "a negative level": lambda: a.components(-1),
                       "a level outside the pyramid": lambda: flat.depth_components(level=2),
                       "one bad item": lambda: gpu.SelectionMask.filter_components_many([a, a], [deep, flat])}.items():
        assert _status(gpu, call) == INVALID, what
        assert L.dvo_amd_last_error().decode().startswith("dvo_amd_mask_"), what
    # what fits: more levels than the mask has, a negative min_area beyond the item's levels
    assert shallow.filter_components(depth=deep, seeds=a, min_area=[0, 0, -1]).info()["levels"] == 2
    # capacity: the true total comes back, at most `capacity` records are written
    M = mixed_items[0]["mask"]
    labels, records = M.components(0)
    assert len(records) > 3
    opt = gpu.component_options()
    few = np.zeros(3, gpu.COMPONENT_DTYPE)
    few[2]["root"] = -7
    n = C.c_int()
    assert L.dvo_amd_mask_components(M._h, None, None, C.byref(opt), 0, None, few.ctypes.data_as(C.c_void_p), 2, C.byref(n)) == 0
    assert n.value == len(records) and np.array_equal(few[:2], records[:2]) and few[2]["root"] == -7
    if L.dvo_amd_device_count() > 1:
        far = gpu.SelectionMask.from_level0(np.ones((48, 80), np.uint8), 3, device=1)
        assert _status(gpu, lambda: a.filter_components(seeds=far)) == MISMATCH


@pytest.mark.gpu
def test_a_filtered_mask_is_an_ordinary_mask(gpu, synth):
    """residual-style speckle on a region of interest, despeckled by reconstruction from its erosion: the match behind the result
    is the match behind the restated planes uploaded from the host, bit for bit"""
    w, h, levels = 160, 120, 4
    K = synth.intrinsics_for(w, h)
    frames = [synth.render(w, h, synth.se3_exp(0.5 * k * synth.XI_GT_PAIR), frame_id=k) for k in range(2)]
    f1, f2 = [gpu.RgbdImagePyramid(I, Z, K, levels) for I, Z in frames]
    trk = gpu.DenseTracker(gpu.Config(FirstLevel=levels - 1, LastLevel=0))
    m0 = np.zeros((h, w), np.uint8)
    m0[h // 4:(3 * h) // 4, w // 4:(3 * w) // 4] = 1
    m0 |= _random(w, h, 0.03, 5)                         # speckle outside
    m0 &= 1 - _random(w, h, 0.02, 6)                     # pinholes inside
    M = gpu.SelectionMask.from_level0(m0, levels)
    planes = cases.mask_pyramid(m0, levels, False)
    radii = gpu.level_radii(2, levels)
    filtered = M.reconstruct(M.erode(2))
    seeds = [ops_ref.morph_ref(p, ops_ref.ERODE, r) for p, r in zip(planes, radii)]
    want, _ = ref.filter_levels(planes, seeds=seeds)
    for l in range(levels):
        assert np.array_equal(filtered.download(l), want[l]), l
    assert 0 < want[0].sum() < planes[0].sum()
    kept = filtered.info()["kept"]
    del M
    got = trk.match(f1, f2, mask=filtered)
    uploaded = gpu.SelectionMask.from_levels(want)
    assert cases.same_result(got, trk.match(f1, f2, mask=uploaded))
    assert not got.isNaN() and not cases.same_result(got, trk.match(f1, f2))
    assert filtered.info()["kept"] == kept == [int(p.sum()) for p in want]


@pytest.mark.gpu
def test_device_time_is_reported_when_asked_for(gpu, mixed_items):
    M = mixed_items[0]["mask"]
    gpu.components_timing(True)
    try:
        M.filter_components(min_area=3)
        first = gpu.components_timing(True)
        assert 0.0 < first < 1000.0
    finally:
        gpu.components_timing(False)
    M.filter_components(min_area=3)
    assert gpu.components_timing(False) == first  # off: the figure stays
