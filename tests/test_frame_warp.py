"""Frame warps on the device (include/dvo_amd.h, "Frame warps"): dvo_amd_warp_inverse / _forward, their many forms and their pyramid
forms.  The rules are pinned in the header and restated twice per direction in tests/warp_ref.py.  Every comparison with the
library is equality -- of float planes on their bit patterns over every pixel, of index planes, of integer counts.  The one
inequality is the use: a frame warped at the true motion is nearer to the other frame than the frame itself.
CPU: exports and layout, the argument checks that need no device, the two restatements against each other on every case, the
loop against the reference's control flow, the exact case, the use.  GPU: the library against the restatement."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_ref as ref  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_warp_options", "dvo_amd_warp_inverse", "dvo_amd_warp_inverse_many", "dvo_amd_pyramid_warp_inverse",
               "dvo_amd_pyramid_warp_inverse_many", "dvo_amd_warp_forward", "dvo_amd_warp_forward_many", "dvo_amd_pyramid_warp_forward",
               "dvo_amd_pyramid_warp_forward_many", "dvo_amd_debug_warp_timing"]
INVALID, NO_DEVICE, MISMATCH = 1, 2, 8
W, H, LEVELS = 64, 48, 3
KX = (64.0, 64.0, 32.0, 24.0)  # the exact set-up: fx = fy = 64, an integer principal point
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(a, b):
    return a.dtype == b.dtype == F and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


# ---- the cases: frames are (I, Z, K, levels) at level 0; T maps the moving camera into the fixed one --------------------------------

def exact_frame(seed, block=True, holes=True):
    """integer grey values; depth 2 with a nearer block at 1 and a hole: every product of the exact set-up is exact"""
    rng = np.random.RandomState(seed)
    I = rng.randint(0, 256, (H, W)).astype(F)
    Z = np.full((H, W), 2.0, F)
    if block:
        Z[10:20, 12:24] = 1.0
    if holes:
        Z[30:33, 40:45] = np.nan
    return I, Z, KX, LEVELS


def shift(dx, dy, z=2.0, tz=0.0):
    """a translation that moves a point at depth z by (dx, dy) pixels of the exact set-up"""
    T = np.eye(4)
    T[0, 3], T[1, 3], T[2, 3] = dx * z / 64.0, dy * z / 64.0, tz
    return T


def patterned_frame(seed):
    """depth 2 with occluders at 1 (nearer than qz - margin) and NaNs on 1, 2, 3, 4 and 9 pixels: with a half-pixel shift a fixed
    pixel meets every number of missing taps"""
    I, Z, K, levels = exact_frame(seed, block=False, holes=False)
    for value, x in ((1.0, 0), (np.nan, 32)):
        Z[6, x + 4] = value
        Z[6, x + 10:x + 12] = value
        Z[12, x + 4:x + 6] = value
        Z[13, x + 4] = value
        Z[12:14, x + 10:x + 12] = value
        Z[20:23, x + 4:x + 7] = value
    return I, Z, K, levels


class Case:
    def __init__(self, fixed, moving, T, level=0, view=None, **options):
        self.fixed, self.moving, self.T, self.level, self.view, self.options = fixed, moving, np.asarray(T, np.float64), level, view, options


def _stand_in(frame, level):
    """a level's planes without a device: the frame subsampled (the GPU tests take the level's planes from the pyramid itself)"""
    I, Z, K, _ = frame
    s = 1 << level
    return I[::s, ::s].copy(), Z[::s, ::s].copy(), tuple(F(k) / F(s) for k in K)


@functools.lru_cache(maxsize=None)
def frames():
    from dvo_slam_amd import synth

    out = {}
    out["exact_a"], out["exact_b"] = exact_frame(1), exact_frame(2)
    out["flat_a"], out["flat_b"] = exact_frame(3, block=False), exact_frame(4, block=False, holes=False)
    out["patterned"] = patterned_frame(5)
    near = exact_frame(6)
    near[1][5:9, 5:9] = 0.125
    out["near"] = near
    K = synth.intrinsics_for(W, H)
    (Ir, Zr), (Ic, Zc), T = synth.make_pair(W, H)
    out["synth_ref"], out["synth_cur"], out["synth_T"] = (Ir, Zr, K, LEVELS), (Ic, Zc, K, LEVELS), T
    (_, _), (If, Zf), Tf = synth.make_pair(W, H, xi_gt=12 * synth.XI_GT_PAIR, frame_id=3)
    out["far_cur"], out["far_T"] = (If, Zf, K, LEVELS), Tf
    Ks = tuple(F(k) for k in (40.0, 38.0, 15.5, 11.25))
    Ts = synth.se3_exp(3 * synth.XI_GT_PAIR)
    out["small_cur"], out["small_T"] = synth.render(32, 24, Ts, frame_id=9, K=Ks) + (Ks, LEVELS), Ts
    return out


@functools.lru_cache(maxsize=None)
def inverse_cases():
    f = frames()
    c = {}
    c["exact"] = Case(f["exact_a"], f["exact_b"], shift(3, 2))
    c["identity"] = Case(f["flat_b"], f["flat_b"], np.eye(4))
    for name, opt in (("half", {}), ("half_no_buffer", dict(occlusion_margin=INF)), ("half_fixed_depth", dict(depth=ref.DEPTH_FIXED))):
        c[name] = Case(f["flat_a"], f["patterned"], shift(0.5, 0.5), **opt)
    c["just_below_zero"] = Case(f["flat_a"], f["flat_b"], shift(1.0 / 64, 1.0 / 64))
    c["just_below_size"] = Case(f["flat_a"], f["flat_b"], shift(-63.0 / 64, -63.0 / 64))
    c["behind"] = Case(f["near"], f["exact_b"], shift(3, 2, tz=0.0625))
    for level in range(LEVELS):
        c["synth_l%d" % level] = Case(f["synth_ref"], f["synth_cur"], f["synth_T"], level=level)
    c["synth_fixed_depth"] = Case(f["synth_ref"], f["synth_cur"], f["synth_T"], depth=ref.DEPTH_FIXED, near_z=2.9)
    c["far"] = Case(f["synth_ref"], f["far_cur"], f["far_T"], occlusion_margin=0.0)
    c["far_l2"] = Case(f["synth_ref"], f["far_cur"], f["far_T"], level=2)
    c["other_camera"] = Case(f["synth_ref"], f["small_cur"], f["small_T"])
    c["other_camera_l1"] = Case(f["small_cur"], f["synth_ref"], np.linalg.inv(f["small_T"]), level=1)
    return c


@functools.lru_cache(maxsize=None)
def forward_cases():
    f = frames()
    c = {}
    splats = (("nearest", ref.SPLAT_NEAREST), ("floor", ref.SPLAT_FLOOR), ("footprint", ref.SPLAT_FOOTPRINT))
    views = {"own": None, "half": ((32.0, 32.0, 16.0, 12.0), 32, 24, 0.1), "zoom": ((128.0, 128.0, 32.0, 24.0), W, H, 0.1),
             "large": ((128.0, 128.0, 64.0, 48.0), 128, 96, 0.1)}
    for sname, splat in splats:
        for vname, view in views.items():
            c["exact_%s_%s" % (vname, sname)] = Case(None, f["exact_b"], shift(3, 2), view=view, splat=splat)
        c["synth_%s" % sname] = Case(None, f["synth_cur"], f["synth_T"], splat=splat)
        c["far_%s_l1" % sname] = Case(None, f["far_cur"], f["far_T"], level=1, splat=splat)
    c["identity"] = Case(None, f["flat_b"], np.eye(4))
    c["equal_depths"] = Case(None, f["flat_b"], shift(3, 2), view=views["half"], splat=ref.SPLAT_FLOOR)
    c["half_pixel_floor"] = Case(None, f["exact_b"], shift(2.5, 1.5), splat=ref.SPLAT_FLOOR)
    c["half_pixel_nearest"] = Case(None, f["exact_b"], shift(2.5, 1.5), splat=ref.SPLAT_NEAREST)
    c["footprint17"] = Case(None, f["flat_a"], np.eye(4), view=((1024.0, 1024.0, 32.0, 24.0), W, H, 0.1), splat=ref.SPLAT_FOOTPRINT)
    c["footprint16"] = Case(None, f["flat_a"], np.eye(4), view=((1024.0, 1024.0, 32.5, 24.5), W, H, 0.1), splat=ref.SPLAT_FOOTPRINT)
    c["behind"] = Case(None, f["synth_cur"], f["synth_T"], view=(f["synth_cur"][2], W, H, 2.9), splat=ref.SPLAT_FOOTPRINT)
    c["synth_l2"] = Case(None, f["synth_cur"], f["synth_T"], level=2, splat=ref.SPLAT_FOOTPRINT)
    c["other_camera"] = Case(None, f["small_cur"], f["small_T"], view=(f["synth_ref"][2], W, H, 0.1), splat=ref.SPLAT_FOOTPRINT)
    return c


@functools.lru_cache(maxsize=None)
def cpu_inverse(name):
    """the vectorised restatement of a case on its stand-in planes: computed once, shared, read-only"""
    c = inverse_cases()[name]
    If, Zf, Kf = _stand_in(c.fixed, c.level)
    got = ref.inverse_ref((Zf, Kf), _stand_in(c.moving, c.level), c.T, c.options)
    got[0].setflags(write=False), got[1].setflags(write=False), got[3].setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def cpu_forward(name):
    c = forward_cases()[name]
    got = ref.forward_ref(_stand_in(c.moving, c.level), c.T, c.view, c.options)
    for a in got[:3]:
        a.setflags(write=False)
    return got


# ---- CPU: exports and layout ------------------------------------------------------------------------------------------------------

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
    assert "dvo_warp.cpp" in __import__("dvo_slam_amd._build", fromlist=["SOURCES"]).SOURCES
    assert (capi.WARP_DEPTH_TRANSFORMED, capi.WARP_DEPTH_FIXED) == (ref.DEPTH_TRANSFORMED, ref.DEPTH_FIXED) == (0, 1)
    assert (capi.WARP_SPLAT_NEAREST, capi.WARP_SPLAT_FLOOR, capi.WARP_SPLAT_FOOTPRINT) == \
        (ref.SPLAT_NEAREST, ref.SPLAT_FLOOR, ref.SPLAT_FOOTPRINT) == (0, 1, 2)
    assert capi.WARP_MAX_FOOTPRINT == ref.MAX_FOOTPRINT == 16
    assert capi.WARP_INVERSE_COUNTS == ref.INVERSE_COUNTS and capi.WARP_INVERSE_DTYPE.itemsize == 64
    assert capi.WARP_FORWARD_COUNTS == ref.FORWARD_COUNTS and capi.WARP_FORWARD_DTYPE.itemsize == 56
    header = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    for define, value in (("DVO_AMD_WARP_DEPTH_TRANSFORMED", 0), ("DVO_AMD_WARP_DEPTH_FIXED", 1), ("DVO_AMD_WARP_SPLAT_NEAREST", 0),
                          ("DVO_AMD_WARP_SPLAT_FLOOR", 1), ("DVO_AMD_WARP_SPLAT_FOOTPRINT", 2), ("DVO_AMD_WARP_MAX_FOOTPRINT", 16),
                          ("DVO_AMD_WARP_INVERSE_COUNTS", 8), ("DVO_AMD_WARP_FORWARD_COUNTS", 7)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define


def test_the_default_options_are_the_documented_ones(capi):
    opt = capi.WarpOptions()
    assert C.sizeof(opt) == 20
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt))
    capi.lib().dvo_amd_default_warp_options(C.byref(opt))
    got = (opt.near_z, opt.occlusion_margin, opt.depth, opt.splat, opt.fill_intensity)
    assert got == (F(0.1), F(0.05), capi.WARP_DEPTH_TRANSFORMED, capi.WARP_SPLAT_NEAREST, 0.0)
    for k, v in ref.DEFAULTS.items():  # the restatement's defaults are the library's
        assert F(getattr(opt, k)) == F(v), k
    capi.lib().dvo_amd_default_warp_options(None)  # a no-op
    assert capi.warp_options(splat=capi.WARP_SPLAT_FOOTPRINT, occlusion_margin=INF).occlusion_margin == INF
    with pytest.raises(TypeError):
        capi.warp_options(depth_sigmas=1.0)


# ---- CPU: the argument checks -----------------------------------------------------------------------------------------------------

class Fakes:
    """zeroed buffers that stand for pyramids of two levels on device 0 (refs, device, n_levels lead a pyramid): an argument error
    is reported before any of them is looked at beyond its level count and its device"""

    def __init__(self, capi, n=3, device=0):
        self.keep = [C.create_string_buffer(1 << 16) for _ in range(2 * n)]
        for b in self.keep:
            C.c_int.from_buffer(b, 4).value = device
            C.c_int.from_buffer(b, 8).value = 2
        self.fixed = (C.c_void_p * n)(*[C.addressof(b) for b in self.keep[:n]])
        self.moving = (C.c_void_p * n)(*[C.addressof(b) for b in self.keep[n:]])
        self.T = (C.c_double * (16 * n))(*np.tile(np.eye(4).ravel(), n))
        self.views = (capi.CView * n)(*[capi.CView(8, 6, 10.0, 10.0, 4.0, 3.0, 0.1) for _ in range(n)])
        self.opt = capi.warp_options()
        self.n = n


BAD_OPTIONS = (("near_z", 0.0), ("near_z", -1.0), ("near_z", np.nan), ("near_z", INF), ("occlusion_margin", -0.5),
               ("occlusion_margin", np.nan), ("depth", 2), ("depth", -1), ("splat", 3), ("splat", -1), ("fill_intensity", np.nan),
               ("fill_intensity", INF))
BAD_VIEWS = (("width", 0), ("height", -1), ("width", 1 << 14, "height", 1 << 13), ("fx", 0.0), ("fy", np.nan), ("fx", INF), ("ox", np.nan),
             ("oy", INF), ("near_z", 0.0), ("near_z", np.nan))


def test_argument_errors_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    f = Fakes(capi)
    cnt = (C.c_longlong * 64)()
    byref = lambda o: None if o is None else C.byref(o)  # noqa: E731

    def refused(entry, got, what, word=None):
        rc, handle = got
        assert rc == INVALID, (entry, what, rc)
        assert not handle, (entry, what)
        reason = L.dvo_amd_last_error().decode()
        assert reason.startswith(entry + ": "), (entry, what, reason)
        assert word is None or word in reason, (entry, what, reason)

    # every entry as f(**overrides) -> (status, an output handle or None); the plane entries have no handle
    def inverse(fixed=f.fixed[0], moving=f.moving[0], T=f.T, level=0, opt=f.opt):
        return L.dvo_amd_warp_inverse(fixed, moving, T, level, byref(opt), None, None, cnt), None

    def inverse_many(n=f.n, fixed=f.fixed, moving=f.moving, T=f.T, level=0, opt=f.opt):
        return L.dvo_amd_warp_inverse_many(n, fixed, moving, T, level, byref(opt), None, None, cnt), None

    def inverse_pyramid(fixed=f.fixed[0], moving=f.moving[0], T=f.T, opt=f.opt, with_out=True):
        h = C.c_void_p(0xDEAD)
        return L.dvo_amd_pyramid_warp_inverse(fixed, moving, T, byref(opt), C.byref(h) if with_out else None, cnt), h.value if with_out else None

    def inverse_pyramid_many(n=f.n, fixed=f.fixed, moving=f.moving, T=f.T, opt=f.opt, with_out=True):
        outs = (C.c_void_p * f.n)(*[0xDEAD] * f.n)
        rc = L.dvo_amd_pyramid_warp_inverse_many(n, fixed, moving, T, byref(opt), outs if with_out else None, cnt)
        return rc, (any(outs) if n >= 0 else None) if with_out else None

    def forward(moving=f.moving[0], T=f.T, view=f.views[0], level=0, opt=f.opt):
        return L.dvo_amd_warp_forward(moving, T, byref(view), level, byref(opt), None, None, None, cnt), None

    def forward_many(n=f.n, moving=f.moving, T=f.T, views=f.views, level=0, opt=f.opt):
        return L.dvo_amd_warp_forward_many(n, moving, T, views, level, byref(opt), None, None, None, cnt), None

    def forward_pyramid(moving=f.moving[0], T=f.T, view=f.views[0], opt=f.opt, with_out=True):
        h = C.c_void_p(0xDEAD)
        rc = L.dvo_amd_pyramid_warp_forward(moving, T, byref(view), byref(opt), C.byref(h) if with_out else None, cnt)
        return rc, h.value if with_out else None

    def forward_pyramid_many(n=f.n, moving=f.moving, T=f.T, views=f.views, opt=f.opt, with_out=True):
        outs = (C.c_void_p * f.n)(*[0xDEAD] * f.n)
        rc = L.dvo_amd_pyramid_warp_forward_many(n, moving, T, views, byref(opt), outs if with_out else None, cnt)
        return rc, (any(outs) if n >= 0 else None) if with_out else None

    singles = {"dvo_amd_warp_inverse": inverse, "dvo_amd_pyramid_warp_inverse": inverse_pyramid, "dvo_amd_warp_forward": forward,
               "dvo_amd_pyramid_warp_forward": forward_pyramid}
    manys = {"dvo_amd_warp_inverse_many": inverse_many, "dvo_amd_pyramid_warp_inverse_many": inverse_pyramid_many,
             "dvo_amd_warp_forward_many": forward_many, "dvo_amd_pyramid_warp_forward_many": forward_pyramid_many}
    holed = (C.c_void_p * 3)(f.moving[0], None, f.moving[2])
    for entry, call in list(singles.items()) + list(manys.items()):
        inv, many, pyr = "inverse" in entry, entry.endswith("_many"), "pyramid" in entry
        for what in ("moving", "T", "opt") + (("fixed",) if inv else ()):
            refused(entry, call(**{what: None}), what, "NULL")
        if pyr:
            assert call(with_out=False)[0] == INVALID
            assert L.dvo_amd_last_error().decode().startswith(entry + ": ")
        if many:
            refused(entry, call(moving=holed), "moving[1]", "NULL")
            refused(entry, call(n=-1), "n < 0", "negative")
        if not pyr:
            refused(entry, call(level=2), "level 2 of 2", "level")
            refused(entry, call(level=-1), "level -1", "level")
        for bad in (np.nan, INF, -INF):
            for at in ((0, 16 + 7, 32 + 15) if many else (0, 7, 15)):
                T = (C.c_double * 48)(*f.T)
                T[at] = bad
                refused(entry, call(T=T), ("T", bad, at), "non-finite")
        for field, value in BAD_OPTIONS:
            refused(entry, call(opt=capi.warp_options(**{field: value})), (field, value), field)
        if not inv:
            for bad in BAD_VIEWS:
                views = (capi.CView * f.n)(*[capi.CView(8, 6, 10.0, 10.0, 4.0, 3.0, 0.1) for _ in range(f.n)])
                at = f.n - 1 if many else 0
                for k in range(0, len(bad), 2):
                    setattr(views[at], bad[k], bad[k + 1])
                refused(entry, call(views=views) if many else call(view=views[0]), bad, "view")
            if pyr:  # the view becomes a pyramid of the moving pyramid's two levels: dvo_amd_pyramid_create_from_device's rule
                odd = capi.CView(6, 6, 10.0, 10.0, 4.0, 3.0, 0.1)
                refused(entry, call(views=(capi.CView * f.n)(*[odd] * f.n)) if many else call(view=odd), "6x6 in two levels")
    # a fixed pyramid with fewer levels than asked for, where the moving one has them
    C.c_int.from_buffer(f.keep[0], 8).value = 1
    refused("dvo_amd_warp_inverse", inverse(level=1), "level 1 of the fixed pyramid's 1", "level")
    C.c_int.from_buffer(f.keep[0], 8).value = 2
    # then the devices, then the device
    other = Fakes(capi, device=1)
    mixed = (C.c_void_p * 3)(f.moving[0], other.moving[1], f.moving[2])
    assert inverse(moving=other.moving[0])[0] == MISMATCH
    assert inverse_pyramid(moving=other.moving[0]) == (MISMATCH, None)
    for call in manys.values():
        assert call(moving=mixed)[0] == MISMATCH
    if L.dvo_amd_device_count() == 0:
        # nothing left to refuse: the device is looked for, and the outputs are still NULL
        for call in singles.values():
            assert call() == (NO_DEVICE, None)
        for entry, call in manys.items():
            assert call() == (NO_DEVICE, False if "pyramid" in entry else None)
            assert call(n=0)[0] == NO_DEVICE
        assert forward(view=None)[0] == NO_DEVICE and forward_many(views=None)[0] == NO_DEVICE
        assert L.dvo_amd_debug_warp_timing(0, 1, None, None, None) == NO_DEVICE
    assert L.dvo_amd_debug_warp_timing(-1, 0, None, None, None) == INVALID
    assert L.dvo_amd_debug_warp_timing(0, 0, None, None, None) == 0


# ---- CPU: the restatements --------------------------------------------------------------------------------------------------------

def _inverse_identities(cnt):
    assert cnt["valid"] == cnt["behind"] + cnt["outside"] + cnt["border"] + cnt["hidden"] + cnt["warped"]
    assert cnt["partial"] <= cnt["warped"]


def _forward_identities(cnt, index):
    assert cnt["valid"] == cnt["behind"] + cnt["outside"] + cnt["too_large"] + cnt["drawn"]
    assert cnt["covered_pixels"] == np.count_nonzero(index >= 0)


@pytest.mark.parametrize("name", sorted(inverse_cases()))
def test_the_inverse_restatement_matches_the_pixel_loop(name):
    c = inverse_cases()[name]
    a = cpu_inverse(name)
    If, Zf, Kf = _stand_in(c.fixed, c.level)
    b = ref.inverse_loop((Zf, Kf), _stand_in(c.moving, c.level), c.T, c.options)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])
    _inverse_identities(a[2])
    assert a[2]["valid"] + a[2]["no_depth"] == Zf.size
    # empty where the rule says so
    assert np.array_equal(np.isnan(a[0]), a[3] != ref.WARPED)
    assert np.array_equal(np.isnan(a[1]), ~np.isin(a[3], (ref.BORDER, ref.HIDDEN, ref.WARPED)))


@pytest.mark.parametrize("name", sorted(forward_cases()))
def test_the_forward_restatement_matches_the_pixel_loop(name):
    c = forward_cases()[name]
    a = cpu_forward(name)
    b = ref.forward_loop(_stand_in(c.moving, c.level), c.T, c.view, c.options)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert a[2].dtype == np.int32
    _forward_identities(a[3], a[2])
    assert np.array_equal(np.isnan(a[0]), a[2] < 0) and np.array_equal(np.isnan(a[1]), a[2] < 0)


def test_the_cases_reach_every_outcome():
    seen = dict.fromkeys(ref.INVERSE_COUNTS, 0)
    for name in inverse_cases():
        for k, v in cpu_inverse(name)[2].items():
            seen[k] += v
    assert all(v > 0 for v in seen.values()), seen
    seen = dict.fromkeys(ref.FORWARD_COUNTS, 0)
    for name in forward_cases():
        for k, v in cpu_forward(name)[3].items():
            seen[k] += v
    assert all(v > 0 for v in seen.values()), seen
    # outside on all four sides of the moving frame
    out = cpu_inverse("other_camera")[3] == ref.OUTSIDE
    assert out[0, :].any() and out[-1, :].any() and out[:, 0].any() and out[:, -1].any()


def test_the_inverse_edges_are_what_they_are_meant_to_be():
    # half a pixel: four taps of weight 1/4; occluders and NaNs take 1, 2, 3 or all 4 of them away
    I, Z, cnt, cls = cpu_inverse("half")
    moving = inverse_cases()["half"].moving
    missing = ~(np.isfinite(moving[1]) & (moving[1] > F(1.95)))
    for v in range(1, H - 1):
        for u in range(1, W - 1):
            if cls[v, u] in (ref.WARPED, ref.HIDDEN):  # the taps (v-1..v, u-1..u)
                n = int(missing[v - 1:v + 1, u - 1:u + 1].sum())
                assert (cls[v, u] == ref.HIDDEN) == (n == 4), (v, u, n)
    taken = {int(missing[v - 1:v + 1, u - 1:u + 1].sum()) for v in range(1, H) for u in range(1, W) if cls[v, u] in (ref.WARPED, ref.HIDDEN)}
    assert taken == {0, 1, 2, 3, 4} and cnt["partial"] > 0 and cnt["hidden"] > 0
    # without the depth buffer only the NaNs are missing; the depth plane does not change
    I2, Z2, cnt2, _ = cpu_inverse("half_no_buffer")
    assert 0 < cnt2["hidden"] < cnt["hidden"] and 0 < cnt2["partial"] < cnt["partial"] and same_bits(Z, Z2)
    # the other depth mode changes the depth plane alone: the fixed frame's own depth where the pixel passed inImage
    I3, Z3, cnt3, cls3 = cpu_inverse("half_fixed_depth")
    assert same_bits(I, I3) and cnt == cnt3
    there = np.isin(cls3, (ref.BORDER, ref.HIDDEN, ref.WARPED))
    assert np.array_equal(bits(Z3)[there], bits(inverse_cases()["half"].fixed[1])[there])
    # px = -1/64: the first column and row are outside; px = wm - 1/64: the last column and row are inside, and border
    _, _, cnt, cls = cpu_inverse("just_below_zero")
    valid = np.isfinite(inverse_cases()["just_below_zero"].fixed[1])
    assert (cls[0, :][valid[0, :]] == ref.OUTSIDE).all() and (cls[:, 0][valid[:, 0]] == ref.OUTSIDE).all()
    assert cnt["outside"] == int(valid[0, :].sum() + valid[1:, 0].sum()) and cnt["border"] == 0
    _, _, cnt, cls = cpu_inverse("just_below_size")
    assert (cls[-1, :] == ref.BORDER).all() and (cls[:, -1] == ref.BORDER).all() and cnt["outside"] == 0
    assert cnt["border"] == W + H - 1
    # behind
    _, _, cnt, cls = cpu_inverse("behind")
    assert cnt["behind"] == 16 and (cls[5:9, 5:9] == ref.BEHIND).all()


def test_the_forward_edges_are_what_they_are_meant_to_be():
    # 17 columns are too large, 16 are drawn
    d, _, x, cnt = cpu_forward("footprint17")
    assert cnt["too_large"] == cnt["valid"] > 0 and cnt["drawn"] == cnt["covered_pixels"] == 0 and (x < 0).all()
    d, _, x, cnt = cpu_forward("footprint16")
    assert cnt["too_large"] == 0 and cnt["drawn"] > 0 and cnt["outside"] > 0
    for r in np.unique(x[x >= 0]):  # clipped at the view's edges or 16 x 16
        ys, xs = np.nonzero(x == r)
        assert xs.max() - xs.min() + 1 <= 16 and ys.max() - ys.min() + 1 <= 16
    inner = [r for r in np.unique(x[x >= 0]) if (x == r).sum() == 256]
    assert inner, "a whole 16 x 16 footprint lies in the view"
    # bit-equal depths on one pixel: the lower index wins (a view of half the size: four source pixels per target pixel)
    d, i, x, cnt = cpu_forward("equal_depths")
    assert cnt["drawn"] > 3 * cnt["covered_pixels"] and (d[x >= 0] == F(2.0)).all()
    # columns 2k-3, 2k-2 and rows 2m-2, 2m-1 land on (k, m): the first of the four wins (column 1 has only source column 0)
    assert (x[:, 0] < 0).all() and (x[0, :] < 0).all() and (x[1:, 1:] >= 0).all()
    vs, us = np.divmod(x[1:, 2:], W)
    assert (us % 2 == 1).all() and (vs % 2 == 0).all() and (x[1:, 1] % W == 0).all()
    # different depths on one pixel: the nearer wins
    d, i, x, cnt = cpu_forward("exact_own_nearest")
    assert cnt["drawn"] > cnt["covered_pixels"]
    block = d == F(1.0)
    assert block.sum() == 10 * 12 and block[10 + 4:20 + 4, 12 + 6:24 + 6].all()
    # footprints clipped at each edge of the view
    d, i, x, cnt = cpu_forward("exact_zoom_footprint")
    assert (x[0, :] >= 0).any() and (x[-1, :] >= 0).any() and (x[:, 0] >= 0).any() and (x[:, -1] >= 0).any() and cnt["outside"] > 0
    # a view larger than the source is filled by the footprints and not by single pixels
    assert cpu_forward("exact_large_footprint")[3]["covered_pixels"] > 2 * cpu_forward("exact_large_nearest")[3]["covered_pixels"]


def test_the_direction_of_T_on_the_exact_case():
    """fx = fy = 64, depths 1 and 2, T a translation of (3, 2) pixels at depth 2 -- (6, 4) at depth 1.  Every product is exact.
    Inverse: a fixed pixel of depth z at (u, v) takes the moving value at (u - 6/z, v - 4/z), one tap of weight 1.  Forward: a
    moving pixel of depth z at (u, v) goes to (u + 6/z, v + 4/z).  Both move the image towards +x, +y."""
    c = inverse_cases()["exact"]
    I, Z, cnt, cls = cpu_inverse("exact")
    Zf, Im = c.fixed[1], c.moving[0]
    assert cnt["warped"] > 0.8 * W * H and cnt["hidden"] > 0
    for v, u in zip(*np.nonzero(cls == ref.WARPED)):
        s = int(2 / Zf[v, u])
        assert I[v, u] == Im[v - 2 * s, u - 3 * s] and Z[v, u] == Zf[v, u]
    # a pixel is hidden where its one tap of weight 1 is nearer than qz - margin: the zero-weight taps do not count
    for v, u in zip(*np.nonzero(cls == ref.HIDDEN)):
        s = int(2 / Zf[v, u])
        zt = c.moving[1][v - 2 * s, u - 3 * s]
        assert not (np.isfinite(zt) and zt > Zf[v, u] - F(0.05))
    d, i, x, fc = cpu_forward("exact_own_nearest")
    flat = Im.ravel()
    for v, u in zip(*np.nonzero(x >= 0)):
        vs, us = divmod(int(x[v, u]), W)
        s = int(2 / d[v, u])
        assert (vs + 2 * s, us + 3 * s) == (v, u) and i[v, u] == flat[x[v, u]] and d[v, u] == c.moving[1][vs, us]
    both = (cls == ref.WARPED) & (x >= 0) & (Zf == F(2.0)) & (d == F(2.0))
    assert both.sum() > 0.5 * W * H and np.array_equal(I[both], i[both])
    # the inverse transformation moves it the other way
    back = ref.inverse_ref((Zf, c.fixed[2]), c.moving[:3], np.linalg.inv(c.T))
    v, u = 40, 8  # (depth 2 on both sides)
    assert back[0][v, u] == Im[v + 2, u + 3] and I[v, u + 6] == Im[v - 2, u + 3]


def test_the_identity_on_the_exact_case():
    c = inverse_cases()["identity"]
    I, Z, cnt, cls = cpu_inverse("identity")
    assert (cls[:-1, :-1] == ref.WARPED).all() and (cls[-1, :] == ref.BORDER).all() and (cls[:, -1] == ref.BORDER).all()
    assert same_bits(I[:-1, :-1], c.moving[0][:-1, :-1]) and same_bits(Z, c.moving[1]) and cnt["partial"] == 0
    d, i, x, fc = cpu_forward("identity")
    assert same_bits(d, c.moving[1]) and same_bits(i, c.moving[0]) and np.array_equal(x.ravel(), np.arange(W * H))


@pytest.mark.parametrize("name", ["exact", "half", "just_below_size", "synth_l0", "far", "other_camera"])
def test_the_loop_with_the_references_formulae_gives_the_references_classes(name):
    """no point of these cases is behind near_z"""
    c = inverse_cases()[name]
    assert cpu_inverse(name)[2]["behind"] == 0 and "depth" not in c.options
    fixed, moving = (c.fixed[1], c.fixed[2]), c.moving[:3]
    opt = dict(c.options, occlusion_margin=0.05)  # (the reference's constant)
    ours = ref.inverse_loop(fixed, moving, c.T, opt, point=ref.reference_point)[3]
    assert np.array_equal(ours, ref.reference_classes(fixed, moving, c.T))


def _mean_abs_difference(fixed_I, warped_I, cls):
    m = cls == ref.WARPED
    return float(np.abs(fixed_I[m].astype(np.float64) - warped_I[m]).mean())


def test_the_true_motion_aligns_the_frames_in_the_restatement():
    f = frames()
    fixed, moving = f["synth_ref"], f["far_cur"]
    at_T = ref.inverse_ref((fixed[1], fixed[2]), moving[:3], f["far_T"])
    at_I = ref.inverse_ref((fixed[1], fixed[2]), moving[:3], np.eye(4))
    a, b = _mean_abs_difference(fixed[0], at_T[0], at_T[3]), _mean_abs_difference(fixed[0], at_I[0], at_I[3])
    print(f"mean |I_fixed - I_warped| over warped pixels: {a:.3f} at T, {b:.3f} at the identity")
    assert a < b


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


class Resident:
    """the frames' pyramids on the device (a frame is uploaded once), their level planes as the device holds them, and the
    restatement of every case on those planes (computed once, shared, read-only)"""

    def __init__(self, capi):
        self.capi, self.made, self.levels, self.wanted = capi, {}, {}, {}

    def pyramid(self, frame):
        if id(frame) not in self.made:
            self.made[id(frame)] = self.capi.RgbdImagePyramid(frame[0], frame[1], frame[2], frame[3], timestamp=3.25 + len(self.made))
        return self.made[id(frame)]

    def planes(self, frame, level):
        key = (id(frame), level)
        if key not in self.levels:
            p = self.pyramid(frame)
            self.levels[key] = (p.plane(level, 0), p.plane(level, 1), tuple(p.level_info(level)[2]))
        return self.levels[key]

    def want(self, kind, name):
        if (kind, name) not in self.wanted:
            c = (inverse_cases() if kind == "inverse" else forward_cases())[name]
            moving = self.planes(c.moving, c.level)
            if kind == "inverse":
                fixed = self.planes(c.fixed, c.level)
                got = ref.inverse_ref((fixed[1], fixed[2]), moving, c.T, c.options)
            else:
                got = ref.forward_ref(moving, c.T, c.view, c.options)
            for a in got:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self.wanted[(kind, name)] = got
        return self.wanted[(kind, name)]

    def inverse(self, name, level="case"):
        c = inverse_cases()[name]
        return self.pyramid(c.moving).warp_inverse(self.pyramid(c.fixed), c.T, c.level if level == "case" else level, c.options)

    def forward(self, name, level="case"):
        c = forward_cases()[name]
        return self.pyramid(c.moving).warp_forward(c.T, c.view, c.level if level == "case" else level, c.options)


@pytest.fixture(scope="module")
def resident(gpu):
    return Resident(gpu)


def _counts(record, names):
    return {k: int(record[k]) for k in names}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(inverse_cases()))
def test_the_inverse_warp_equals_the_restatement(resident, name):
    I, Z, cnt = resident.inverse(name)
    want = resident.want("inverse", name)
    assert same_bits(I, want[0]), name
    assert same_bits(Z, want[1]), name
    assert _counts(cnt, ref.INVERSE_COUNTS) == want[2], name
    _inverse_identities(_counts(cnt, ref.INVERSE_COUNTS))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(forward_cases()))
def test_the_forward_warp_equals_the_restatement(resident, name):
    d, i, x, cnt = resident.forward(name)
    want = resident.want("forward", name)
    assert same_bits(d, want[0]), name
    assert same_bits(i, want[1]), name
    assert x.dtype == np.int32 and np.array_equal(x, want[2]), name
    assert _counts(cnt, ref.FORWARD_COUNTS) == want[3], name
    _forward_identities(_counts(cnt, ref.FORWARD_COUNTS), x)


@pytest.mark.gpu
def test_the_exact_case_and_the_identity_on_the_device(resident):
    c = inverse_cases()["exact"]
    I, Z, cnt = resident.inverse("exact")
    Zf, Im = c.fixed[1], c.moving[0]
    cls = resident.want("inverse", "exact")[3]
    assert cnt["warped"] > 0.8 * W * H
    for v, u in zip(*np.nonzero(cls == ref.WARPED)):
        s = int(2 / Zf[v, u])
        assert I[v, u] == Im[v - 2 * s, u - 3 * s]
    d, i, x, _ = resident.forward("exact_own_nearest")
    both = (cls == ref.WARPED) & (x >= 0) & (Zf == F(2.0)) & (d == F(2.0))
    assert both.sum() > 0.5 * W * H and np.array_equal(I[both], i[both])  # the same T moves the image the same way
    for v, u in zip(*np.nonzero(x >= 0)):
        vs, us = divmod(int(x[v, u]), W)
        s = int(2 / d[v, u])
        assert (vs + 2 * s, us + 3 * s) == (v, u)
    c = inverse_cases()["identity"]
    I, Z, cnt = resident.inverse("identity")
    assert same_bits(I[:-1, :-1], c.moving[0][:-1, :-1]) and np.isnan(I[-1, :]).all() and np.isnan(I[:, -1]).all()
    assert cnt["border"] == W + H - 1 and cnt["warped"] == (W - 1) * (H - 1)
    d, i, x, cnt = resident.forward("identity")
    assert same_bits(d, c.moving[1]) and same_bits(i, c.moving[0]) and np.array_equal(x.ravel(), np.arange(W * H))


def _same_pyramid(a, b, what):
    assert a.levels() == b.levels(), what
    for level in range(a.levels()):
        ia, ib = a.level_info(level), b.level_info(level)
        assert ia[:2] == ib[:2] and np.array_equal(ia[2], ib[2]), (what, level)
        for plane in range(6):
            assert same_bits(a.plane(level, plane), b.plane(level, plane)), (what, level, plane)


def _from_device_planes(capi, I, Z, K, levels, timestamp):
    import torch

    d_i, d_z = torch.from_numpy(np.ascontiguousarray(I)).cuda(), torch.from_numpy(np.ascontiguousarray(Z)).cuda()
    torch.cuda.synchronize()
    h, w = I.shape
    return capi.RgbdImagePyramid.from_device(d_i.data_ptr(), d_z.data_ptr(), w, h, K, levels, timestamp=timestamp)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["half", "synth_l0", "synth_fixed_depth", "other_camera"])
def test_the_inverse_pyramid_form(gpu, resident, name):
    c = inverse_cases()[name]
    options = dict(c.options, fill_intensity=7.5)
    fixed, moving = resident.pyramid(c.fixed), resident.pyramid(c.moving)
    I, Z, cnt = moving.warp_inverse(fixed, c.T, 0, options)
    p, pcnt = moving.warp_inverse(fixed, c.T, None, options)
    assert _counts(pcnt, ref.INVERSE_COUNTS) == _counts(cnt, ref.INVERSE_COUNTS)
    eI, eZ = ref.empty_rule(I, Z, resident.want("inverse", name)[3], 7.5)
    assert same_bits(p.plane(0, 0), eI) and same_bits(p.plane(0, 1), eZ)
    assert np.array_equal(np.isfinite(eZ), resident.want("inverse", name)[3] == ref.WARPED) and (eI[~np.isfinite(eZ)] == F(7.5)).all()
    assert p.levels() == fixed.levels() and p.timestamp() == fixed.timestamp()
    _same_pyramid(p, _from_device_planes(gpu, eI, eZ, c.fixed[2], c.fixed[3], fixed.timestamp()), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["exact_own_nearest", "exact_half_floor", "exact_large_footprint", "synth_footprint"])
def test_the_forward_pyramid_form(gpu, resident, name):
    c = forward_cases()[name]
    options = dict(c.options, fill_intensity=7.5)
    moving = resident.pyramid(c.moving)
    d, i, x, cnt = moving.warp_forward(c.T, c.view, 0, options)
    p, pcnt = moving.warp_forward(c.T, c.view, None, options)
    assert _counts(pcnt, ref.FORWARD_COUNTS) == _counts(cnt, ref.FORWARD_COUNTS)
    eI = np.where(x >= 0, i, F(7.5)).astype(F)
    assert same_bits(p.plane(0, 0), eI) and same_bits(p.plane(0, 1), d)
    K = c.view[0] if c.view is not None else c.moving[2]
    assert p.levels() == moving.levels() and p.timestamp() == moving.timestamp()
    assert p.level_info(0)[:2] == (d.shape[1], d.shape[0]) and np.array_equal(p.level_info(0)[2], np.asarray(K, F))
    _same_pyramid(p, _from_device_planes(gpu, eI, d, K, c.moving[3], moving.timestamp()), name)


@pytest.mark.gpu
def test_a_warped_pyramid_is_tracked(gpu, resident):
    f = frames()
    fixed, moving = resident.pyramid(f["synth_ref"]), resident.pyramid(f["synth_cur"])
    trk = gpu.DenseTracker(gpu.Config(FirstLevel=2, LastLevel=0), device=0)
    for p in (moving.warp_inverse(fixed, f["synth_T"])[0], moving.warp_forward(f["synth_T"], options=dict(splat=ref.SPLAT_FOOTPRINT))[0]):
        r = trk.match(fixed, p)
        assert not r.isNaN() and np.isfinite(r.Transformation).all()


MIXED_INVERSE = ["synth_l0", "other_camera", "half_fixed_depth", "exact", "far"]  # one set of options per call: the defaults
MIXED_FORWARD = ["exact_half_footprint", "synth_footprint", "exact_large_footprint", "other_camera", "footprint16"]


@pytest.mark.gpu
def test_many_equals_singles_in_any_order_and_twice(gpu, resident):
    ic = [inverse_cases()[n] for n in MIXED_INVERSE]
    singles = [resident.pyramid(c.moving).warp_inverse(resident.pyramid(c.fixed), c.T, 0) for c in ic]
    for order in ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [0, 1, 2, 3, 4]):
        I, Z, cnt = gpu.warp_inverse_many([resident.pyramid(ic[k].fixed) for k in order], [resident.pyramid(ic[k].moving) for k in order],
                                          [ic[k].T for k in order], 0)
        for j, k in enumerate(order):
            assert same_bits(I[j], singles[k][0]) and same_bits(Z[j], singles[k][1]), (order, j)
            assert _counts(cnt[j], ref.INVERSE_COUNTS) == _counts(singles[k][2], ref.INVERSE_COUNTS)
        pyramids, pcnt = gpu.warp_inverse_many([resident.pyramid(ic[k].fixed) for k in order], [resident.pyramid(ic[k].moving) for k in order],
                                               [ic[k].T for k in order])
        assert np.array_equal(pcnt, cnt)
        for j, k in enumerate(order):
            eI, eZ = ref.empty_rule(singles[k][0], singles[k][1], np.where(np.isnan(singles[k][0]), 0, ref.WARPED), 0.0)
            assert same_bits(pyramids[j].plane(0, 0), eI) and same_bits(pyramids[j].plane(0, 1), eZ)
    fc = [forward_cases()[n] for n in MIXED_FORWARD]
    opt = dict(splat=ref.SPLAT_FOOTPRINT)
    views = [c.view if c.view is not None else (c.moving[2], W, H, 0.1) for c in fc]
    singles = [resident.pyramid(c.moving).warp_forward(c.T, v, 0, opt) for c, v in zip(fc, views)]
    for order in ([0, 1, 2, 3, 4], [3, 1, 4, 0, 2], [0, 1, 2, 3, 4]):
        d, i, x, cnt = gpu.warp_forward_many([resident.pyramid(fc[k].moving) for k in order], [fc[k].T for k in order],
                                             [views[k] for k in order], 0, opt)
        for j, k in enumerate(order):
            assert same_bits(d[j], singles[k][0]) and same_bits(i[j], singles[k][1]) and np.array_equal(x[j], singles[k][2]), (order, j)
            assert _counts(cnt[j], ref.FORWARD_COUNTS) == _counts(singles[k][3], ref.FORWARD_COUNTS)
        pyramids, pcnt = gpu.warp_forward_many([resident.pyramid(fc[k].moving) for k in order], [fc[k].T for k in order],
                                               [views[k] for k in order], None, opt)
        assert np.array_equal(pcnt, cnt)
        for j, k in enumerate(order):
            assert same_bits(pyramids[j].plane(0, 1), singles[k][0])
    # no item: nothing happens
    assert gpu.warp_inverse_many([], [], [], 0)[0] == [] and gpu.warp_forward_many([], [], None, 0)[0] == []
    assert gpu.warp_inverse_many([], [], [])[0] == [] and gpu.warp_forward_many([], [])[0] == []


@pytest.mark.gpu
def test_the_launch_counts(gpu, resident):
    """read from the call's own counters (dvo_amd_debug_warp_timing), not with a profiler: 1 launch for an inverse warp and 3 for a
    forward warp counting the clear, one synchronisation each, whatever n is"""
    ic = [inverse_cases()[n] for n in MIXED_INVERSE]
    fc = [forward_cases()[n] for n in MIXED_FORWARD]
    gpu.warp_timing(True)
    try:
        resident.inverse("synth_l2")
        got = gpu.warp_timing(True)
        assert (got["launches"], got["synchronisations"]) == (1, 1) and got["ms"] > 0.0
        gpu.warp_inverse_many([resident.pyramid(c.fixed) for c in ic], [resident.pyramid(c.moving) for c in ic], [c.T for c in ic], 0)
        got = gpu.warp_timing(True)
        assert (got["launches"], got["synchronisations"]) == (1, 1) and got["ms"] > 0.0
        resident.forward("synth_l2")
        got = gpu.warp_timing(True)
        assert (got["launches"], got["synchronisations"]) == (3, 1) and got["ms"] > 0.0
        gpu.warp_forward_many([resident.pyramid(c.moving) for c in fc], [c.T for c in fc], None, 0)
        got = gpu.warp_timing(True)
        assert (got["launches"], got["synchronisations"]) == (3, 1)
        resident.pyramid(ic[0].moving).warp_inverse(resident.pyramid(ic[0].fixed), ic[0].T)
        assert gpu.warp_timing(True)["launches"] == 1
        resident.pyramid(fc[0].moving).warp_forward(fc[0].T)
        assert gpu.warp_timing(True)["launches"] == 3
    finally:
        gpu.warp_timing(False)


@pytest.mark.gpu
def test_the_true_motion_aligns_the_frames(resident):
    f = frames()
    fixed, moving = resident.pyramid(f["synth_ref"]), resident.pyramid(f["far_cur"])
    at_T, at_I = moving.warp_inverse(fixed, f["far_T"], 0), moving.warp_inverse(fixed, np.eye(4), 0)
    a, b = [_mean_abs_difference(f["synth_ref"][0], got[0], np.where(np.isnan(got[0]), 0, ref.WARPED)) for got in (at_T, at_I)]
    print(f"mean |I_fixed - I_warped| over warped pixels: {a:.3f} at T, {b:.3f} at the identity")
    assert a < b
