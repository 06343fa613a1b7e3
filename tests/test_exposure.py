"""Exposure compensation (include/dvo_amd.h, "Exposure compensation"): dvo_amd_estimate_exposure / _many,
dvo_amd_pyramid_adjust_intensity / _many and DenseTracker.match_compensated.  The rule is pinned in the header and restated in
tests/exposure_ref.py.  Every comparison of the library with the restatement is equality: integers, doubles bit for bit (compared
as hex strings), float planes bit for bit.  The bars that are no equality are the issue's: a recovered gain within 2 % and a bias
within 2.5 grey levels of the truth, at least 0.7 of the consistent pixels used, a gain error beyond 40 % without refits on the
planted rectangle, and match_compensated at no more than half the pose error of the plain match.
CPU: the surface, the refusals that need no device, the vectorised restatement against its pixel loop, recovery, trimming and the
degenerate cases by the restatement alone, the host solve as a stand-alone program under UBSan.  GPU: the device's records and
planes against the restatement."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exposure_ref as er  # noqa: E402
import selection_mask_cases as cases  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_exposure_options", "dvo_amd_estimate_exposure", "dvo_amd_estimate_exposure_many",
               "dvo_amd_pyramid_adjust_intensity", "dvo_amd_pyramid_adjust_intensity_many"]
DEBUG_SYMBOLS = ["dvo_amd_debug_exposure_timing"]
INVALID, NO_DEVICE, DEVICE_MISMATCH = 1, 2, 8
EXPOSURES = ((1.0, 0.0), (1.3, -12.0), (0.7, 20.0), (1.6, 0.0))
GAIN_BAR, BIAS_BAR, USED_BAR = 0.02, 2.5, 0.7


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


def bits(record):
    """a record with every double as its hex string: equality of two such dicts is equality bit for bit"""
    h = lambda v: v.hex() if isinstance(v, float) else v  # noqa: E731
    return {k: [h(x) for x in v] if isinstance(v, list) else h(v) for k, v in record.items()}


# ---- CPU: the surface -----------------------------------------------------------------------------------------------------------

def _struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.sub(r"\[.*?\]", "", t).split()[-1] for t in [first] + rest]
    return names


def test_the_exports_and_the_structure_layouts_match_the_header(capi):
    L = capi.lib()
    for name in NEW_SYMBOLS + DEBUG_SYMBOLS:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS, name
    raw = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("dvo_amd.h", "dvo_amd_debug.h")}
    text = {h: re.sub(r"/\*.*?\*/", "", t, flags=re.S) for h, t in raw.items()}
    declared = {h: set(re.findall(r"\b(dvo_amd_[a-z0-9_]+)\s*\(", t)) for h, t in text.items()}
    assert sorted(capi.EXPORTS) == sorted(declared["dvo_amd.h"] | declared["dvo_amd_debug.h"])
    assert set(NEW_SYMBOLS) <= declared["dvo_amd.h"] and set(DEBUG_SYMBOLS) <= declared["dvo_amd_debug.h"]
    assert L.dvo_amd_abi_version() == 3
    assert "Exposure compensation" in raw["dvo_amd.h"] and "regression dilution" in raw["dvo_amd.h"]  # the low gain is stated
    assert "#define DVO_AMD_EXPOSURE_MAX_REFITS %d\n" % capi.EXPOSURE_MAX_REFITS in raw["dvo_amd.h"]
    assert [f[0] for f in capi.ExposureOptions._fields_] == _struct_fields(raw["dvo_amd.h"], "dvo_amd_exposure_options")
    assert [f[0] for f in capi.ExposureEstimate._fields_] == _struct_fields(raw["dvo_amd.h"], "dvo_amd_exposure_estimate")
    assert C.sizeof(capi.ExposureOptions) == 56 and capi.ExposureOptions.min_pairs.offset == 32 and capi.ExposureOptions.min_gain.offset == 40
    assert C.sizeof(capi.ExposureEstimate) == 392 and capi.ExposureEstimate.valid.offset == 32
    assert capi.ExposureEstimate.gain_pass.offset == 392 - 3 * 72
    assert set(capi.ExposureEstimate().as_dict()) == set(er.COUNTS + er.SUMS + ("gain", "bias", "r2", "passes", "degenerate", "gain_pass",
                                                                               "bias_pass", "used_pass"))
    assert capi.EXPOSURE_COUNTS == er.COUNTS and capi.EXPOSURE_SUMS == er.SUMS
    assert "dvo_exposure.cpp" in __import__("dvo_slam_amd._build", fromlist=["SOURCES"]).SOURCES


def test_the_default_options_are_the_documented_ones(capi):
    opt = capi.ExposureOptions()
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt))
    capi.lib().dvo_amd_default_exposure_options(C.byref(opt))
    got = {name: getattr(opt, name) for name, _ in capi.ExposureOptions._fields_}
    assert got == {k: (float(F(v)) if isinstance(v, float) and k not in ("min_gain", "max_gain") else v) for k, v in er.DEFAULTS.items()}
    capi.lib().dvo_amd_default_exposure_options(None)  # a no-op
    made = capi.exposure_options(level=2, trim=np.inf, refits=0, min_pairs=1 << 40, max_gain=2.5)
    assert (made.level, made.trim, made.refits, made.min_pairs, made.max_gain, made.scale) == (2, np.inf, 0, 1 << 40, 2.5, 16.0)
    with pytest.raises(TypeError):
        capi.exposure_options(gain=1.0)


class Fakes:
    """zeroed buffers that stand for a context, two pyramids and a mask: an argument error is reported before any of them is looked
    at beyond its head (refs, device, n_levels / w, h, levels lead them; the pyramids get two levels of size 0 x 0)"""

    def __init__(self, capi):
        self.keep = [C.create_string_buffer(1 << 20) for _ in range(4)]
        self.ctx, self.ref, self.cur, self.mask = [C.c_void_p(C.addressof(b)) for b in self.keep]
        C.c_int.from_buffer(self.keep[1], 8).value = 2
        C.c_int.from_buffer(self.keep[2], 8).value = 2
        C.c_int.from_buffer(self.keep[3], 16).value = 2  # a 0 x 0 mask of two levels: it fits
        self.T = (C.c_double * 16)(*np.eye(4).ravel())
        self.opt = capi.exposure_options(level=1)
        self.out = capi.ExposureEstimate()
        C.memset(C.byref(self.out), 0x5A, C.sizeof(self.out))

    def untouched(self):
        return bytes(self.out) == b"\x5a" * C.sizeof(self.out)


def test_estimate_argument_errors_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    f = Fakes(capi)
    single, many = "dvo_amd_estimate_exposure", "dvo_amd_estimate_exposure_many"

    def call(ctx=f.ctx, reference=f.ref, current=f.cur, T=f.T, mask=None, o=f.opt, out=f.out):
        return L.dvo_amd_estimate_exposure(ctx, reference, current, T, mask, None if o is None else C.byref(o), None if out is None else C.byref(out))

    one_r, one_c, null_in = (C.c_void_p * 1)(f.ref), (C.c_void_p * 1)(f.cur), (C.c_void_p * 1)(None)

    def call_many(n=1, ctx=f.ctx, references=one_r, currents=one_c, T=f.T, masks=None, o=f.opt, out=f.out):
        return L.dvo_amd_estimate_exposure_many(ctx, n, references, currents, T, masks, None if o is None else (capi.ExposureOptions * 1)(o),
                                                None if out is None else C.byref(out))

    def refused(entry, rc, what, word=None):
        assert rc == INVALID, (entry, what, rc)
        reason = L.dvo_amd_last_error().decode()
        assert reason.startswith(entry + ": "), (entry, what, reason)
        assert word is None or word in reason, (entry, what, reason)
        assert f.untouched(), (entry, what)

    for what, kw in {"ctx": dict(ctx=None), "reference": dict(reference=None), "current": dict(current=None), "options": dict(o=None),
                     "out": dict(out=None)}.items():
        refused(single, call(**kw), what, "NULL")
    for what, kw in {"ctx": dict(ctx=None), "references": dict(references=None), "currents": dict(currents=None), "options": dict(o=None),
                     "out": dict(out=None), "references[0]": dict(references=null_in), "currents[0]": dict(currents=null_in)}.items():
        refused(many, call_many(**kw), what, "NULL")
    refused(many, call_many(n=-1), "n", "n < 0")

    def with_option(**fields):
        bad = capi.ExposureOptions.from_buffer_copy(f.opt)
        for k, v in fields.items():
            setattr(bad, k, v)
        return bad

    for level in (-1, 2, 7, 8, 1 << 20):  # the pyramids have levels 0 and 1
        refused(single, call(o=with_option(level=level)), level, "level")
        refused(many, call_many(o=with_option(level=level)), level, "level")
    shallow = C.create_string_buffer(1 << 20)  # a current with one level: the reference's level 1 is missing there
    C.c_int.from_buffer(shallow, 8).value = 1
    refused(single, call(current=C.c_void_p(C.addressof(shallow))), "shallow", "level")
    big = C.create_string_buffer(1 << 20)  # a reference whose level 0 is 4096 x 1025: more than 2^22 pixels
    C.c_int.from_buffer(big, 8).value = 1
    C.c_int.from_buffer(big, 24).value, C.c_int.from_buffer(big, 28).value = 4096, 1025
    refused(single, call(reference=C.c_void_p(C.addressof(big)), o=with_option(level=0)), "big", "2^22")
    bad_options = {
        "near_z": (0.0, -1.0, np.nan, np.inf), "depth_sigmas": (-1.0, np.nan, np.inf), "scale": (0.0, -16.0, np.nan, np.inf),
        "min_intensity": (np.nan, -np.inf, 252.0, -65537.0), "max_intensity": (np.nan, np.inf, 3.0, 65537.0), "trim": (0.0, -1.0, np.nan),
        "refits": (-1, 9, 100), "min_pairs": (1, 0, -5), "min_gain": (0.0, -1.0, np.nan, np.inf, 5.0), "max_gain": (np.nan, np.inf, 0.2),
    }
    words = {"min_intensity": "intensity", "max_intensity": "intensity", "min_gain": "gain", "max_gain": "gain"}
    for field, values in bad_options.items():
        for v in values:
            refused(single, call(o=with_option(**{field: v})), (field, v), words.get(field, field))
            refused(many, call_many(o=with_option(**{field: v})), (field, v), words.get(field, field))
    refused(single, call(o=with_option(max_intensity=65535.0, scale=16.5)), "bound * scale", "2^20")
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 7, 15):
            T = (C.c_double * 16)(*np.eye(4).ravel())
            T[at] = bad
            refused(single, call(T=T), (bad, at), "transformation")
            refused(many, call_many(T=T), (bad, at), "transformation")
    misfit = C.create_string_buffer(1 << 20)  # an 8 x 8 mask on a 0 x 0 reference
    C.c_int.from_buffer(misfit, 8).value, C.c_int.from_buffer(misfit, 12).value, C.c_int.from_buffer(misfit, 16).value = 8, 8, 2
    refused(single, call(mask=C.c_void_p(C.addressof(misfit))), "mask size", "mask")
    refused(many, call_many(masks=(C.c_void_p * 1)(C.addressof(misfit))), "mask size", "mask")
    few = C.create_string_buffer(1 << 20)  # a mask with one level on a reference with two
    C.c_int.from_buffer(few, 16).value = 1
    refused(single, call(mask=C.c_void_p(C.addressof(few))), "mask levels", "mask")
    # a mask, a pyramid on another device: after every argument error, before the device is looked for
    C.c_int.from_buffer(f.keep[3], 4).value = 1
    assert call(mask=f.mask) == DEVICE_MISMATCH and call(mask=f.mask, o=with_option(trim=0.0)) == INVALID
    C.c_int.from_buffer(f.keep[3], 4).value = 0
    C.c_int.from_buffer(f.keep[2], 4).value = 1
    assert call() == DEVICE_MISMATCH and call_many() == DEVICE_MISMATCH and f.untouched()
    C.c_int.from_buffer(f.keep[2], 4).value = 0
    if L.dvo_amd_device_count() == 0:
        # nothing left to refuse: the device is looked for, and the record stays as it was
        for o in (f.opt, with_option(level=0, trim=np.inf, refits=8, min_pairs=2), with_option(max_intensity=65536.0, scale=16.0),
                  with_option(min_intensity=-100.0, max_intensity=-50.0), with_option(min_gain=1.0, max_gain=1.0)):
            assert call(o=o) == NO_DEVICE and call_many(o=o) == NO_DEVICE
        assert call(T=None) == NO_DEVICE and call(mask=f.mask) == NO_DEVICE and call_many(masks=(C.c_void_p * 1)(None)) == NO_DEVICE
        assert call_many(n=0) == NO_DEVICE
        assert f.untouched()


def test_adjust_argument_errors_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    f = Fakes(capi)
    single, many = "dvo_amd_pyramid_adjust_intensity", "dvo_amd_pyramid_adjust_intensity_many"
    dp = C.POINTER(C.c_double)
    marker = 0x5A5A5A5A

    def refused(entry, rc, out, what, word):
        assert rc == INVALID, (entry, what, rc)
        reason = L.dvo_amd_last_error().decode()
        assert reason.startswith(entry + ": ") and word in reason, (entry, what, reason)
        assert out is None or not out[0], (entry, what)  # NULL on failure

    def fresh():
        return (C.c_void_p * 2)(marker, marker)

    out = fresh()
    refused(single, L.dvo_amd_pyramid_adjust_intensity(None, 1.0, 0.0, out), out, "p", "NULL")
    refused(single, L.dvo_amd_pyramid_adjust_intensity(f.ref, 1.0, 0.0, None), None, "out", "NULL")
    for g, b in ((np.nan, 0.0), (np.inf, 0.0), (1.0, np.nan), (1.0, -np.inf)):
        out = fresh()
        refused(single, L.dvo_amd_pyramid_adjust_intensity(f.ref, g, b, out), out, (g, b), "finite")
    ps, one, zero = (C.c_void_p * 2)(f.ref, f.cur), (C.c_double * 2)(1.0, 1.5), (C.c_double * 2)(0.0, -3.0)
    for what, args in {"p": (2, None, one, zero), "gain": (2, ps, None, zero), "bias": (2, ps, one, None)}.items():
        out = fresh()
        refused(many, L.dvo_amd_pyramid_adjust_intensity_many(*args, out), out, what, "NULL")
    refused(many, L.dvo_amd_pyramid_adjust_intensity_many(2, ps, one, zero, None), None, "out", "NULL")
    refused(many, L.dvo_amd_pyramid_adjust_intensity_many(-1, ps, one, zero, fresh()), None, "n", "n < 0")
    out = fresh()
    refused(many, L.dvo_amd_pyramid_adjust_intensity_many(2, (C.c_void_p * 2)(f.ref, None), one, zero, out), out, "p[1]", "NULL")
    assert not out[1]
    out = fresh()
    refused(many, L.dvo_amd_pyramid_adjust_intensity_many(2, ps, (C.c_double * 2)(1.0, np.nan), zero, out), out, "gain[1]", "finite")
    C.c_int.from_buffer(f.keep[2], 4).value = 1  # the second pyramid on another device
    out = fresh()
    assert L.dvo_amd_pyramid_adjust_intensity_many(2, ps, one, zero, out) == DEVICE_MISMATCH and not out[0] and not out[1]
    C.c_int.from_buffer(f.keep[2], 4).value = 0
    if L.dvo_amd_device_count() == 0:
        out = fresh()
        assert L.dvo_amd_pyramid_adjust_intensity_many(2, ps, one, zero, out) == NO_DEVICE and not out[0] and not out[1]
        assert L.dvo_amd_pyramid_adjust_intensity(f.ref, 0.0, 1e30, out) == NO_DEVICE  # any finite pair is taken
        assert L.dvo_amd_pyramid_adjust_intensity_many(0, ps, one, zero, out) == NO_DEVICE
        with pytest.raises(capi.DvoAmdError):
            capi.exposure_timing(True)
    assert capi.exposure_timing(False) == 0.0  # switching the bracket off needs no device


# ---- CPU: the restatement -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pairs(synth):
    """the issue's four exposures of the 160x120 pair: {(g, b): (planes_ref, planes_cur, T_true)}, computed once and left unchanged"""
    out = {}
    for g, b in EXPOSURES:
        ref, cur, T_gt, K = er.exposure_pair(synth, g, b)
        out[(g, b)] = ((ref[0], ref[1], K), (cur[0], cur[1], K), np.linalg.inv(T_gt))
    return out


def looking_back(T):
    """T followed by half a turn about the current camera's y axis: everything lands behind it"""
    return np.diag([-1.0, 1.0, -1.0, 1.0]) @ np.asarray(T, np.float64)


def small_cases(synth):
    """pairs small enough for the pixel loop: 40x30 under three transformations and a mask, a 36x20 reference with a 24x18 current of
    other intrinsics, a pair with NaN and out-of-range intensities"""
    ref, cur, T_gt, _ = er.exposure_pair(synth, 1.3, -12.0, w=40, h=30)
    K = synth.intrinsics_for(40, 30)
    a, b, T = (ref[0], ref[1], K), (cur[0], cur[1], K), np.linalg.inv(T_gt)
    mask = (np.add.outer(np.arange(30), np.arange(40)) % 3 != 0).astype(np.uint8)
    few = dict(min_pairs=8)
    yield "true", a, b, T, None, few
    yield "identity", a, b, None, None, dict(few, refits=1, trim=3.0)
    yield "masked", a, b, T, mask, dict(few, refits=8, trim=2.0, scale=3.7)
    yield "all masked", a, b, T, np.zeros((30, 40), np.uint8), few
    yield "half behind", a, b, looking_back(T) @ synth.se3_exp([0, 0, 0, 0, 1.2, 0]), None, few
    yield "behind", a, b, looking_back(T), None, few
    K2 = tuple(F(k) for k in (31.0, 29.5, 12.7, 8.2))
    gc, zc = synth.sensor_frame(24, 18, T_gt, K=K2, frame_id=1)
    Ic, Zc = synth.raw_to_float(gc, zc)
    r2 = synth.raw_to_float(*synth.sensor_frame(36, 20, None, K=synth.intrinsics_for(36, 20)))
    yield "mixed cameras", (r2[0], r2[1], synth.intrinsics_for(36, 20)), (Ic, Zc, K2), T, None, dict(few, near_z=0.5, depth_sigmas=3.0)
    Ib = cur[0].copy()
    Ib[5:9, :] = np.nan
    Ib[12:14, :] = 255.0
    Ib[20, :] = 0.0
    yield "saturated", a, (Ib, cur[1], K), T, None, dict(few, min_intensity=20.0, max_intensity=200.0)
    yield "degenerate in pass 1", a, b, T, None, dict(min_pairs=64, trim=0.01)
    yield "gain out of range", a, b, T, None, dict(few, min_gain=0.9)


def test_the_vectorised_restatement_equals_the_pixel_loop(synth):
    seen = set()
    for name, a, b, T, mask, options in small_cases(synth):
        fast, slow = er.estimate_ref(a, b, T, mask, options), er.estimate_brute(a, b, T, mask, options)
        assert bits(fast) == bits(slow), name
        assert fast["valid"] == sum(fast[k] for k in er.COVIS[1:]) and fast["consistent"] == fast["masked"] + fast["saturated"] + fast["candidates"]
        assert fast["candidates"] == fast["used"] + fast["trimmed"] and fast["n"] == fast["used"] == fast["used_pass"][fast["passes"] - 1]
        seen.add((fast["degenerate"], fast["passes"] > 1, fast["behind"] > 0, fast["masked"] > 0, fast["saturated"] > 0, fast["trimmed"] > 0))
    # the cases reach what they are there for
    assert {s[0] for s in seen} == {0, 1, 3} and any(s[0] == 1 and s[1] for s in seen)
    assert all(any(s[i] for s in seen) for i in (2, 3, 4, 5))


def test_the_restatement_recovers_a_known_exposure(pairs):
    worst = dict(gain=0.0, bias=0.0, share=1.0)
    for (g, b), (a, c, T_true) in pairs.items():
        for T in (T_true, None):
            r = er.estimate_ref(a, c, T)
            gain_error, bias_error, share = abs(r["gain"] * g - 1.0), abs(r["bias"] + b / g), r["used"] / r["consistent"]
            print(f"exposure ({g}, {b}) at {'the identity' if T is None else 'the true T'}: gain {r['gain']:.5f} (true {1 / g:.5f}, "
                  f"error {100 * gain_error:.2f} %), bias {r['bias']:.3f} (true {-b / g:.3f}, error {bias_error:.2f}), used {share:.3f}")
            assert r["degenerate"] == 0 and r["passes"] == 5
            assert gain_error <= GAIN_BAR and bias_error <= BIAS_BAR and share >= USED_BAR, (g, b, T is None)
            assert r["gain"] * g < 1.0  # least squares of y on a noisy x: the gain comes out low (stated in the header)
            worst = dict(gain=max(worst["gain"], gain_error), bias=max(worst["bias"], bias_error), share=min(worst["share"], share))
    print("worst:", worst)


def planted(I):
    out = I.copy()
    out[30:75, 40:100] = F(255.0) - out[30:75, 40:100]
    return out


def test_the_refits_trim_a_planted_rectangle(synth):
    ref, cur, T_gt, K = er.exposure_pair(synth, 1.3, -12.0, edit=planted)
    a, c, T = (ref[0], ref[1], K), (cur[0], cur[1], K), np.linalg.inv(T_gt)
    once, fitted = er.estimate_ref(a, c, T, options=dict(refits=0)), er.estimate_ref(a, c, T)
    print("refits 0:", once["gain"], once["bias"], " refits 4:", fitted["gain"], fitted["bias"], " true:", 1 / 1.3, 12 / 1.3)
    assert once["passes"] == 1 and abs(once["gain"] * 1.3 - 1.0) > 0.40
    assert fitted["passes"] == 5 and abs(fitted["gain"] * 1.3 - 1.0) <= GAIN_BAR and abs(fitted["bias"] - 12.0 / 1.3) <= BIAS_BAR
    assert fitted["trimmed"] >= 0.8 * 45 * 60 * 0.9  # most of the rectangle is gone


def test_the_degenerate_cases_return_one_and_zero_with_their_code(pairs):
    a, c, T = pairs[(1.0, 0.0)]
    flat = (np.full_like(c[0], 100.0), c[1], c[2])
    dark = (np.full_like(c[0], 2.0), c[1], c[2])
    for name, cur, options, code in (("a constant image", flat, None, 2), ("everything saturated", dark, None, 1),
                                     ("a gain outside the range", c, dict(max_gain=0.9), 3)):
        r = er.estimate_ref(a, cur, T, options=options)
        assert (r["gain"], r["bias"], r["r2"], r["degenerate"], r["passes"]) == (1.0, 0.0, 0.0, code, 1), name
        assert (r["gain_pass"][0], r["bias_pass"][0]) == (1.0, 0.0) and r["used_pass"][0] == r["used"]
    assert er.estimate_ref(a, dark, T)["saturated"] == er.estimate_ref(a, dark, T)["consistent"] > 0
    assert er.solve_ref(63, 1, 1, 1, 1, 1)[3] == 1 and er.solve_ref(64, 64, 64, 64, 64, 64)[3] == 2  # n < min_pairs; det = 0


# ---- CPU: the host solve as a stand-alone program under UBSan ---------------------------------------------------------------------

def _sanitized_solve(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++11", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all"]
    if subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no UBSan runtime")
    exe = tmp_path / "exposure_solve"
    res = subprocess.run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "dvo_slam_amd", "csrc"),
                                          os.path.join(ROOT, "tests", "exposure_solve_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return str(exe)


def test_the_host_solve_is_clean_under_ubsan_at_the_bound_and_equals_python_integers(tmp_path):
    exe = _sanitized_solve(tmp_path)
    N, Q = 1 << 22, 1 << 20
    rng = np.random.default_rng(11)
    sums = [
        (N, N * Q, N * Q, N * Q * Q, N * Q * Q, N * Q * Q),                  # every pair at (2^20, 2^20): sxx = 2^62, det = 0
        (N, N * Q - Q, N * Q // 2, N * Q * Q - Q * Q, (N * Q * Q) // 2, N * Q * Q),  # at the bound with det > 0
        (N, -N * Q + 5, N * Q - 3, N * Q * Q, -(N * Q * Q) + 7 * Q, N * Q * Q),      # negative intensities: sx < 0, sxy < 0
        (63, 100, 100, 1000, 1000, 1000), (2, 0, 0, 0, 0, 0), (1158, 2823776, 2342304, 7352024064, 6068791808, 5015205376),
    ]
    for _ in range(40):  # sums of random pairs near the bound: exact by construction
        n = int(rng.integers(2, 200))
        X, Y = [rng.integers(Q - 4096, Q + 1, n).astype(object) * int(s) for s in rng.choice([-1, 1], 2)]
        w = N // n  # every pair w times: n w <= 2^22
        sums.append((n * w, int(X.sum()) * w, int(Y.sum()) * w, int((X * X).sum()) * w, int((X * Y).sum()) * w, int((Y * Y).sum()) * w))
    options = [dict(), dict(min_gain=1e-6, max_gain=1e6, scale=0.37), dict(min_pairs=2, min_gain=0.999, max_gain=1.001)]
    wides = [0, 1, -1, (1 << 53) + 1, (1 << 64) - 1, 1 << 64, (1 << 64) + 1, (1 << 117) + (1 << 64), (1 << 117) + (1 << 64) + 1,
             -((1 << 105) + (1 << 52)), -((1 << 105) + (1 << 52) + 1), (1 << 127) - 1, -(1 << 126) - 12345, (1 << 104) - 1,
             ((1 << 53) + 1) << 40, (((1 << 53) + 1) << 40) + 1, (((1 << 53) + 3) << 40) - 1]
    wides += [int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) * int(s) for s in rng.choice([-1, 1], 60)]
    lines, want = [], []
    for s in sums:
        for o in options:
            full = dict(er.DEFAULTS, **o)
            lines.append("s " + " ".join(str(v) for v in s) + " %d %r %r %r" % (full["min_pairs"], full["min_gain"], full["max_gain"],
                                                                                float(F(full["scale"]))))
            gain, bias, r2, code = er.solve_ref(*s, options=o)
            want.append("%s %s %s %d" % (gain.hex(), bias.hex(), r2.hex(), code))
    for v in wides:
        lines.append("d %d" % v)
        want.append(float(v).hex())
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0 and "runtime error" not in res.stderr, res.stderr
    got = [" ".join(float.fromhex(t).hex() if "x" in t else t for t in ln.split()) for ln in res.stdout.strip().splitlines()]
    assert got == want
    assert {w.split()[-1] for w in want[:len(sums) * len(options)]} >= {"0", "1", "2", "3"}  # every outcome of rule 8 was reached


# ---- GPU: the estimate against the restatement ------------------------------------------------------------------------------------

def planes(p, level):
    return p.plane(level, 0), p.plane(level, 1), p.level_info(level)[2]


class Scenes:
    """the pyramids of the GPU tests, built once per module, only read"""

    def __init__(self, capi, synth, pairs):
        self.capi = capi
        self.trk = capi.DenseTracker(capi.Config())
        a, c, self.T = pairs[(1.3, -12.0)]
        K = a[2]
        self.ref = capi.RgbdImagePyramid(a[0], a[1], K, 4, timestamp=12.5)
        self.cur = capi.RgbdImagePyramid(c[0], c[1], K, 4, timestamp=13.5)
        # 68x36, one level: the width is no multiple of a wave, the 2448 pixels no multiple of a block
        ref, cur, T_gt, _ = er.exposure_pair(synth, 0.7, 20.0, w=68, h=36)
        Ks = synth.intrinsics_for(68, 36)
        self.small_ref, self.small_cur = capi.RgbdImagePyramid(ref[0], ref[1], Ks, 1), capi.RgbdImagePyramid(cur[0], cur[1], Ks, 1)
        # an 80x60 current of other intrinsics for the 160x120 reference
        k = synth.intrinsics_for(80, 60)
        K2 = (F(k[0] * 1.1), F(k[1] * 1.05), F(k[2] + 1.5), F(k[3] - 1.0))
        Ic, Zc = synth.raw_to_float(*synth.sensor_frame(80, 60, np.linalg.inv(self.T), K=K2, frame_id=1))
        self.other_cur = capi.RgbdImagePyramid(F(1.0 / 1.3) * Ic + F(9.0), Zc, K2, 3)
        m0 = np.ones((120, 160), bool)  # (whole 8x8 cells: level 3 of the mask keeps pixels too)
        m0[:, :24] = False
        m0[40:80, 64:96] = False
        self.mask = capi.SelectionMask.from_level0(m0, 4)
        self.no_mask = capi.SelectionMask.from_level0(np.zeros((120, 160), np.uint8), 4)
        self.small_mask = capi.SelectionMask.from_level0(np.arange(68 * 36).reshape(36, 68) % 7 != 0, 1)

    def want(self, reference, current, T, mask, options):
        o = dict(er.DEFAULTS, **(options or {}))
        m = None if mask is None else mask.download(o["level"])
        return er.estimate_ref(planes(reference, o["level"]), planes(current, o["level"]), T, m, o)


@pytest.fixture(scope="module")
def scenes(capi, synth, pairs):
    return Scenes(capi, synth, pairs)


def check(s, reference, current, T=None, mask=None, options=None):
    got = current.estimate_exposure(reference, T=T, mask=mask, options=options, tracker=s.trk).as_dict()
    want = s.want(reference, current, T, mask, options)
    assert bits(got) == bits(want), (options, got, want)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 3])
def test_gpu_the_record_equals_the_restatement_under_every_transformation_and_mask(scenes, level):
    s = scenes
    for T in (None, s.T, looking_back(s.T)):
        for mask in (None, s.mask, s.no_mask):
            got = check(s, s.ref, s.cur, T, mask, dict(level=level, min_pairs=16))
            if T is not None and T is not s.T:
                assert got["behind"] == got["valid"] > 0 and got["degenerate"] == 1
            elif mask is s.no_mask:
                assert got["masked"] == got["consistent"] > 0 and got["degenerate"] == 1 and (got["gain"], got["bias"]) == (1.0, 0.0)
            else:
                assert got["degenerate"] == 0 and got["passes"] == 5 and (mask is None) == (got["masked"] == 0)
    fitted = check(s, s.ref, s.cur, s.T, None, dict(level=level))
    if level == 0:
        assert abs(fitted["gain"] * 1.3 - 1.0) <= GAIN_BAR and abs(fitted["bias"] - 12.0 / 1.3) <= BIAS_BAR


@pytest.mark.gpu
def test_gpu_a_level_that_fills_neither_a_wave_nor_a_block(scenes):
    s = scenes
    assert s.small_ref.level_info(0)[:2] == (68, 36)
    for mask in (None, s.small_mask):
        for options in (None, dict(refits=0), dict(refits=8, trim=3.0, scale=5.3, min_intensity=30.0, max_intensity=220.0)):
            got = check(s, s.small_ref, s.small_cur, None, mask, options)
            assert got["degenerate"] == 0 and got["valid"] > 2000


@pytest.mark.gpu
def test_gpu_mixed_cameras(scenes):
    s = scenes
    for level in (0, 2):
        for T in (None, s.T):
            got = check(s, s.ref, s.other_cur, T, s.mask if level else None, dict(level=level, min_pairs=16))
            assert got["consistent"] > 0 and got["degenerate"] == 0
    with pytest.raises(s.capi.DvoAmdError) as e:  # level 3 exists in the reference alone
        s.other_cur.estimate_exposure(s.ref, options=dict(level=3), tracker=s.trk)
    assert e.value.status == INVALID


@pytest.mark.gpu
def test_gpu_a_pair_that_goes_degenerate_in_pass_1_but_not_in_pass_0(scenes):
    # a trim of a fifth of a grey level leaves pass 1 the few hundred pixels that pass 0's line happens to meet: fewer than min_pairs
    got = check(scenes, scenes.ref, scenes.cur, scenes.T, None, dict(trim=0.2, min_pairs=6000))
    assert (got["passes"], got["degenerate"], got["gain"], got["bias"]) == (2, 1, 1.0, 0.0)
    assert got["gain_pass"][0] not in (0.0, 1.0) and got["used_pass"][0] == got["candidates"] > 6000 > got["used_pass"][1] > 0
    assert (got["gain_pass"][1], got["bias_pass"][1], got["used"], got["n"]) == (1.0, 0.0, got["used_pass"][1], got["used_pass"][1])
    ranged = check(scenes, scenes.ref, scenes.cur, scenes.T, None, dict(max_gain=0.5))
    assert (ranged["passes"], ranged["degenerate"]) == (1, 3)


@pytest.mark.gpu
def test_gpu_the_accumulators_are_64_bits_wide(capi, synth, scenes):
    w = h = 68
    rng = np.random.default_rng(3)
    Ir = rng.uniform(60000.0, 65535.0, (h, w)).astype(F)
    Ic = np.minimum(F(65535.0), Ir * F(0.999) + rng.uniform(-20.0, 20.0, (h, w)).astype(F))
    Z = np.full((h, w), 2.0, F)
    K = synth.intrinsics_for(w, h)
    ref, cur = capi.RgbdImagePyramid(Ir, Z, K, 1), capi.RgbdImagePyramid(Ic, Z, K, 1)
    got = check(scenes, ref, cur, None, None, dict(scale=16.0, max_intensity=65535.0, trim=np.inf, min_gain=0.5, max_gain=2.0))
    assert got["sxx"] > 1 << 50 and got["syy"] > 1 << 50 and got["used"] == w * h and got["degenerate"] == 0
    assert abs(got["gain"] - 1.0) < 0.05


def batch_of_40(s):
    combos = [(s.ref, s.cur, s.mask, 4), (s.small_ref, s.small_cur, s.small_mask, 1), (s.ref, s.other_cur, s.no_mask, 3),
              (s.cur, s.ref, s.mask, 4), (s.small_cur, s.small_ref, None, 1)]
    references, currents, Ts, masks, options = [], [], [], [], []
    for k in range(40):
        reference, current, mask, levels = combos[k % len(combos)]
        references.append(reference), currents.append(current)
        Ts.append((np.eye(4), s.T, np.linalg.inv(s.T), looking_back(s.T))[(k // 5) % 4 if k % 11 else 3])
        masks.append(mask if k % 3 == 0 else None)
        options.append(dict(level=k % levels, refits=k % 9, trim=(12.0, 3.0, np.inf, 0.01)[k % 4], scale=(16.0, 1.0, 7.25)[k % 3],
                            min_pairs=(64, 2, 500)[k % 3], min_intensity=(4.0, 40.0)[k % 2], max_intensity=(251.0, 180.0)[(k // 2) % 2],
                            depth_sigmas=(20.0, 2.0)[(k // 3) % 2]))
    return references, currents, Ts, masks, options


@pytest.mark.gpu
def test_gpu_forty_pairs_in_one_call_equal_forty_single_calls_and_two_runs_are_identical(capi, scenes):
    s = scenes
    references, currents, Ts, masks, options = batch_of_40(s)
    together = [e.as_dict() for e in capi.estimate_exposure_many(s.trk, references, currents, Ts, masks, options)]
    again = [e.as_dict() for e in capi.estimate_exposure_many(s.trk, references, currents, Ts, masks, options)]
    assert [bits(r) for r in together] == [bits(r) for r in again]
    for k in range(40):
        alone = currents[k].estimate_exposure(references[k], T=Ts[k], mask=masks[k], options=options[k], tracker=s.trk).as_dict()
        assert bits(alone) == bits(together[k]), k
        if k % 4 == 0:  # (ten of them against the restatement as well: every size, the mask, every T)
            assert bits(together[k]) == bits(s.want(references[k], currents[k], Ts[k], masks[k], options[k])), k
    assert len({r["passes"] for r in together}) >= 5 and {r["degenerate"] for r in together} >= {0, 1}
    # the identity given equals no transformation given
    first = capi.estimate_exposure_many(s.trk, references[:5], currents[:5], None, masks[:5], options[:5])
    given = capi.estimate_exposure_many(s.trk, references[:5], currents[:5], [np.eye(4)] * 5, masks[:5], options[:5])
    assert [bits(e.as_dict()) for e in first] == [bits(e.as_dict()) for e in given]


@pytest.mark.gpu
def test_gpu_an_empty_call_does_nothing_and_the_shared_context_serves(capi, scenes):
    s = scenes
    assert capi.estimate_exposure_many(s.trk, [], [], None, None, None) == []
    assert capi.estimate_exposure_many(s.trk, [], [], [], [], []) == []
    assert capi.adjust_intensity_many([], [], []) == []
    shared = s.cur.estimate_exposure(s.ref, T=s.T).as_dict()  # no tracker given
    assert bits(shared) == bits(s.want(s.ref, s.cur, s.T, None, None))
    capi.exposure_timing(True)
    s.cur.estimate_exposure(s.ref, T=s.T, tracker=s.trk)
    assert capi.exposure_timing(False) > 0.0


# ---- GPU: the adjustment ----------------------------------------------------------------------------------------------------------

def all_planes(p):
    return [[p.plane(l, k) for k in range(6)] for l in range(p.levels())]


def same_planes(a, b):
    return len(a) == len(b) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for la, lb in zip(a, b) for x, y in zip(la, lb))


@pytest.mark.gpu
def test_gpu_the_adjusted_pyramid_is_the_one_pyramid_create_makes_of_the_restated_planes(capi, scenes):
    s = scenes
    items = [(s.cur, 1.0 / 1.3, 12.0 / 1.3), (s.small_cur, 1.43, -27.0), (s.other_cur, 0.0, 17.0), (s.ref, -1.0, 255.0),
             (s.small_ref, 1.0, 0.0), (s.cur, 1e-3, -1e4), (s.ref, 3.999, 0.125), (s.other_cur, 1.0000001, 1e-7)]
    before = [all_planes(p) for p, _, _ in items]
    single = items[0][0].adjust_intensity(items[0][1], items[0][2])
    many = capi.adjust_intensity_many([p for p, _, _ in items], [g for _, g, _ in items], [b for _, _, b in items])
    for k, ((p, g, b), made) in enumerate(zip(items, [single] + many[1:])):
        w, h, K = p.level_info(0)
        restated = capi.RgbdImagePyramid(er.adjust_ref(p.plane(0, 0), g, b), p.plane(0, 1), K, p.levels(), timestamp=p.timestamp())
        assert made.levels() == p.levels() and made.timestamp() == p.timestamp() and made.level_info(0)[:2] == (w, h)
        assert all(np.array_equal(made.level_info(l)[2], restated.level_info(l)[2]) for l in range(p.levels()))
        assert same_planes(all_planes(made), all_planes(restated)), k
        assert np.array_equal(made.plane(0, 1).view(np.uint32), p.plane(0, 1).view(np.uint32))  # the input's depth, bit for bit
    assert same_planes(all_planes(many[0]), all_planes(single))
    assert same_planes(all_planes(many[4]), before[4])  # (1, 0) changes no bit
    assert all(same_planes(all_planes(p), planes_before) for (p, _, _), planes_before in zip(items, before))  # the inputs are unchanged
    restated = capi.RgbdImagePyramid(er.adjust_ref(s.cur.plane(0, 0), items[0][1], items[0][2]), s.cur.plane(0, 1), s.cur.level_info(0)[2], 4)
    assert cases.same_result(s.trk.match(s.ref, single), s.trk.match(s.ref, restated))


# ---- GPU: end to end --------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_gpu_match_compensated_halves_the_pose_error_of_an_exposure_step(capi, synth, pairs, scenes):
    """the (0.7, +20) pair of the issue's table: the oracle's plain match ends at 1.12e-2, its compensated one at 9.2e-4"""
    a, c, T = pairs[(0.7, 20.0)]
    T_gt = np.linalg.inv(T)
    reference, current = capi.RgbdImagePyramid(a[0], a[1], a[2], 4), capi.RgbdImagePyramid(c[0], c[1], c[2], 4)
    trk = scenes.trk
    plain = trk.match(reference, current)
    result, estimates, adjusted = trk.match_compensated(reference, current)
    plain_error, compensated_error = synth.pose_error(T_gt, plain.Transformation), synth.pose_error(T_gt, result.Transformation)
    print(f"pose error: plain {plain_error:.3e}, compensated {compensated_error:.3e}; estimate {estimates[0].gain:.4f}, {estimates[0].bias:.2f}")
    assert not plain.isNaN() and not result.isNaN() and len(estimates) == 1
    assert bits(estimates[0].as_dict()) == bits(er.estimate_ref(a, c, None))  # (level 0's planes are the frames themselves)
    assert cases.same_result(result, trk.match(reference, current.adjust_intensity(estimates[0].gain, estimates[0].bias)))
    assert same_planes(all_planes(adjusted), all_planes(current.adjust_intensity(estimates[0].gain, estimates[0].bias)))
    assert compensated_error <= 0.5 * plain_error
    seeded = capi.DenseTracker(capi.Config(UseInitialEstimate=True))
    twice, two, _ = seeded.match_compensated(reference, current, T_init=np.eye(4), rounds=2)  # (such a tracker wants a start)
    assert len(two) == 2 and bits(two[0].as_dict()) == bits(estimates[0].as_dict()) and not twice.isNaN()
    first = seeded.match(reference, current.adjust_intensity(two[0].gain, two[0].bias), T_init=np.eye(4))
    assert bits(two[1].as_dict()) == bits(er.estimate_ref(a, c, capi.rigid_inverse(first.Transformation)))
    print(f"two rounds: {synth.pose_error(T_gt, twice.Transformation):.3e}; second estimate {two[1].gain:.4f}, {two[1].bias:.2f}")
