"""Depth fusion on the device (include/dvo_amd.h, "Depth fusion"): dvo_amd_pyramid_fuse_depth and dvo_amd_pyramid_fuse_depth_many.
The rule is pinned in the header and restated in tests/depth_fusion_ref.py.  Every comparison with the library is equality -- of
float planes bit for bit (NaN positions included), of byte planes, of integer counts, of tracking results.  The one inequality is
the gain: nine observations must beat the noise of four.
CPU: exports and layout, the argument checks that need no device, the restatement against its pixel loop, the convention on a
case whose arithmetic is exact, the gain, the coverage of the scenes.  GPU: the library against the restatement."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depth_fusion_ref as ref  # noqa: E402
import selection_mask_cases as cases  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_fuse_options", "dvo_amd_pyramid_fuse_depth", "dvo_amd_pyramid_fuse_depth_many",
               "dvo_amd_debug_fuse_timing"]
INVALID, NO_DEVICE, MISMATCH = 1, 2, 8
SAMPLES = {"bilinear": ref.BILINEAR, "nearest": ref.NEAREST}
# (depth_sigmas, min_observations, drop_unconfirmed)
GRID = [(sigmas, min_obs, drop) for sigmas in (3.0, 20.0) for min_obs in (0, 2) for drop in (0, 1)]


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


# ---- the scenes: (I, Z, K, levels) of the keyframe and of every frame, and T[k]: frame k's camera -> the keyframe's ------------------

class Scene:
    def __init__(self, key, frames, Ts):
        self.key, self.frames, self.Ts = key, list(frames), [np.asarray(T, np.float64) for T in Ts]

    def planes(self):
        """what the restatement takes: the keyframe's (Z, K) and the frames'"""
        return (self.key[1], self.key[2]), [(f[1], f[2]) for f in self.frames]

    def ref(self, **opt):
        return _scene_ref(self, tuple(sorted(opt.items())))


@functools.lru_cache(maxsize=None)
def _scene_ref(scene, opt):
    """the restated (fused, observations, frame counts, keyframe counts): computed once per option set, shared"""
    key, frames = scene.planes()
    out = ref.fuse_ref(key, frames, scene.Ts, dict(opt))
    out[0].setflags(write=False), out[1].setflags(write=False)
    return out


def _sensor(synth, w, h, pose, frame_id, K=None):
    grey, raw = synth.sensor_frame(w, h, pose, frame_id=frame_id, K=K)
    return synth.raw_to_float(grey, raw)


def _y_rotation(deg, t):
    a = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    T[:3, 3] = t
    return T


@functools.lru_cache(maxsize=None)
def scenes():
    from dvo_slam_amd import synth

    poses = [synth.se3_exp(t * synth.XI_STEP_STREAM) for t in range(9)]
    out = {}
    # the stream of the issue: a 160x120 four-level keyframe and the 8 frames that follow it, as a sensor delivers them
    w, h = 160, 120
    K = synth.intrinsics_for(w, h)
    stream = [_sensor(synth, w, h, poses[t], t) + (K, 4) for t in range(9)]
    out["stream"] = Scene(stream[0], stream[1:], poses[1:])
    # a one-level 68x36 keyframe: its width is no multiple of a wave (rows straddle waves), and its 2448 pixels are no multiple of
    # a block's 512 (nor of 1024): the last block is partial
    ws, hs = 68, 36
    Ks = synth.intrinsics_for(ws, hs)
    small = [_sensor(synth, ws, hs, poses[2 * t], 20 + t) + (Ks, 1) for t in range(4)]
    out["small"] = Scene(small[0], small[1:], [poses[2], poses[4], poses[6]])
    # the 160x120 keyframe with 80x60 frames of another camera (two levels: fewer than the keyframe has)
    Kh = tuple(F(k) for k in (F(1.1) * synth.intrinsics_for(80, 60)[0], F(0.95) * synth.intrinsics_for(80, 60)[1], F(41.5), F(28.25)))
    half = [_sensor(synth, 80, 60, poses[t], 40 + t, K=Kh) + (Kh, 2) for t in (1, 3, 5)]
    out["mixed"] = Scene(stream[0], half, [poses[1], poses[3], poses[5]])
    out["none"] = Scene(stream[0], [], [])
    out["repeated"] = Scene(stream[0], [stream[3]] * 255, [poses[3]] * 255)
    # the keyframe among its own frames, and more frames than one batch of the kernel's counters holds (32), all different poses
    out["cycle"] = Scene(stream[0], [stream[t % 9] for t in range(40)], [poses[t % 9] for t in range(40)])
    # behind: a frame half a metre in front of the far wall (z = 3), looking back at the keyframe
    wb, hb = 80, 60
    Kb = synth.intrinsics_for(wb, hb)
    key_b = synth.render(wb, hb, np.eye(4), frame_id=60) + (Kb, 2)
    back = _y_rotation(180.0, [0.0, 0.0, 2.5])
    out["behind"] = Scene(key_b, [synth.render(wb, hb, back, frame_id=61) + (Kb, 2)], [back])
    # grazing: a frame to the right of the keyframe looking across its view: along the keyframe's rays its depth grows slowly
    side = _y_rotation(-75.0, [1.0, 0.0, 2.0])
    out["grazing"] = Scene(key_b, [synth.render(wb, hb, side, frame_id=62) + (Kb, 2)], [side])
    return out


def _opt(sample, sigmas, min_obs, drop, **more):
    return dict(sample=sample, depth_sigmas=sigmas, min_observations=min_obs, drop_unconfirmed=drop, **more)


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
    assert (capi.FUSE_BILINEAR, capi.FUSE_NEAREST, capi.FUSE_MAX_FRAMES) == (ref.BILINEAR, ref.NEAREST, ref.MAX_FRAMES) == (0, 1, 255)
    assert capi.FUSE_FRAME_COUNTS == ref.FRAME_COUNTS and capi.FUSE_FRAME_DTYPE.itemsize == 64
    assert capi.FUSE_KEYFRAME_COUNTS == ref.KEYFRAME_COUNTS and capi.FUSE_KEYFRAME_DTYPE.itemsize == 32
    header = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    for define, value in (("DVO_AMD_FUSE_MAX_FRAMES", 255), ("DVO_AMD_FUSE_FRAME_COUNTS", 8), ("DVO_AMD_FUSE_KEYFRAME_COUNTS", 4),
                          ("DVO_AMD_FUSE_BILINEAR", 0), ("DVO_AMD_FUSE_NEAREST", 1)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define


def test_the_default_options_are_the_documented_ones(capi):
    opt = capi.FuseOptions()
    assert C.sizeof(opt) == 24
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt))
    capi.lib().dvo_amd_default_fuse_options(C.byref(opt))
    got = (opt.near_z, opt.depth_sigmas, opt.min_cos, opt.sample, opt.min_observations, opt.drop_unconfirmed)
    assert got == (F(0.1), 5.0, 0.5, capi.FUSE_BILINEAR, 0, 0)
    for k, v in ref.DEFAULTS.items():  # the restatement's defaults are the library's
        assert F(getattr(opt, k)) == F(v), k
    capi.lib().dvo_amd_default_fuse_options(None)  # a no-op
    assert capi.fuse_options(sample=capi.FUSE_NEAREST, min_cos=0.25).min_cos == 0.25
    with pytest.raises(TypeError):
        capi.fuse_options(unseen_keep=1)


# ---- CPU: the argument checks -----------------------------------------------------------------------------------------------------

class Fakes:
    """zeroed buffers that stand for pyramids (refs, device, n_levels lead a pyramid): an argument error is reported before any of
    them is looked at beyond its device"""

    def __init__(self, capi, n=3):
        self.keep = [C.create_string_buffer(1 << 16) for _ in range(n + 1)]
        for b in self.keep:
            C.c_int.from_buffer(b, 8).value = 1
        self.key = C.c_void_p(C.addressof(self.keep[0]))
        self.frames = (C.c_void_p * n)(*[C.addressof(b) for b in self.keep[1:]])
        self.T = (C.c_double * (16 * n))(*np.tile(np.eye(4).ravel(), n))
        self.opt = capi.fuse_options()
        self.n = n


def test_argument_errors_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    f = Fakes(capi)
    single, many = "dvo_amd_pyramid_fuse_depth", "dvo_amd_pyramid_fuse_depth_many"
    fc, kc = (C.c_longlong * 64)(), (C.c_longlong * 16)()

    def call(key=f.key, n=f.n, frames=f.frames, T=f.T, opt=f.opt, with_out=True):
        h = C.c_void_p(0xDEAD)
        rc = L.dvo_amd_pyramid_fuse_depth(key, n, frames, T, None if opt is None else C.byref(opt), C.byref(h) if with_out else None, fc, kc,
                                          None)
        return rc, h.value if with_out else None

    def refused(entry, got, what, word=None):
        rc, handle = got
        assert rc == INVALID, (entry, what, rc)
        assert not handle, (entry, what)
        reason = L.dvo_amd_last_error().decode()
        assert reason.startswith(entry + ": "), (entry, what, reason)
        assert word is None or word in reason, (entry, what, reason)

    for what, kw in {"keyframe": dict(key=None), "frames": dict(frames=None), "T": dict(T=None), "options": dict(opt=None)}.items():
        refused(single, call(**kw), what, "NULL")
    assert call(with_out=False)[0] == INVALID
    holed = (C.c_void_p * 3)(f.frames[0], None, f.frames[2])
    refused(single, call(frames=holed), "frames[1]", "NULL")
    refused(single, call(n=-1), "n < 0", "negative")
    big = (C.c_void_p * 256)(*[f.frames[0]] * 256)
    bigT = (C.c_double * (16 * 256))(*np.tile(np.eye(4).ravel(), 256))
    refused(single, call(n=256, frames=big, T=bigT), "n > 255", "255")
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 16 + 7, 32 + 15):
            T = (C.c_double * 48)(*f.T)
            T[at] = bad
            refused(single, call(T=T), ("T", bad, at), "non-finite")
    for field, value in (("near_z", 0.0), ("near_z", -1.0), ("near_z", np.nan), ("near_z", np.inf), ("depth_sigmas", -0.5),
                         ("depth_sigmas", np.nan), ("depth_sigmas", np.inf), ("min_cos", 0.0), ("min_cos", -0.5), ("min_cos", np.nan),
                         ("min_cos", np.inf), ("sample", 2), ("sample", -1), ("min_observations", -1), ("min_observations", 256)):
        refused(single, call(opt=capi.fuse_options(**{field: value})), (field, value), field if field != "sample" else "sample")

    keys = (C.c_void_p * 2)(f.key, f.key)
    offsets = (C.c_int * 3)(0, 1, 3)

    def call_many(nk=2, keyframes=keys, off=offsets, frames=f.frames, T=f.T, opt=f.opt, with_out=True):
        outs = (C.c_void_p * 2)(0xDEAD, 0xDEAD)
        rc = L.dvo_amd_pyramid_fuse_depth_many(nk, keyframes, off, frames, T, None if opt is None else C.byref(opt),
                                               outs if with_out else None, fc, kc, None)
        return rc, (outs[0] or outs[1]) if with_out else None

    for what, kw in {"keyframes": dict(keyframes=None), "offsets": dict(off=None), "frames": dict(frames=None), "T": dict(T=None),
                     "options": dict(opt=None), "keyframes[1]": dict(keyframes=(C.c_void_p * 2)(f.key, None)),
                     "frames[1]": dict(frames=holed)}.items():
        refused(many, call_many(**kw), what, "NULL")
    assert call_many(with_out=False)[0] == INVALID
    refused(many, (call_many(nk=-1)[0], None), "n_keyframes < 0", "negative")  # (a negative count names no output to clear)
    refused(many, call_many(off=(C.c_int * 3)(1, 2, 3)), "offsets start", "start at 0")
    refused(many, call_many(off=(C.c_int * 3)(0, 2, 1)), "offsets decrease", "decrease")
    refused(many, call_many(off=(C.c_int * 3)(0, 256, 256), frames=big, T=bigT), "a keyframe with 256 frames", "255")
    refused(many, call_many(opt=capi.fuse_options(sample=7)), "sample", "sample")
    if L.dvo_amd_device_count() == 0:
        # nothing left to refuse: the device is looked for, and the outputs are still NULL
        assert call() == (NO_DEVICE, None)
        assert call(n=0, frames=None, T=None) == (NO_DEVICE, None)      # without frames, frames and T may be NULL
        assert call_many() == (NO_DEVICE, None)
        assert call_many(nk=0) == (NO_DEVICE, 0xDEAD)                   # (no output is touched where there is none)


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------

def _same_ref(a, b, what):
    assert np.array_equal(a[0], b[0], equal_nan=True), what
    assert a[0].dtype == b[0].dtype == F and a[1].dtype == b[1].dtype == np.uint8
    assert np.array_equal(a[1], b[1]), what
    assert a[2] == b[2] and a[3] == b[3], what


def test_the_restatement_matches_the_pixel_loop(synth):
    """24x16, three frames of two sizes, a hole and an occluder: every class, every option"""
    w, h = 24, 16
    K = synth.intrinsics_for(w, h)
    K2 = tuple(F(k) for k in (40.0, 37.0, 15.5, 9.25))
    poses = [synth.se3_exp(t * 4 * synth.XI_STEP_STREAM) for t in range(4)]
    key = _sensor(synth, w, h, poses[0], 70)[1].copy()
    key[3:5, 4:9] = np.nan
    frames = [(_sensor(synth, w, h, poses[1], 71)[1], K), (_sensor(synth, 32, 20, poses[2], 72, K=K2)[1].copy(), K2),
              (_sensor(synth, w, h, poses[3], 73)[1].copy(), K)]
    frames[1][0][8:12, 10:20] *= F(0.7)
    frames[2][0][5:9, 2:8] *= F(1.3)
    frames[2][0][10:12, 12:15] = np.nan
    Ts = poses[1:]
    seen = dict.fromkeys(ref.FRAME_COUNTS + ref.KEYFRAME_COUNTS, 0)
    for sample in SAMPLES.values():
        for sigmas, min_obs, drop in GRID[:4] + [(0.0, 1, 1)]:
            for min_cos, near_z in ((0.5, 0.1), (0.999, 2.9)):  # (a near plane inside the scene: some points are behind it)
                opt = _opt(sample, sigmas, min_obs, drop, min_cos=min_cos, near_z=near_z)
                a, b = ref.fuse_ref((key, K), frames, Ts, opt), ref.fuse_brute((key, K), frames, Ts, opt)
                _same_ref(a, b, opt)
                for c in a[2]:
                    assert c["valid"] == sum(c[k] for k in ref.FRAME_COUNTS[1:7]) == int(np.isfinite(key).sum())
                    assert c["fused"] <= c["consistent"]
                assert a[3]["with_depth"] == sum(a[3][k] for k in ref.KEYFRAME_COUNTS[1:])
                assert int(a[1].sum()) == sum(c["fused"] for c in a[2])
                for d in a[2] + [a[3]]:
                    for k, v in d.items():
                        seen[k] += v
    assert all(v > 0 for v in seen.values()), seen
    # without frames the rule returns (w * z0) / w: the keyframe's depth to the last bit or the one next to it (two roundings)
    none = ref.fuse_ref((key, K), [], [])
    there = np.isfinite(key)
    assert np.array_equal(np.isfinite(none[0]), there) and not none[1].any() and none[2] == []
    assert (np.abs(none[0][there].view(np.int32) - key[there].view(np.int32)) <= 1).all()
    _same_ref(none, ref.fuse_brute((key, K), [], []), "n = 0")


def test_the_convention_on_an_exact_case():
    """A fronto-parallel plane at z = 2, fx = fy = 64, an integer principal point; the frame's camera stands 1 m nearer and sees
    the plane at 1.  T = match(keyframe, frame)'s transformation maps frame points into the keyframe: a translation of +1 along z.
    Every product is exact: keyframe pixel u lands on the frame's pixel 2 (u - ox) + ox, a = b = 0, d = 0, c = 1, and the fused depth
    is z0 exactly.  With the inverse handed in the plane is expected at 3 and found at 1: everything inside is occluded."""
    w, h = 24, 12
    K = (64.0, 64.0, 11.0, 5.0)
    Z0, Zk = np.full((h, w), 2.0, F), np.full((h, w), 1.0, F)
    T = np.eye(4)
    T[2, 3] = 1.0
    for sample in SAMPLES.values():
        fused, obs, (c,), kc = ref.fuse_ref((Z0, K), [(Zk, K)], [T], dict(sample=sample))
        assert np.array_equal(fused, Z0)
        u, v = np.meshgrid(np.arange(w), np.arange(h))
        last = 1 if sample == ref.NEAREST else 2
        inside = (2 * (u - 11) + 11 >= 0) & (2 * (u - 11) + 11 <= w - last) & (2 * (v - 5) + 5 >= 0) & (2 * (v - 5) + 5 <= h - last)
        assert np.array_equal(obs, inside.astype(np.uint8)) and 0 < inside.sum() < w * h
        assert c == dict(valid=w * h, behind=0, outside=int((~inside).sum()), no_depth=0, consistent=int(inside.sum()), occluded=0,
                         seen_through=0, fused=int(inside.sum()))
        assert kc == dict(with_depth=w * h, confirmed=w * h, unconfirmed_kept=0, unconfirmed_dropped=0)
        _, obs, (c,), _ = ref.fuse_ref((Z0, K), [(Zk, K)], [np.linalg.inv(T)], dict(sample=sample))
        assert not obs.any() and c["consistent"] == c["fused"] == 0
        assert c["occluded"] + c["seen_through"] + c["outside"] == w * h and c["occluded"] > 0


@pytest.mark.parametrize("sample", sorted(SAMPLES))
def test_nine_observations_beat_the_noise_of_four(synth, sample):
    """160x120, the keyframe and 8 frames of the stream at their ground-truth poses, depth_sigmas 3: the RMS error of the fused
    depth against the noise-free render, over the pixels where both are finite, is below 0.5 of the unfused keyframe's (what
    four equally noisy observations would give).  Measured when the rule was written: 0.30 bilinear, 0.42 nearest."""
    s = scenes()["stream"]
    truth = synth.render(160, 120, np.eye(4), nan_fraction=0, hole=False)[1]
    fused = s.ref(sample=SAMPLES[sample], depth_sigmas=3.0)[0]
    both = np.isfinite(fused) & np.isfinite(truth)
    assert np.array_equal(np.isfinite(fused), np.isfinite(s.key[1])) and both.sum() > 0.9 * 160 * 120

    def rms(z):
        return float(np.sqrt(np.mean((z[both].astype(np.float64) - truth[both]) ** 2)))

    before, after = rms(s.key[1]), rms(fused)
    print(f"{sample}: rms {1e3 * before:.2f} mm -> {1e3 * after:.2f} mm, ratio {after / before:.3f}")
    assert after < 0.5 * before, (before, after)


def test_the_scenes_reach_every_count():
    """over the scenes the GPU tests compare, under the options they use"""
    seen = dict.fromkeys(ref.FRAME_COUNTS + ref.KEYFRAME_COUNTS + ("grazing",), 0)
    for name, s in scenes().items():
        if name in ("repeated", "cycle"):
            continue
        for sample in SAMPLES.values():
            for opt in (_opt(sample, 3.0, 0, 0), _opt(sample, 3.0, 2, 0), _opt(sample, 3.0, 2, 1)):
                _, _, fcs, kc = s.ref(**opt)
                for c in fcs:
                    for k, v in c.items():
                        seen[k] += v
                    seen["grazing"] += c["consistent"] - c["fused"]
                for k, v in kc.items():
                    seen[k] += v
    assert all(v > 0 for v in seen.values()), seen
    _, _, (c,), _ = scenes()["behind"].ref(sample=ref.NEAREST, depth_sigmas=3.0)
    assert c["behind"] > 0
    _, _, (c,), _ = scenes()["grazing"].ref(sample=ref.BILINEAR, depth_sigmas=3.0)
    assert 0 < c["fused"] < c["consistent"]
    _, _, fcs, _ = scenes()["stream"].ref(sample=ref.BILINEAR, depth_sigmas=3.0)
    for name in ("outside", "no_depth", "occluded", "seen_through", "consistent"):
        assert sum(c[name] for c in fcs) > 0, name


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


class Resident:
    """a scene's pyramids on the device (a frame that occurs twice is uploaded once)"""

    def __init__(self, capi, scene):
        made = {}

        def pyramid(f):
            if id(f) not in made:
                made[id(f)] = capi.RgbdImagePyramid(f[0], f[1], f[2], f[3], timestamp=12.5 + len(made))
            return made[id(f)]

        self.scene, self.key, self.frames = scene, pyramid(scene.key), [pyramid(f) for f in scene.frames]

    def fuse(self, **opt):
        """(pyramid, fused plane, observations, frame counts as dicts, keyframe counts as a dict)"""
        p, fc, kc, obs = self.key.fuse_depth(self.frames, self.scene.Ts, opt, counts=True, observations=True)
        return p, p.plane(0, 1), obs, [{k: int(r[k]) for k in ref.FRAME_COUNTS} for r in fc], {k: int(kc[k]) for k in ref.KEYFRAME_COUNTS}


@pytest.fixture(scope="module")
def resident(gpu):
    return {name: Resident(gpu, s) for name, s in scenes().items()}


def _equals_the_restatement(r, opt, what):
    want = r.scene.ref(**opt)
    _, fused, obs, fc, kc = r.fuse(**opt)
    assert fused.dtype == F and np.array_equal(fused, want[0], equal_nan=True), what
    assert np.array_equal(np.isnan(fused), np.isnan(want[0])), what
    assert obs.dtype == np.uint8 and np.array_equal(obs, want[1]), what
    assert fc == want[2], what
    assert kc == want[3], what


@pytest.mark.gpu
@pytest.mark.parametrize("sample", sorted(SAMPLES))
@pytest.mark.parametrize("name", ["stream", "small", "mixed"])
def test_fusion_equals_the_restatement(resident, name, sample):
    for sigmas, min_obs, drop in GRID:
        opt = _opt(SAMPLES[sample], sigmas, min_obs, drop)
        _equals_the_restatement(resident[name], opt, (name, opt))
    _equals_the_restatement(resident[name], dict(sample=SAMPLES[sample]), (name, "defaults"))
    _equals_the_restatement(resident[name], dict(sample=SAMPLES[sample], min_cos=0.999, near_z=2.0), (name, "min_cos, near_z"))


@pytest.mark.gpu
@pytest.mark.parametrize("sample", sorted(SAMPLES))
@pytest.mark.parametrize("name", ["none", "repeated", "cycle", "behind", "grazing"])
def test_fusion_equals_the_restatement_at_its_edges(resident, name, sample):
    r = resident[name]
    for min_obs, drop in ((0, 0), (2, 1)):
        opt = _opt(SAMPLES[sample], 3.0, min_obs, drop)
        _equals_the_restatement(r, opt, (name, opt))
    if name == "none":
        _, fused, obs, fc, kc = r.fuse(sample=SAMPLES[sample])
        assert fc == [] and not obs.any() and kc["confirmed"] == kc["with_depth"] == int(np.isfinite(r.scene.key[1]).sum())
    if name == "repeated":
        _, _, obs, fc, _ = r.fuse(sample=SAMPLES[sample], depth_sigmas=3.0)
        assert len(fc) == 255 and obs.max() == 255


@pytest.mark.gpu
def test_the_result_is_an_ordinary_pyramid(gpu, resident):
    r = resident["stream"]
    I0, _, K, levels = r.scene.key
    opt = dict(depth_sigmas=3.0)
    cfg = gpu.Config(FirstLevel=levels - 1, LastLevel=0)
    trk = gpu.DenseTracker(cfg)
    before = [[r.key.plane(l, p) for p in range(6)] for l in range(levels)]
    tracked_before = trk.match(r.key, r.frames[0])
    fused, plane, _, _, _ = r.fuse(**opt)
    want = r.scene.ref(**opt)[0]
    host = gpu.RgbdImagePyramid(I0, want, K, levels, timestamp=r.key.timestamp())
    assert fused.levels() == host.levels() == levels and fused.timestamp() == r.key.timestamp()
    for l in range(levels):
        assert fused.level_info(l)[:2] == host.level_info(l)[:2] == r.key.level_info(l)[:2]
        assert np.array_equal(fused.level_info(l)[2], r.key.level_info(l)[2])
        for p in range(6):
            assert np.array_equal(fused.plane(l, p), host.plane(l, p), equal_nan=True), (l, p)
    assert np.array_equal(fused.plane(0, 0), I0) and not np.array_equal(plane, r.scene.key[1], equal_nan=True)
    for l in range(levels):
        thresholds = (cfg.IntensityDerivativeThreshold, cfg.DepthDerivativeThreshold)
        a, b = fused.select(l, *thresholds), host.select(l, *thresholds)
        assert a[0] == b[0] > 0 and np.array_equal(a[1], b[1])
    for frame in (r.frames[0], r.frames[7]):
        got = trk.match(fused, frame)
        assert not got.isNaN() and cases.same_result(got, trk.match(host, frame))
    assert not cases.same_result(trk.match(fused, r.frames[0]), tracked_before)
    # the keyframe itself is only read
    for l in range(levels):
        for p in range(6):
            assert np.array_equal(r.key.plane(l, p), before[l][p], equal_nan=True), (l, p)
    assert cases.same_result(trk.match(r.key, r.frames[0]), tracked_before)
    # counts=False, observations=False: the pyramid alone; the inputs may go before the result is used
    alone = r.key.fuse_depth(r.frames, r.scene.Ts, opt)
    assert isinstance(alone, gpu.RgbdImagePyramid) and np.array_equal(alone.plane(0, 1), want, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stream", "mixed", "behind"])
def test_nearest_counts_are_the_covisibility_counts(gpu, resident, name):
    from dvo_slam_amd import constraints as Cn

    r = resident[name]
    tracker = gpu.DenseTracker()
    for near_z, sigmas in ((0.1, 3.0), (2.0, 20.0)):
        _, _, _, fc, _ = r.fuse(sample=ref.NEAREST, near_z=near_z, depth_sigmas=sigmas)
        for k, frame in enumerate(r.frames):
            keyframes = [Cn.Keyframe(0, r.key, np.eye(4), None), Cn.Keyframe(1, frame, r.scene.Ts[k], None)]
            covis = gpu.covisibility(tracker, keyframes, [(0, 1)], level=0, near_z=near_z, depth_sigmas=sigmas)[0]
            assert [int(covis[c]) for c in ref.FRAME_COUNTS[:7]] == [fc[k][c] for c in ref.FRAME_COUNTS[:7]], (name, k, near_z)


@pytest.mark.gpu
def test_the_many_form_equals_single_calls(gpu, resident, synth):
    """five keyframes with 0, 1, 3, 3 and 8 frames in one call, in any order of the keyframes"""
    r = resident["stream"]
    pyramids = [r.key] + r.frames
    poses = [np.eye(4)] + r.scene.Ts
    groups = [(0, []), (3, [4]), (1, [0, 2, 3]), (5, [4, 6, 5]), (8, [0, 1, 2, 3, 4, 5, 6, 7])]
    opt = dict(depth_sigmas=3.0, min_observations=1)

    def relative(j, k):
        return np.linalg.inv(poses[j]) @ poses[k]

    single = [pyramids[j].fuse_depth([pyramids[k] for k in ks], [relative(j, k) for k in ks], opt, counts=True, observations=True)
              for j, ks in groups]
    for order in (list(range(5)), [4, 2, 0, 3, 1]):
        got = gpu.RgbdImagePyramid.fuse_depth_many([pyramids[groups[g][0]] for g in order],
                                                   [[pyramids[k] for k in groups[g][1]] for g in order],
                                                   [[relative(groups[g][0], k) for k in groups[g][1]] for g in order], opt, counts=True,
                                                   observations=True)
        assert [len(part) for part in got] == [5, 5, 5, 5]
        for at, g in enumerate(order):
            want = single[g]
            for l in range(4):
                assert np.array_equal(got[0][at].plane(l, 1), want[0].plane(l, 1), equal_nan=True), (order, g, l)
            assert got[0][at].timestamp() == want[0].timestamp() == pyramids[groups[g][0]].timestamp()
            assert np.array_equal(got[1][at], want[1]) and len(got[1][at]) == len(groups[g][1]), (order, g)
            assert got[2][at] == want[2] and np.array_equal(got[3][at], want[3]), (order, g)
    assert single[4][2]["confirmed"] > 0 and single[0][2]["unconfirmed_kept"] == single[0][2]["with_depth"]
    plain = gpu.RgbdImagePyramid.fuse_depth_many([r.key, r.frames[0]], [[r.frames[0]], []], [[poses[1]], []])
    assert len(plain) == 2 and all(isinstance(p, gpu.RgbdImagePyramid) for p in plain)
    assert gpu.RgbdImagePyramid.fuse_depth_many([], [], []) == []


@pytest.mark.gpu
def test_two_runs_give_the_same_bits(resident):
    for name in ("stream", "cycle"):
        a, b = resident[name].fuse(depth_sigmas=3.0), resident[name].fuse(depth_sigmas=3.0)
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3:] == b[3:], name


@pytest.mark.gpu
def test_frames_of_fewer_levels_and_other_devices(gpu, resident):
    r = resident["mixed"]
    assert r.key.levels() == 4 and all(f.levels() == 2 for f in r.frames)  # only level 0 of a frame is read
    p = r.key.fuse_depth(r.frames, r.scene.Ts)
    assert p.levels() == 4 and p.level_info(0)[:2] == (160, 120)
    L = gpu.lib()
    if L.dvo_amd_device_count() > 1:
        I, Z, K, levels = r.scene.frames[0]
        elsewhere = gpu.RgbdImagePyramid(I, Z, K, levels, device=1)
        with pytest.raises(gpu.DvoAmdError) as err:
            r.key.fuse_depth([r.frames[0], elsewhere], r.scene.Ts[:2])
        assert err.value.status == MISMATCH
    # a bad argument next to resident pyramids: refused, and the output stays NULL
    h = C.c_void_p(0xDEAD)
    T = (C.c_double * 16)(*np.eye(4).ravel())
    T[5] = np.nan
    opt = gpu.fuse_options()
    assert L.dvo_amd_pyramid_fuse_depth(r.key._h, 1, (C.c_void_p * 1)(r.frames[0]._h), T, C.byref(opt), C.byref(h), None, None,
                                        None) == INVALID and not h.value


@pytest.mark.gpu
def test_device_time_is_reported_when_asked_for(gpu, resident):
    r = resident["stream"]
    gpu.fuse_timing(True)
    try:
        r.key.fuse_depth(r.frames, r.scene.Ts)
        assert 0.0 < gpu.fuse_timing(True) < 1000.0
    finally:
        gpu.fuse_timing(False)
