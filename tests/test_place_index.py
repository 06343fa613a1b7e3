"""The place index (include/dvo_amd.h, "Place index"): dvo_amd_place_index_* / dvo_amd_place_scores / dvo_amd_place_query[_frames].
The rule is pinned in the header and restated in tests/place_ref.py.  Every comparison with the library is equality: int8 rows,
int32 norms and dots, candidate ids, counts, and doubles bit for bit.
CPU: exports and layout, the argument checks that need no device, the restatement against its pixel loop, rounding and clamping on
a plane whose arithmetic is exact, and the retrieval property the descriptor is there for.  GPU: the library against the restatement.
A pyramid level is at least 4x2 with a width that is a multiple of 4 (dvo_amd_pyramid_create refuses anything else), so where the
restatement is checked on 17x9 and 2x2 planes the device is checked on 20x9 and 4x2."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_ref as ref  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dvo_amd_default_place_options", "dvo_amd_default_place_query_options", "dvo_amd_place_index_create",
               "dvo_amd_place_index_destroy", "dvo_amd_place_index_add", "dvo_amd_place_index_info", "dvo_amd_place_index_download",
               "dvo_amd_place_scores", "dvo_amd_place_query", "dvo_amd_place_query_frames", "dvo_amd_debug_place_timing"]
INVALID, NO_DEVICE = 1, 2


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    c.lib()
    return c


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
    assert (capi.PLACE_MAX_K, capi.PLACE_MAX_DIM, capi.PLACE_INITIAL_CAPACITY) == (ref.MAX_K, ref.MAX_DIM, ref.INITIAL_CAPACITY) == (64, 65536, 64)
    header = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    for define, value in (("DVO_AMD_PLACE_MAX_K", 64), ("DVO_AMD_PLACE_MAX_DIM", 65536), ("DVO_AMD_PLACE_INITIAL_CAPACITY", 64)):
        assert re.search(r"#define %s %d\b" % (define, value), header), define
    for word in ("removed or re-ordered", "one image size per index", "viewpoint invariance", "no depth in the descriptor", "only proposes"):
        assert word in header, word  # what is not covered is said where the entries are declared


def test_the_default_options_are_the_documented_ones(capi):
    opt, q = capi.PlaceOptions(), capi.PlaceQueryOptions()
    assert C.sizeof(opt) == 8 and C.sizeof(q) == 24
    C.memset(C.byref(opt), 0x5A, C.sizeof(opt)), C.memset(C.byref(q), 0x5A, C.sizeof(q))
    capi.lib().dvo_amd_default_place_options(C.byref(opt))
    capi.lib().dvo_amd_default_place_query_options(C.byref(q))
    assert (opt.level, opt.gain) == (3, 1.0) == (ref.DEFAULTS["level"], ref.DEFAULTS["gain"])
    assert (q.k, q.min_score, q.exclude_recent) == (5, 0.0, 0) == tuple(ref.QUERY_DEFAULTS[k] for k in ("k", "min_score", "exclude_recent"))
    capi.lib().dvo_amd_default_place_options(None), capi.lib().dvo_amd_default_place_query_options(None)  # no-ops
    assert capi.place_options(level=2, gain=0.5).gain == 0.5 and capi.place_query_options(k=64).k == 64
    with pytest.raises(TypeError):
        capi.place_options(levels=2)
    with pytest.raises(TypeError):
        capi.place_query_options(exclude=2)


# ---- CPU: the argument checks that need no device -----------------------------------------------------------------------------------

def _refused(L, entry, rc, what, word=None):
    assert rc == INVALID, (entry, what, rc)
    reason = L.dvo_amd_last_error().decode()
    assert reason.startswith(entry + ": "), (entry, what, reason)
    assert word is None or word in reason, (entry, what, reason)


def test_argument_errors_are_refused_with_a_reason_before_a_device_is_looked_for(capi):
    L = capi.lib()
    create = "dvo_amd_place_index_create"
    h = C.c_void_p(0xDEAD)
    _refused(L, create, L.dvo_amd_place_index_create(0, None, C.byref(h)), "options", "NULL")
    assert not h.value
    _refused(L, create, L.dvo_amd_place_index_create(0, C.byref(capi.place_options()), None), "out", "NULL")
    for field, value in (("level", -1), ("level", capi.MAX_LEVELS), ("gain", 0.0), ("gain", -1.0), ("gain", np.nan), ("gain", np.inf)):
        h = C.c_void_p(0xDEAD)
        _refused(L, create, L.dvo_amd_place_index_create(0, C.byref(capi.place_options(**{field: value})), C.byref(h)), (field, value), field)
        assert not h.value
    # without an index every other entry stops at its first check
    ints, doubles, one = (C.c_int * 64)(), (C.c_double * 64)(), (C.c_void_p * 1)(0)
    q = capi.place_query_options()
    _refused(L, "dvo_amd_place_index_add", L.dvo_amd_place_index_add(None, 1, one, ints), "index", "NULL")
    assert ints[0] == -1
    _refused(L, "dvo_amd_place_index_info", L.dvo_amd_place_index_info(None, ints, ints, ints, ints), "index", "NULL")
    _refused(L, "dvo_amd_place_index_download", L.dvo_amd_place_index_download(None, 0, 0, None, ints), "index", "NULL")
    _refused(L, "dvo_amd_place_scores", L.dvo_amd_place_scores(None, 1, ints, 0, 1, ints), "index", "NULL")
    _refused(L, "dvo_amd_place_query", L.dvo_amd_place_query(None, 1, ints, C.byref(q), ints, doubles, ints), "index", "NULL")
    _refused(L, "dvo_amd_place_query_frames", L.dvo_amd_place_query_frames(None, 1, one, C.byref(q), ints, doubles, ints), "index", "NULL")
    L.dvo_amd_place_index_destroy(None)  # a no-op
    assert L.dvo_amd_debug_place_timing(-1, 0, None) == INVALID
    if L.dvo_amd_device_count() == 0:
        h = C.c_void_p(0xDEAD)
        assert L.dvo_amd_place_index_create(0, C.byref(capi.place_options()), C.byref(h)) == NO_DEVICE and not h.value
        with pytest.raises(capi.DvoAmdError) as e:
            capi.PlaceIndex()
        assert e.value.status == NO_DEVICE


# ---- CPU: the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(17, 9), (20, 15), (2, 2)])
def test_the_restatement_matches_the_pixel_loop(w, h):
    rng = np.random.default_rng(w * 100 + h)
    for gain in (1.0, 0.37, 3.0):
        I = rng.uniform(0, 255, (h, w)).astype(F)
        a, b = ref.descriptor(I, gain), ref.descriptor_loop(I, gain)
        assert a[0].dtype == np.int8 and len(a[0]) == ref.dim_of(w, h) and len(a[0]) % 64 == 0
        assert np.array_equal(a[0], b[0]) and a[1] == b[1], (w, h, gain)
        assert not a[0][w * h:].any() and a[0].min() >= -127
    I = rng.uniform(0, 255, (h, w)).astype(F)
    I[0, 0], I[h - 1, w - 1] = np.nan, np.inf
    a, b = ref.descriptor(I), ref.descriptor_loop(I)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert (w, h) != (2, 2) or not a[0].any()  # (every 2x2 neighbourhood is the whole plane)


def test_rounding_clamping_and_non_finite_values_on_a_plane_whose_arithmetic_is_exact():
    I, expect = ref.tie_plane()
    for q, nn in (ref.descriptor(I), ref.descriptor_loop(I)):
        for p, d, want in expect:
            assert q[p] == want, (p, d, q[p], want)
        assert nn == int((q.astype(np.int64) ** 2).sum())
    assert [e[2] for e in expect[:len(ref.TIE_D)]] == [0, 0, 2, -2, 2, 126, 127, 127, -127]
    assert sum(1 for e in expect if e[1] is None) == 27


def test_a_brightness_offset_and_a_gain_leave_the_ranking_alone():
    """the score's invariances on the restatement alone: + c leaves the descriptor (up to rounding), * g the cosine"""
    rng = np.random.default_rng(7)
    planes = [rng.uniform(20, 200, (15, 20)).astype(F) for _ in range(6)]
    X, nn = ref.describe(planes)
    Q, qn = ref.describe([planes[2] * F(0.8) + F(10)])
    cand, score, count = ref.query_frames(X, nn, Q, qn, 6, min_score=-2.0)
    assert count[0] == 6 and cand[0, 0] == 2 and score[0, 0] > 0.99 and score[0, 1] < 0.5


# ---- the retrieval scene: 160x120 sensor frames, level 2 ------------------------------------------------------------------------------

RW, RH, RLEVELS, RLEVEL = 160, 120, 4, 2


@functools.lru_cache(maxsize=None)
def retrieval_frames():
    """(keyframes, frame, frame_shifted): 20 keyframes -- the nine stream frames of the default scene (ids 0..8), six frames of
    scene seed + 77 (9..14), five more of the default scene at exp(t * XI_GT_PAIR) (15..19) -- and a fresh-noise frame at
    poses[3] * exp(0.3 * XI_STEP_STREAM), as it is and as 0.8 * I + 10.  Each a float (I, Z) pair."""
    from dvo_slam_amd import synth

    def sensor(pose, frame_id, seed=synth.SEED):
        return synth.raw_to_float(*synth.sensor_frame(RW, RH, pose, seed=seed, frame_id=frame_id))

    poses = synth.stream_poses(9)
    keyframes = [sensor(poses[t], t) for t in range(9)]
    keyframes += [sensor(poses[t], 20 + t, seed=synth.SEED + 77) for t in range(6)]
    keyframes += [sensor(synth.se3_exp(t * synth.XI_GT_PAIR), 40 + t) for t in range(1, 6)]
    I, Z = sensor(poses[3] @ synth.se3_exp(0.3 * synth.XI_STEP_STREAM), 60)
    return keyframes, (I, Z), (F(0.8) * I + F(10), Z)


def test_the_descriptor_retrieves_the_revisited_keyframe(orc, synth):
    """on the restatement, with the level planes of the oracle's pyramid: the best candidate is keyframe 3, every frame of the other
    scene scores below every stream frame, and 0.8 * I + 10 gives the same ranking"""
    keyframes, frame, shifted = retrieval_frames()
    K = synth.intrinsics_for(RW, RH)

    def level_plane(f):
        return orc.Pyramid(f[0], f[1], K, RLEVELS).plane(RLEVEL, 0)

    X, nn = ref.describe([level_plane(f) for f in keyframes])
    assert X.shape == (20, ref.dim_of(RW >> RLEVEL, RH >> RLEVEL))
    Q, qn = ref.describe([level_plane(frame), level_plane(shifted)])
    cand, score, count = ref.query_frames(X, nn, Q, qn, 20, min_score=-2.0)
    assert list(count) == [20, 20]
    by_id = {int(j): float(s) for j, s in zip(cand[0], score[0])}
    stream, other = [by_id[j] for j in range(9)], [by_id[j] for j in range(9, 15)]
    print("keyframe 3 %.4f, stream min %.4f, other scene max %.4f" % (by_id[3], min(stream), max(other)))
    assert cand[0, 0] == 3
    assert max(other) < min(stream)
    assert list(cand[1]) == list(cand[0])


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def _gpu(capi):
    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")


def _pyramid(capi, I, levels=1):
    from dvo_slam_amd import synth

    I = np.ascontiguousarray(I, dtype=F)
    h, w = I.shape
    return capi.RgbdImagePyramid(I, np.ones((h, w), F), synth.intrinsics_for(w, h), levels)


def _same_doubles(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def _same_result(got, want):
    return np.array_equal(got[0], want[0]) and _same_doubles(got[1], want[1]) and np.array_equal(got[2], want[2])


class Bank:
    """130 one-level 20x15 pyramids of random planes (dim 320: five k-steps, so a wave of k_place_dots takes a second one) in one
    index, with the restated rows and norms of what the device holds (fed with the planes the pyramids hand back)"""

    def __init__(self, capi, n=130, w=20, h=15, seed=11):
        rng = np.random.default_rng(seed)
        self.pyramids = [_pyramid(capi, rng.uniform(0, 255, (h, w))) for _ in range(n)]
        self.index = capi.PlaceIndex(level=0)
        self.ids = self.index.add(self.pyramids)
        self.X, self.nn = ref.describe([p.plane(0, 0) for p in self.pyramids])
        self.X.setflags(write=False), self.nn.setflags(write=False)


@pytest.fixture(scope="module")
def bank(capi):
    _gpu(capi)
    return Bank(capi)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(20, 9), (8, 8), (20, 15), (4, 2), (48, 3)])
def test_descriptors_and_norms_equal_the_restatement(capi, w, h):
    """20x9: 180 -> 192, rows straddle waves, padding; 8x8: 64, no padding; 4x2: borders only; 48x3: the tie / clamp plane with
    its non-finite patches"""
    _gpu(capi)
    rng = np.random.default_rng(w * 100 + h)
    planes = [rng.uniform(0, 255, (h, w)).astype(F) for _ in range(3)]
    planes[1][0, 0], planes[1][h - 1, w - 1], planes[2][h // 2, w // 2] = np.nan, np.inf, -np.inf
    expect = []
    if (w, h) == (48, 3):
        planes[0], expect = ref.tie_plane()
    for gain in (1.0, 0.37):
        index = capi.PlaceIndex(level=0, gain=gain)
        pyramids = [_pyramid(capi, I) for I in planes]
        assert index.add(pyramids) == range(0, 3)
        assert index.info() == {"size": 3, "width": w, "height": h, "dim": ref.dim_of(w, h)} and len(index) == 3
        got = [p.plane(0, 0) for p in pyramids]
        assert all(np.array_equal(g, I, equal_nan=True) for g, I in zip(got, planes))  # (non-finite intensities are accepted)
        X, nn = ref.describe(got, gain)
        rows, norms = index.descriptors()
        assert rows.dtype == np.int8 and norms.dtype == np.int32
        assert np.array_equal(rows, X) and np.array_equal(norms, nn), (w, h, gain)
        if gain == 1.0:
            for p, _, want in expect:
                assert rows[0, p] == want
        rows1, norms1 = index.descriptors(1, 2)
        assert np.array_equal(rows1, X[1:]) and np.array_equal(norms1, nn[1:])


@pytest.mark.gpu
def test_a_four_level_pyramid_is_described_at_levels_one_to_three(capi):
    _gpu(capi)
    from dvo_slam_amd import synth

    keyframes, _, _ = retrieval_frames()
    K = synth.intrinsics_for(RW, RH)
    pyramids = [capi.RgbdImagePyramid(I, Z, K, RLEVELS) for I, Z in keyframes[:2]]
    for level in (1, 2, 3):
        index = capi.PlaceIndex(level=level, gain=0.5)
        index.add(pyramids)
        X, nn = ref.describe([p.plane(level, 0) for p in pyramids], 0.5)
        rows, norms = index.descriptors()
        assert rows.shape == (2, ref.dim_of(RW >> level, RH >> level))
        assert np.array_equal(rows, X) and np.array_equal(norms, nn), level
    too_few = capi.RgbdImagePyramid(keyframes[0][0], keyframes[0][1], K, 2)
    with pytest.raises(capi.DvoAmdError) as e:
        capi.PlaceIndex(level=2).add([too_few])
    assert e.value.status == INVALID and "fewer than 3 levels" in capi.lib().dvo_amd_last_error().decode()


@pytest.mark.gpu
def test_forty_pyramids_in_one_add_equal_the_same_one_by_one(capi, bank):
    one = capi.PlaceIndex(level=0)
    for i, p in enumerate(bank.pyramids[:40]):
        assert one.add([p]) == range(i, i + 1)
    rows, norms = one.descriptors()
    assert np.array_equal(rows, bank.X[:40]) and np.array_equal(norms, bank.nn[:40])
    many = capi.PlaceIndex(level=0)
    assert many.add(bank.pyramids[:40]) == range(0, 40)
    rows2, norms2 = many.descriptors()
    assert np.array_equal(rows2, rows) and np.array_equal(norms2, norms)
    assert many.add([]) == range(40, 40) and len(many) == 40


@pytest.mark.gpu
def test_growth_across_the_initial_capacity_keeps_every_row(capi, bank):
    index = capi.PlaceIndex(level=0)
    at = 0
    for n in (63, 1, 1, 40):  # 63 + 1 fills the 64 rows, the next add reallocates, the last crosses 128 as well
        assert index.add(bank.pyramids[at:at + n]) == range(at, at + n)
        at += n
        assert len(index) == at
    rows, norms = index.descriptors()
    assert np.array_equal(rows, bank.X[:at]) and np.array_equal(norms, bank.nn[:at])
    assert np.array_equal(index.scores([0, 64, 104]), ref.dots(bank.X[[0, 64, 104]], bank.X[:at]))
    want = ref.query(bank.X[:at], bank.nn[:at], [104, 0], 5)
    assert _same_result(index.query([104, 0], k=5), want)  # (r of every row is uploaded anew behind a reallocation)


DOT_CASES = [(n, nq) for n in (1, 15, 16, 17, 33, 130) for nq in (1, 2, 16, 17, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,nq", sorted(set(DOT_CASES)))
def test_dots_equal_the_int64_matmul(bank, n, nq):
    """n keys x nq queries: every tile shape of k_place_dots (1, 2 and 4 blocks of 16 per side), partial tiles on both sides,
    n_queries != n with data that has no symmetry (a transposed write would show), key ranges that start off a tile boundary"""
    rng = np.random.default_rng(1000 * n + nq)
    for first in sorted({0, min(3, 130 - n), 130 - n}):
        ids = rng.integers(0, 130, nq)
        got = bank.index.scores(ids, first, n)
        assert got.dtype == np.int32 and got.shape == (nq, n)
        assert np.array_equal(got, ref.dots(bank.X[ids], bank.X[first:first + n])), (n, nq, first)


@pytest.mark.gpu
def test_dots_over_seventy_five_k_steps_extremes_a_flat_image_and_the_canary(capi):
    _gpu(capi)
    L = capi.lib()
    rng = np.random.default_rng(5)
    # one-level 80x60: dim 4800, 75 k-steps shared by four waves (19, 19, 19, 18)
    pyramids = [_pyramid(capi, rng.uniform(0, 255, (60, 80))) for _ in range(17)]
    index = capi.PlaceIndex(level=0)
    index.add(pyramids)
    X, nn = ref.describe([p.plane(0, 0) for p in pyramids])
    rows, norms = index.descriptors()
    assert rows.shape == (17, 4800) and np.array_equal(rows, X) and np.array_equal(norms, nn)
    for ids in ([5], list(range(17)), [16, 0, 3]):
        assert np.array_equal(index.scores(ids), ref.dots(X[ids], X))
    # a canary around the output: the call writes n_queries * n ints and nothing else
    ids = (C.c_int * 3)(16, 0, 3)
    out = np.full(4 + 3 * 5 + 4, -77, np.int32)
    assert L.dvo_amd_place_scores(index._h, 3, ids, 2, 5, out[4:].ctypes.data_as(C.POINTER(C.c_int))) == 0
    assert np.array_equal(out[4:19].reshape(3, 5), ref.dots(X[[16, 0, 3]], X[2:7])) and (out[:4] == -77).all() and (out[19:] == -77).all()

    # a checkerboard and its inverse at a gain that clamps every pixel: the extremes +- dim * 127^2; a flat image: nn = 0, r = 0
    board = (np.indices((16, 16)).sum(0) % 2).astype(F) * F(255)
    flat = np.full((16, 16), F(93.5))
    index = capi.PlaceIndex(level=0, gain=4.0)
    index.add([_pyramid(capi, I) for I in (board, F(255) - board, flat)])
    rows, norms = index.descriptors()
    assert index.info()["dim"] == 256 and set(np.unique(rows[0])) == {-127, 127} and np.array_equal(rows[1], -rows[0])
    assert not rows[2].any() and list(norms) == [256 * 127 * 127, 256 * 127 * 127, 0]
    assert np.array_equal(index.scores([0, 1, 2]), [[256 * 16129, -256 * 16129, 0], [-256 * 16129, 256 * 16129, 0], [0, 0, 0]])
    X, nn = ref.describe([board, F(255) - board, flat], 4.0)
    got = index.query([0, 1, 2], k=2, min_score=-2.0)
    assert _same_result(got, ref.query(X, nn, [0, 1, 2], 2, min_score=-2.0))
    assert list(got[0][2]) == [0, 1] and list(got[1][2]) == [0.0, 0.0]  # the flat image scores 0 against everything
    assert list(got[0][0]) == [2, 1] and got[1][0][0] == 0.0 and got[1][0][1] < -0.99


@pytest.mark.gpu
def test_queries_equal_the_restatement(capi, bank):
    X, nn, index = bank.X, bank.nn, bank.index
    N = len(X)
    ends = [0, 1, 2, 3, 64, N - 4, N - 3, N - 2, N - 1]
    for exclude in (0, 1, 3):
        for k in (1, 5, 64):
            got = index.query(ends, k=k, exclude_recent=exclude, min_score=-2.0)
            assert got[0].shape == (len(ends), k) and _same_result(got, ref.query(X, nn, ends, k, -2.0, exclude)), (exclude, k)
            for row, q in zip(got[0], ends):
                assert all(abs(int(j) - q) > exclude for j in row)
    # the default min_score of 0 leaves about half of the keys of random planes; a threshold equal to a returned score keeps that key
    got = index.query([7], k=64)
    assert _same_result(got, ref.query(X, nn, [7], 64))
    assert got[2][0] > 5
    threshold = float(got[1][0][4])
    kept = index.query([7], k=64, min_score=threshold)
    assert kept[2][0] == 5 and kept[0][0][4] == got[0][0][4] and _same_result(kept, ref.query(X, nn, [7], 64, threshold))
    above = index.query([7], k=64, min_score=np.nextafter(threshold, 2.0))
    assert above[2][0] == 4
    # all pairs in one call equal N single calls, and the same call twice gives the same bits
    everything = index.query(range(N), k=5, exclude_recent=1)
    assert _same_result(everything, ref.query(X, nn, range(N), 5, 0.0, 1))
    for q in (0, 17, 129):
        single = index.query([q], k=5, exclude_recent=1)
        assert _same_result(single, tuple(part[q:q + 1] for part in everything))
    assert _same_result(index.query(range(N), k=5, exclude_recent=1), everything)


@pytest.mark.gpu
def test_ties_go_to_the_lower_id_small_indices_and_frames(capi, bank):
    # every pyramid twice: a key and its duplicate tie, the query's own duplicate scores highest
    index = capi.PlaceIndex(level=0)
    index.add(bank.pyramids[:16] + bank.pyramids[:16] + bank.pyramids[:1])
    X, nn = np.concatenate([bank.X[:16], bank.X[:16], bank.X[:1]]), np.concatenate([bank.nn[:16], bank.nn[:16], bank.nn[:1]])
    got = index.query(range(33), k=64, min_score=-2.0)
    assert _same_result(got, ref.query(X, nn, range(33), 64, -2.0)) and (got[2] == 32).all()  # k above the eligible set
    assert (got[0][:, 32:] == -1).all() and np.isnan(got[1][:, 32:]).all() and (got[0][:, :32] >= 0).all()
    assert list(got[0][5][:3]) == [21] + sorted(got[0][5][1:3]) and got[1][5][1] == got[1][5][2]
    assert list(got[0][0][:2]) == [16, 32] and got[1][0][0] == got[1][0][1]  # two duplicates of row 0: the lower id first
    # N = 1: nothing is eligible for the only row; a frame sees it
    solo = capi.PlaceIndex(level=0)
    solo.add(bank.pyramids[:1])
    got = solo.query([0], k=3, min_score=-2.0)
    assert got[2][0] == 0 and list(got[0][0]) == [-1] * 3 and np.isnan(got[1][0]).all()
    got = solo.query_frames(bank.pyramids[:2], k=3, min_score=-2.0)
    assert _same_result(got, ref.query_frames(bank.X[:1], bank.nn[:1], bank.X[:2], bank.nn[:2], 3, -2.0)) and list(got[2]) == [1, 1]
    # an empty index: counts of 0, nothing else
    empty = capi.PlaceIndex(level=0)
    got = empty.query_frames(bank.pyramids[:2], k=4)
    assert list(got[2]) == [0, 0] and (got[0] == -1).all() and np.isnan(got[1]).all() and len(empty) == 0
    assert empty.query([], k=4)[0].shape == (0, 4)
    # a frame that is also in the index: query_frames(p) is query(id) without exclusion, once the key id itself is dropped
    for q in (0, 77, 129):
        frames = bank.index.query_frames([bank.pyramids[q]], k=64, min_score=-2.0)
        assert _same_result(frames, ref.query_frames(bank.X, bank.nn, bank.X[q:q + 1], bank.nn[q:q + 1], 64, -2.0))
        assert frames[0][0][0] == q  # itself, at a cosine of 1 up to two roundings
        ids = bank.index.query([q], k=64, min_score=-2.0)
        assert list(frames[0][0][1:]) == list(ids[0][0][:63]) and _same_doubles(frames[1][0][1:], ids[1][0][:63])


@pytest.mark.gpu
def test_row_panels_above_the_scratch_cap_change_nothing(capi):
    """8200 rows of dim 64: the 8200 x 8200 dots are 269 MB, above the 256 MiB cap, so a call over all rows is processed in two
    panels of query rows (8128 + 72).  The index holds 82 pyramids a hundred times over: every row has 99 exact duplicates."""
    _gpu(capi)
    rng = np.random.default_rng(82)
    pyramids = [_pyramid(capi, rng.uniform(0, 255, (8, 8))) for _ in range(82)]
    index = capi.PlaceIndex(level=0)
    for _ in range(100):
        index.add(pyramids)
    N = len(index)
    assert N == 8200 and 4 * N * N > 256 << 20
    X64, nn64 = ref.describe([p.plane(0, 0) for p in pyramids])
    X, nn = np.tile(X64, (100, 1)), np.tile(nn64, 100)
    Xf = X.astype(np.float64)  # (|dot| <= 64 * 127^2: a double matmul is exact, and fast)
    got = index.scores(range(N))
    assert got.shape == (N, N)
    for s in range(0, N, 1024):
        assert np.array_equal(got[s:s + 1024], Xf[s:s + 1024] @ Xf.T), s
    del got
    cand, score, counts = index.query(range(N), k=3, exclude_recent=2)
    r = np.array([ref.inv_norm(v) for v in nn])
    for q in (0, 1, 81, 82, 4100, 8127, 8128, 8129, 8199):  # both sides of the panel boundary
        want = ref.query_row(ref.dots(X[q:q + 1], X)[0], r[q], r, q, 3, 0.0, 2)
        assert np.array_equal(cand[q], want[0]) and _same_doubles(score[q], want[1]) and counts[q] == want[2] == 3, q
        assert _same_result(index.query([q], k=3, exclude_recent=2), (cand[q:q + 1], score[q:q + 1], counts[q:q + 1]))
    assert list(cand[0]) == [82, 164, 246] and list(cand[8199]) == [81, 163, 245]  # the duplicates of lowest id


@pytest.mark.gpu
def test_argument_errors_that_need_an_index(capi, bank):
    L = capi.lib()
    ix = bank.index._h
    ints, doubles = (C.c_int * 4096)(), (C.c_double * 4096)()
    q = capi.place_query_options()
    handles = (C.c_void_p * 2)(bank.pyramids[0]._h, bank.pyramids[1]._h)
    add, download, scores, query, frames = ("dvo_amd_place_index_add", "dvo_amd_place_index_download", "dvo_amd_place_scores",
                                            "dvo_amd_place_query", "dvo_amd_place_query_frames")
    _refused(L, add, L.dvo_amd_place_index_add(ix, -1, handles, None), "n < 0", "negative")
    _refused(L, add, L.dvo_amd_place_index_add(ix, 2, None, None), "pyramids", "NULL")
    _refused(L, add, L.dvo_amd_place_index_add(ix, 2, (C.c_void_p * 2)(handles[0], None), None), "pyramids[1]", "NULL")
    other = _pyramid(capi, np.zeros((8, 8), F))
    _refused(L, add, L.dvo_amd_place_index_add(ix, 2, (C.c_void_p * 2)(handles[0], other._h), None), "another size", "8x8")
    _refused(L, frames, L.dvo_amd_place_query_frames(ix, 1, (C.c_void_p * 1)(other._h), C.byref(q), ints, doubles, ints), "another size", "8x8")
    big = _pyramid(capi, np.zeros((260, 256), F))
    fresh = capi.PlaceIndex(level=0)
    _refused(L, add, L.dvo_amd_place_index_add(fresh._h, 1, (C.c_void_p * 1)(big._h), None), "66560 values", "65536")
    assert len(fresh) == 0 and len(bank.index) == 130
    _refused(L, download, L.dvo_amd_place_index_download(ix, 0, -1, None, ints), "n < 0", "negative")
    for first, n in ((-1, 1), (130, 1), (100, 31)):
        _refused(L, download, L.dvo_amd_place_index_download(ix, first, n, None, ints), (first, n), "outside")
        _refused(L, scores, L.dvo_amd_place_scores(ix, 1, ints, first, n, ints), (first, n), "outside")
    _refused(L, scores, L.dvo_amd_place_scores(ix, -1, ints, 0, 1, ints), "n_queries < 0", "negative")
    _refused(L, scores, L.dvo_amd_place_scores(ix, 1, ints, 0, -1, ints), "n < 0", "negative")
    _refused(L, scores, L.dvo_amd_place_scores(ix, 1, None, 0, 1, ints), "ids", "NULL")
    _refused(L, scores, L.dvo_amd_place_scores(ix, 1, ints, 0, 1, None), "dots", "NULL")
    for bad in (-1, 130):
        ids = (C.c_int * 2)(0, bad)
        _refused(L, scores, L.dvo_amd_place_scores(ix, 2, ids, 0, 1, ints), bad, "outside")
        _refused(L, query, L.dvo_amd_place_query(ix, 2, ids, C.byref(q), ints, doubles, ints), bad, "outside")
    _refused(L, query, L.dvo_amd_place_query(ix, 1, ints, None, ints, doubles, ints), "options", "NULL")
    _refused(L, query, L.dvo_amd_place_query(ix, -1, ints, C.byref(q), ints, doubles, ints), "n_queries < 0", "negative")
    for missing in range(4):
        args = [ints, ints, doubles, ints]
        args[missing] = None
        _refused(L, query, L.dvo_amd_place_query(ix, 1, args[0], C.byref(q), args[1], args[2], args[3]), missing, "NULL")
    for field, value in (("k", 0), ("k", 65), ("min_score", np.nan), ("exclude_recent", -1)):
        bad = capi.place_query_options(**{field: value})
        _refused(L, query, L.dvo_amd_place_query(ix, 1, ints, C.byref(bad), ints, doubles, ints), (field, value), field)
        _refused(L, frames, L.dvo_amd_place_query_frames(ix, 1, handles, C.byref(bad), ints, doubles, ints), (field, value), field)
    _refused(L, frames, L.dvo_amd_place_query_frames(ix, 1, (C.c_void_p * 1)(None), C.byref(q), ints, doubles, ints), "frames[0]", "NULL")
    # counts of zero are fine and touch nothing
    ints[0] = 12345
    assert L.dvo_amd_place_scores(ix, 0, None, 0, 130, None) == 0 and L.dvo_amd_place_query(ix, 0, None, C.byref(q), None, None, None) == 0
    assert L.dvo_amd_place_index_add(ix, 0, None, ints) == 0 and ints[0] == 130
    assert capi.place_timing(True) >= 0.0
    bank.index.query([3], k=5)
    assert capi.place_timing(False) > 0.0


@pytest.mark.gpu
def test_the_chain_on_the_device_from_appearance_to_validated_constraints(capi, synth):
    _gpu(capi)
    from dvo_slam_amd import constraints as Cn

    keyframes, frame, shifted = retrieval_frames()
    K = synth.intrinsics_for(RW, RH)
    trk = capi.DenseTracker(capi.Config())
    poses = synth.stream_poses(9)

    def keyframe(i, f):
        p = capi.RgbdImagePyramid(f[0], f[1], K, RLEVELS)
        pose = poses[i] if i < 9 else np.eye(4)  # (the search reads no pose; the validator's relative proposals do)
        return Cn.Keyframe(i, p, pose, Cn.LogLikelihoodTrackingResultEvaluation(trk.match(p, p)))

    every = [keyframe(i, f) for i, f in enumerate(keyframes)]
    search = Cn.AppearanceConstraintSearch(k=4, level=RLEVEL)
    pyramid = capi.RgbdImagePyramid(frame[0], frame[1], K, RLEVELS)
    found = search.findForFrame(every, pyramid)
    assert len(search.index) == 20 and len(found) == 4 and found[0] is every[3]
    assert all(kf.id < 9 or kf.id >= 15 for kf in found) and list(search.scores) == sorted(search.scores, reverse=True)
    again = search.findForFrame(every, capi.RgbdImagePyramid(shifted[0], shifted[1], K, RLEVELS))
    assert [kf.id for kf in again] == [kf.id for kf in found]
    result = trk.match(every[3].image, pyramid)  # relocalisation: from the identity, against the keyframe the search proposes
    assert not result.isNaN() and np.isfinite(result.Transformation).all()
    assert synth.pose_error(result.Transformation, synth.se3_exp(0.3 * synth.XI_STEP_STREAM)) < 0.01

    candidates = search.findPossibleConstraints(every, every[4])
    assert len(search.index) == 20 and every[4] not in candidates and len(candidates) == 4
    assert {kf.id for kf in candidates} <= set(range(9)) | set(range(15, 20))
    val = Cn.createConstraintProposalValidator(min_constraint_ratio=0.0, ratio_coarse=-1e300, ratio_fine=-1e300, tracker=trk)
    proposals = Cn.proposalsForCandidates(every[4], candidates)
    assert len(proposals) == 8
    survivors = val.validate(proposals)
    assert survivors and all({p.Reference.id, p.Current.id} <= {4} | {kf.id for kf in candidates} for p in survivors)
    with pytest.raises(ValueError):
        search.findPossibleConstraints(every[:3], every[0])  # the index holds more keyframes than `all`
