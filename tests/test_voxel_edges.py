"""The voxel pipeline at its sort, range and merge-tile edges (csrc/dvo_map.cpp: the radix sort and its pass count, k_rekey /
k_delta_keys field widths, the index range, the chunk / tile borders of k_heads, the scans and k_accum, sums that wrap, and the
three border rules of k_merge), on inputs crafted to sit on those edges (tests/voxel_edge_cases.py).

Everything is compared bit for bit; there is no tolerance in this file.  The oracle is numpy: voxel_ref / _restate_map of
tests/test_map_cloud.py for the aggregate and the keyframe map (not a rebuild on the device), a Python dict for the merge.
CPU: voxel_ref against a brute force that wraps its sums modulo 2^64 as the header says; the census of every generated family
(pass count, kept / out-of-range / non-finite points, runs ending on a multiple of 16 and of 4096, merged positions of the
matches of a merge case) -- the proof that the GPU cases sit where they claim to.
GPU: dvo_amd_voxel_downsample, dvo_amd_map_cloud, the keyframe map and dvo_amd_debug_map_merge against those oracles."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_edge_cases as vc  # noqa: E402
from test_keyframe_map import _keyframe, _step_pose  # noqa: E402
from test_map_cloud import BIAS, _restate_map, random_cloud, same_bits, voxel_brute, voxel_ref  # noqa: E402


def _ref(xyz, rgb, leaf):
    with np.errstate(all="ignore"):  # (1 / leaf overflows at the denormal leaf)
        return voxel_ref(xyz, rgb, leaf)


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


# ---- CPU: the reference ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sign", [1, -1])
def test_voxel_ref_wraps_like_the_header(sign):
    """numpy's int64 reduceat wraps modulo 2^64, which is the header's rule: pinned against Python integers"""
    xyz, rgb = vc.wrapping_voxel(sign, _rng(1, sign > 0))
    assert vc.wraps_of(xyz)[0] >= 40 and vc.wraps_of(xyz)[1] == 0      # x wraps many times over, y does not
    # a second voxel that wraps (160 * 0.9 * 2^60 = 9 * 2^64), a third that does not
    far = np.tile(np.array([[(int(0.9 * BIAS) + 0.5) * 65536.0 * sign, 100.0, -300.0]], np.float32), (160, 1))
    xyz = np.concatenate([xyz, far, np.array([[1.0, 2.0, 3.0], [5.0, 2.5, 3.5]], np.float32)])
    rgb = np.concatenate([rgb, np.arange(162, dtype=np.uint32)])
    a, b = voxel_ref(xyz, rgb, vc.WRAP_LEAF), vc.voxel_brute_wrapped(xyz, rgb, vc.WRAP_LEAF)
    assert a[2]["voxels"] == 3 and {k: a[2][k] for k in b[2]} == b[2]
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    # without the wrap the answer is another one: the wrap is what is being pinned
    assert not same_bits(voxel_brute(xyz, rgb, vc.WRAP_LEAF)[0], b[0])


def test_wrapped_brute_force_equals_brute_force_without_a_wrap():
    xyz, rgb = random_cloud(_rng(2), 1500, 0.05)
    a, b, r = voxel_brute(xyz, rgb, 0.05), vc.voxel_brute_wrapped(xyz, rgb, 0.05), voxel_ref(xyz, rgb, 0.05)
    assert a[2] == b[2] and same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(r[0], b[0]) and same_bits(r[1], b[1])
    for gen in (vc.llrint_ties, lambda g: vc.colour_rounding(g)[:2], lambda g: vc.special_values(0, 1.0, g)[:2]):
        xyz, rgb = gen(_rng(3))
        b, r = vc.voxel_brute_wrapped(xyz, rgb, 1.0), voxel_ref(xyz, rgb, 1.0)
        assert same_bits(r[0], b[0]) and same_bits(r[1], b[1]) and {k: r[2][k] for k in b[2]} == b[2]


# ---- CPU: the census of every family ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", vc.COUNTS)
def test_census_of_the_count_families(n):
    c = vc.census(vc.counts_distinct(n, _rng(10, n))[0], 1.0)
    assert (c["points"], c["kept"], c["out_of_range"], c["non_finite"]) == (n, n, 0, 0)
    assert c["voxels"] == n and c["longest_run"] == 1 and c["ends_16"] == n // 16 and c["ends_4096"] == n // 4096
    # the field widths the layout of the distinct voxels gives (rank v -> (v // 4087 - 3, v // 67 % 61 - 30, v % 67 - 33))
    bits = ((n - 1) // 4087).bit_length(), min((n - 1) // 67, 60).bit_length(), min(n - 1, 66).bit_length()
    assert c["bits"] == bits and c["passes"] == -(-sum(bits) // 8)
    c = vc.census(vc.counts_runs(n, _rng(11, n))[0], 1.0)
    ends, at, k = [], 0, 0
    while at < n:                                    # the layout as its docstring states it, restated
        at = min(n, at + (16 if k % 20 < 4 else 17))
        ends.append(at)
        k += 1
    assert c["kept"] == n and c["voxels"] == len(ends) and c["longest_run"] == (17 if n >= 81 else min(n, 16))
    assert c["ends_16"] == sum(e % 16 == 0 for e in ends) and c["ends_4096"] == sum(e % 4096 == 0 for e in ends)
    if n >= 256:
        assert c["ends_16"] >= 4 and c["voxels"] - c["ends_16"] >= 10    # runs that end on a chunk border, runs that straddle one
    if n >= 8191:
        assert c["ends_4096"] >= 1                                       # 4032 = 12 * 336 is a period's end, 4096 = 4032 + 4 * 16
    c = vc.census(vc.counts_big_run(n, _rng(12, n))[0], 1.0)
    assert c["kept"] == n and c["longest_run"] == min(n, 4096) and c["voxels"] == 1 + max(0, n - 4096)
    assert c["ends_4096"] == n // 4096 and (n < 4096 or c["ends_16"] == 1 + (n - 4096) // 16)


@pytest.mark.parametrize("bits", vc.WIDTHS)
def test_census_of_the_key_width_families(bits):
    xyz, _ = vc.key_width(bits, _rng(20, *bits))
    c = vc.census(xyz, 1.0)
    assert c["bits"] == bits and c["passes"] == -(-sum(bits) // 8) and c["kept"] == len(xyz) >= 3000 and c["out_of_range"] == 0
    assert all(c["index_max"][a] - c["index_min"][a] == (1 << bits[a]) - 1 for a in range(3))   # the extreme corners are present
    for a in range(3):
        if bits[a] == 21:
            assert (c["index_min"][a], c["index_max"][a]) == (-BIAS, BIAS - 1)
    assert c["voxels"] < c["kept"] and (sum(bits) < 12 or c["voxels"] > 900)                    # runs, and many voxels


def test_key_width_families_cover_every_pass_count():
    total = sorted({sum(b) for b in vc.WIDTHS})
    assert total == [0, 1, 7, 8, 9, 16, 17, 21, 24, 25, 32, 33, 40, 48, 56, 57, 63]
    passes = [-(-t // 8) for t in total]
    assert sorted(set(passes)) == list(range(9))       # 0 .. 8: the result ends in either ping-pong buffer
    assert len(vc.WIDTHS) == 20 and len(vc.COUNTS) == 19


@pytest.mark.parametrize("leaf", vc.RANGE_LEAVES)
def test_census_of_the_range_families(leaf):
    lo, below, hi, above = vc.border_floats(leaf)
    inv = np.float32(1.0) / np.float32(leaf)
    assert np.floor(lo * inv) == -BIAS and np.floor(below * inv) == -BIAS - 1 and np.nextafter(lo, np.float32(-np.inf)) == below
    assert np.floor(hi * inv) == BIAS - 1 and np.floor(above * inv) == BIAS and np.nextafter(hi, np.float32(np.inf)) == above
    for axis in range(3):
        xyz, _, kept, oor = vc.range_edges(axis, leaf, _rng(30, axis))
        c = vc.census(xyz, leaf)
        assert (c["kept"], c["out_of_range"], c["non_finite"]) == (kept, oor, 0) == (10, 4, 0)
        assert c["index_min"][axis] == -BIAS and c["index_max"][axis] == BIAS - 1 and c["bits"][axis] == 21
        with np.errstate(over="ignore"):
            f = np.floor(xyz[:, axis] * inv)
        assert {-BIAS - 1, -BIAS, BIAS - 1, BIAS} <= set(f.tolist())
        xyz, _, bad, oor = vc.special_values(axis, leaf, _rng(31, axis))
        c = vc.census(xyz, leaf)
        assert (c["non_finite"], c["out_of_range"], c["kept"]) == (bad, oor, len(xyz) - bad - oor) == (3, 2, 6)
        # the negative denormal: floorf(-1e-45 * (1 / leaf)) = -1, not flushed to 0 (at leaf 65536 the product rounds to -0: index 0)
        assert c["index_min"][axis] == (0 if leaf > 1 else -1)
    # 3e38 is finite and its product with 1 / 0.01 is not
    with np.errstate(over="ignore"):
        assert np.isfinite(np.float32(3e38)) and np.isinf(np.float32(3e38) * (np.float32(1.0) / np.float32(0.01)))


def test_census_of_the_leaf_bounds():
    xyz, _ = vc.smallest_leaf_points(_rng(32))
    c = vc.census(xyz, vc.LEAF_MIN_NORMAL)
    assert (c["kept"], c["out_of_range"], c["non_finite"]) == (43, 1, 1) and c["voxels"] > 20 and max(c["bits"]) >= 10
    c = vc.census(xyz, vc.LEAF_MIN_DENORMAL)
    assert (c["kept"], c["out_of_range"], c["non_finite"]) == (0, 44, 1)
    assert vc.LEAF_MIN_DENORMAL > 0 and np.nextafter(np.float32(0), np.float32(1)) == np.float32(vc.LEAF_MIN_DENORMAL)
    assert min(v for v in vc.BAD_LEAVES if v > 65536 and np.isfinite(v)) == 65536.0078125


def test_census_of_the_sum_families():
    for sign in (1, -1):
        xyz, _ = vc.wrapping_voxel(sign, _rng(40, sign > 0))
        c = vc.census(xyz, vc.WRAP_LEAF)
        assert (c["kept"], c["voxels"], c["longest_run"]) == (1000, 1, 1000) and vc.wraps_of(xyz)[0] >= 40
        assert (xyz[:, 0] > 0).all() if sign > 0 else (xyz[:, 0] < 0).all()
    xyz, _ = vc.llrint_ties(_rng(41))
    even, odd = vc.ties_census(xyz)
    assert even >= 4 and odd >= 4 and even + odd == len(xyz)
    assert vc.census(xyz, 1.0)["index_min"] == (-1, -1, -1) and vc.census(xyz, 1.0)["index_max"] == (0, 0, 0)
    xyz, rgb, expect = vc.colour_rounding(_rng(42))
    rx, rr, st = voxel_ref(xyz, rgb, 1.0)
    assert st["voxels"] == 8 and same_bits(rr, expect)
    # per count: one channel rounded up from a remainder and one rounded down with one left over
    key = np.floor(xyz).astype(np.int64)
    for n, cnt in enumerate(vc.COLOUR_COUNTS):
        for second in (0, 1):
            m = (key[:, 0] == n) & (key[:, 1] == second)
            assert m.sum() == cnt
            ch = np.stack([(rgb[m] >> 16) & 0xFF, (rgb[m] >> 8) & 0xFF], axis=1).astype(np.int64).sum(axis=0)
            rem = sorted(int(v) % cnt for v in ch)
            assert rem == ([0, 0] if cnt == 1 else [-(-cnt // 2) - 1, -(-cnt // 2)])


# ---- the merge cases ----------------------------------------------------------------------------------------------------------------

def _matched_positions(ka, kb):
    """merged positions (store first on equal keys) of the store entries that have a delta entry of their key"""
    keys = np.concatenate([ka, kb])
    side = np.r_[np.zeros(len(ka), np.int64), np.ones(len(kb), np.int64)]
    order = np.lexsort((side, keys))
    k, s = keys[order], side[order]
    return [int(p) for p in np.flatnonzero((s[:-1] == 0) & (s[1:] == 1) & (k[:-1] == k[1:]))] if len(k) > 1 else []


def _merge_cases():
    """name -> (ka, va, kb, vb, facts); facts: total entries, n_out, and the merged positions of the store entries that have a
    delta entry of their key: all of them (matched), or some (matched_among, where the rest of the case is random)"""
    T = vc.MERGE_TILE
    out = {}

    def add(name, case, **facts):
        out[name] = (*case[:4], facts)

    def tokens(name, toks, seed, cancel=(), base=1 << 30, **facts):
        add(name, vc.merge_case(toks, _rng(50, seed), base=base, cancel=cancel), **facts)

    tokens("empty store", ["b"] * 5, 1, total=5, n_out=5)
    tokens("empty delta", ["a"] * 5, 2, total=5, n_out=5)
    tokens("one and one", ["a", "b"], 3, total=2, n_out=2)
    tokens("one and one, equal", ["ab"], 4, total=2, matched=[0], n_out=1)
    tokens("one and one, cancelled", ["ab"], 5, cancel=[0], total=2, matched=[0], n_out=0)
    for total in (2047, 2048, 2049, 4096, 4097):
        tokens(f"total {total}", vc.random_tokens(_rng(51, total), total), total, total=total)
    # a store entry last in its tile, its match first in the next: sb[lb] for the one, sa[-1] for the other
    tokens("match across the first border", ["a"] * (T - 1) + ["ab"] + ["b"] * 5 + ["a"] * 3, 6, total=T + 9, matched=[T - 1])
    mixed = vc.random_tokens(_rng(52), 2 * T - 1)
    tokens("match across the second border", mixed + ["ab"] + vc.random_tokens(_rng(53), 100), 7, total=2 * T + 101,
           matched_among=[2 * T - 1])
    tokens("match across a border, delta ends there", ["b"] * (T - 1) + ["ab"], 8, total=T + 1, matched=[T - 1])
    tokens("match inside a tile's end", ["a"] * (T - 2) + ["ab"] + ["a", "b"] * 4, 9, total=T + 8, matched=[T - 2])
    tokens("all cancel", ["ab"] * 3000, 10, cancel=range(3000), total=6000, matched=list(range(0, 6000, 2)), n_out=0)
    toks = ["a"] * (T - 3) + ["ab"] * 3 + ["b"] + ["ab"] * 2 + ["a"] * (T - 11) + ["ab"] * 2 + ["b"] * 7
    around = [T - 3, T - 2, T - 1, T + 1, T + 2, len(toks) - 9, len(toks) - 8]       # the 'ab' tokens
    tokens("cancel around the borders", toks, 11, cancel=around, total=len(toks) + 7,
           matched=[T - 3, T - 1, T + 1, T + 4, T + 6, 2 * T - 3, 2 * T - 1], n_out=len(toks) - 7)
    tokens("delta below the store", ["b"] * 700 + ["a"] * 3000, 12, total=3700, n_out=3700)
    tokens("delta above the store", ["a"] * 3000 + ["b"] * 700, 13, total=3700, n_out=3700)
    tokens("delta inside one gap", ["a"] * 1500 + ["b"] * 2500 + ["a"] * 1500, 14, total=5500, n_out=5500)
    tokens("alternation, store first", ["a", "b"] * 3000, 15, total=6000, n_out=6000)
    tokens("alternation, delta first", ["b", "a"] * 3000 + ["b"], 16, total=6001, n_out=6001)
    tokens("5000 and 3", ["a"] * 2047 + ["ab"] + ["a"] * 2000 + ["b"] + ["a"] * 952 + ["b"], 17, total=5003, matched=[2047], n_out=5002)
    tokens("3 and 5000", ["b"] * 2047 + ["ab"] + ["b"] * 2000 + ["a"] + ["b"] * 952 + ["a"], 18, total=5003, matched=[2047], n_out=5002)
    # a delta entry with count 0 and no match is dropped, sums or not; so is a store entry whose count the delta takes to 0
    ka, va, kb, vb, _ = vc.merge_case(["a", "b", "a", "b", "ab", "b"], _rng(50, 19))
    vb[0, 0] = vb[1, 0] = 0
    va[2, 0], vb[2, 0] = 7, (1 << 64) - 7
    add("count 0", (ka, va, kb, vb), total=7, matched=[4], n_out=3)
    # a negative delta count, as the wrapped u64 the device holds, leaves a positive count
    ka, va, kb, vb, _ = vc.merge_case(["a", "ab", "ab", "a"], _rng(50, 20))
    va[1, 0], vb[0, 0] = 5, (1 << 64) - 3
    va[2, 0], vb[1, 0] = 1, (1 << 64) - 1
    add("negative count", (ka, va, kb, vb), total=6, matched=[1, 3], n_out=3)
    # keys that use bit 62, up to the largest key there is
    ka, va, kb, vb, _ = vc.merge_case(vc.random_tokens(_rng(54), 3000), _rng(50, 21), base=(1 << 62) + (1 << 61))
    top = np.uint64((1 << 63) - 1)
    ka, va = np.r_[ka, top - np.uint64(1), top], np.concatenate([va, vc._sums(_rng(55), 2)])
    kb, vb = np.r_[kb, top], np.concatenate([vb, vc._sums(_rng(56), 1)])
    add("bit 62", (ka, va, kb, vb), total=3003)
    return out


MERGE_CASES = _merge_cases()


def test_census_of_the_merge_cases():
    T = vc.MERGE_TILE
    for name, (ka, va, kb, vb, facts) in MERGE_CASES.items():
        for k in (ka, kb):
            assert k.dtype == np.uint64 and (np.diff(k.astype(object)) > 0).all() and (len(k) == 0 or int(k[-1]) < 1 << 63), name
        assert va.shape == (len(ka), 8) and vb.shape == (len(kb), 8) and va.dtype == vb.dtype == np.uint64
        assert len(ka) + len(kb) == facts["total"], name
        matched = _matched_positions(ka, kb)
        assert set(facts.get("matched_among", [])) <= set(matched), (name, matched[:10])
        if "matched_among" not in facts and not name.startswith(("total", "bit 62")):
            assert matched == facts.get("matched", []), (name, matched[:10])     # these and no other
        rk, rv = vc.merge_reference(ka, va, kb, vb)
        if "n_out" in facts:
            assert len(rk) == facts["n_out"], (name, len(rk))
        assert (rv[:, 0] != 0).all() and (np.diff(rk.astype(object)) > 0).all()
    assert MERGE_CASES["empty store"][0].size == 0 and MERGE_CASES["empty delta"][2].size == 0
    # the three border rules, by position: a match whose store entry is the last of a tile (sb[lb], and sa[-1] for its delta
    # entry, first of the next tile), and one wholly inside a tile's end
    assert T - 1 in _matched_positions(*MERGE_CASES["match across the first border"][0:3:2])
    assert 2 * T - 1 in _matched_positions(*MERGE_CASES["match across the second border"][0:3:2])
    assert T - 2 in _matched_positions(*MERGE_CASES["match inside a tile's end"][0:3:2])
    assert int(MERGE_CASES["bit 62"][0][0]) >> 62 == 1 and int(MERGE_CASES["bit 62"][0][-1]) == (1 << 63) - 1
    assert {len(v[0]) for k, v in MERGE_CASES.items() if "5000" in k} == {5000, 3}
    # every 'total' case holds matches, store-only and delta-only entries
    for total in (2047, 2048, 2049, 4096, 4097):
        ka, va, kb, vb, _ = MERGE_CASES[f"total {total}"]
        m = len(_matched_positions(ka, kb))
        assert 0 < m < min(len(ka), len(kb))


def test_merge_reference_rules():
    ka, kb = np.array([5, 9], np.uint64), np.array([5, 7, 9], np.uint64)
    va = np.array([[2, 1, 1, 1, 1, 1, 1, 0], [1, vc.M64, 0, 0, 0, 0, 0, 0]], np.uint64)
    vb = np.array([[vc.M64, 3, 0, 0, 0, 0, 0, 9], [0, 4, 4, 4, 4, 4, 4, 4], [vc.M64, 1, 0, 0, 0, 0, 0, 0]], np.uint64)
    k, v = vc.merge_reference(ka, va, kb, vb)
    assert k.tolist() == [5] and v.tolist() == [[1, 4, 1, 1, 1, 1, 1, 9]]     # 7: count 0, dropped; 9: cancelled


def test_merge_probe_fails_loudly_without_a_gpu():
    from dvo_slam_amd import capi

    L = capi.lib()
    if L.dvo_amd_device_count() > 0:
        pytest.skip("a GPU is present")
    k, v, n = np.arange(1, 3, dtype=np.uint64), np.ones((2, 8), np.uint64), C.c_longlong(-1)
    ko, vo = np.zeros(4, np.uint64), np.zeros((4, 8), np.uint64)
    assert L.dvo_amd_debug_map_merge(None, 0, None, None, 0, None, None, None, None, None) == 2
    assert L.dvo_amd_debug_map_merge(None, 2, k.ctypes.data, v.ctypes.data, 2, k.ctypes.data, v.ctypes.data, ko.ctypes.data,
                                     vo.ctypes.data, C.byref(n)) == 2
    assert n.value == -1 and not ko.any() and not vo.any()
    with pytest.raises(capi.DvoAmdError) as e:
        capi.DenseTracker.debug_map_merge(type("T", (), {"_h": None})(), k, v, k, v)
    assert e.value.status == 2


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capi_gpu():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi


@pytest.fixture(scope="module")
def trk(capi_gpu):
    return capi_gpu.DenseTracker()


def _assert_downsample(trk, xyz, rgb, leaf, rng, what):
    """the library equals voxel_ref on (xyz, rgb) -- xyz, rgb and stats, bit for bit -- and on a permutation of it"""
    ref = _ref(xyz, rgb, leaf)
    a = trk.voxel_downsample(xyz, rgb, leaf)
    assert a[2] == ref[2], (what, a[2], ref[2])
    assert same_bits(a[0], ref[0]), what
    assert same_bits(a[1], ref[1]), what
    perm = rng.permutation(len(xyz))
    b = trk.voxel_downsample(xyz[perm], rgb[perm], leaf)
    assert b[2] == ref[2] and same_bits(b[0], ref[0]) and same_bits(b[1], ref[1]), (what, "permuted")
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("n", vc.COUNTS)
@pytest.mark.parametrize("family", list(vc.COUNT_FAMILIES))
def test_point_counts(trk, family, n):
    seed = {"distinct": 10, "runs": 11, "big_run": 12}[family]                  # (the seeds of the census test)
    xyz, rgb = vc.COUNT_FAMILIES[family](n, _rng(seed, n))
    _assert_downsample(trk, xyz, rgb, 1.0, _rng(13, n), (family, n))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", vc.WIDTHS)
def test_key_widths(trk, bits):
    xyz, rgb = vc.key_width(bits, _rng(20, *bits))
    ref = _assert_downsample(trk, xyz, rgb, 1.0, _rng(21, *bits), bits)
    assert ref[2]["voxels"] == vc.census(xyz, 1.0)["voxels"]


@pytest.mark.gpu
@pytest.mark.parametrize("leaf", vc.RANGE_LEAVES)
def test_index_range_and_special_values(trk, leaf):
    for axis in range(3):
        xyz, rgb, kept, oor = vc.range_edges(axis, leaf, _rng(30, axis))
        ref = _assert_downsample(trk, xyz, rgb, leaf, _rng(33, axis), ("range", axis, leaf))
        assert ref[2]["out_of_range"] == oor and ref[2]["finite"] == kept + oor
        xyz, rgb, bad, oor = vc.special_values(axis, leaf, _rng(31, axis))
        ref = _assert_downsample(trk, xyz, rgb, leaf, _rng(34, axis), ("special", axis, leaf))
        assert ref[2]["out_of_range"] == oor and ref[2]["finite"] == len(xyz) - bad
    # both at once on all three axes, among ordinary points
    parts = [vc.range_edges(a, leaf, _rng(35, a))[:2] for a in range(3)] + [vc.special_values(a, leaf, _rng(36, a))[:2] for a in range(3)]
    cloud = random_cloud(_rng(37), 2000, 0.05)
    xyz = np.concatenate([p[0] for p in parts] + [cloud[0] * np.float32(leaf / 0.05)])
    rgb = np.concatenate([p[1] for p in parts] + [cloud[1]])
    _assert_downsample(trk, xyz, rgb, leaf, _rng(38), ("mixed", leaf))


@pytest.mark.gpu
def test_leaf_bounds(capi_gpu, trk):
    xyz, rgb = vc.smallest_leaf_points(_rng(32))
    ref = _assert_downsample(trk, xyz, rgb, vc.LEAF_MIN_NORMAL, _rng(39), "smallest normal leaf")
    assert ref[2]["voxels"] > 20 and ref[2]["out_of_range"] == 1
    ref = _assert_downsample(trk, xyz, rgb, vc.LEAF_MIN_DENORMAL, _rng(39), "smallest leaf")
    assert ref[2] == {"points_in": 45, "finite": 44, "out_of_range": 44, "voxels": 0}
    for axis in range(3):
        xyz, rgb, _, _ = vc.range_edges(axis, vc.LEAF_MAX, _rng(30, axis))
        _assert_downsample(trk, xyz, rgb, vc.LEAF_MAX, _rng(39), "largest leaf")
    pts = np.zeros((4, 4), np.float32)
    st = capi_gpu.CCloudStats()
    L = capi_gpu.lib()
    for bad in vc.BAD_LEAVES:
        assert L.dvo_amd_voxel_downsample(trk._h, 4, pts.ctypes.data, bad, pts.ctypes.data, 4, C.byref(st)) == 1, bad
        h = C.c_void_p()
        assert L.dvo_amd_map_create(trk._h, bad, C.byref(h)) == 1 and not h.value, bad
    assert L.dvo_amd_voxel_downsample(trk._h, 4, pts.ctypes.data, 65536.0, pts.ctypes.data, 4, C.byref(st)) == 0


@pytest.mark.gpu
def test_sums(trk):
    for sign in (1, -1):
        xyz, rgb = vc.wrapping_voxel(sign, _rng(40, sign > 0))
        ref = _assert_downsample(trk, xyz, rgb, vc.WRAP_LEAF, _rng(43), ("wrap", sign))
        assert ref[2]["voxels"] == 1
        # the wrapped voxel among others, and twice over (the sum wraps on)
        far = np.tile(np.array([[(int(0.9 * BIAS) + 0.5) * 65536.0 * sign, 100.0, -300.0]], np.float32), (160, 1))
        xyz2 = np.concatenate([xyz, far, xyz, np.array([[1.0, 2.0, 3.0]], np.float32)])
        rgb2 = np.concatenate([rgb, np.arange(160, dtype=np.uint32), rgb, np.zeros(1, np.uint32)])
        _assert_downsample(trk, xyz2, rgb2, vc.WRAP_LEAF, _rng(44), ("wrap among others", sign))
    xyz, rgb = vc.llrint_ties(_rng(41))
    _assert_downsample(trk, xyz, rgb, 1.0, _rng(45), "llrint ties")
    xyz, rgb, expect = vc.colour_rounding(_rng(42))
    ref = _assert_downsample(trk, xyz, rgb, 1.0, _rng(46), "colour rounding")
    assert same_bits(ref[1], expect)


@pytest.mark.gpu
def test_capacity(capi_gpu, trk):
    L = capi_gpu.lib()
    for what, (xyz, rgb) in (("runs", vc.counts_runs(4097, _rng(11, 4097))), ("width", vc.key_width((9, 8, 8), _rng(20, 9, 8, 8)))):
        ref = _ref(xyz, rgb, 1.0)
        V = ref[2]["voxels"]
        pts = capi_gpu._pack_points(xyz, rgb)
        out = np.zeros((V, 4), np.float32)
        st = capi_gpu.CCloudStats()
        assert L.dvo_amd_voxel_downsample(trk._h, len(pts), pts.ctypes.data, 1.0, out.ctypes.data, V - 1, C.byref(st)) == 7, what
        assert st.voxels == V and not out.any(), what                       # the size needed; out untouched
        assert L.dvo_amd_voxel_downsample(trk._h, len(pts), pts.ctypes.data, 1.0, out.ctypes.data, V, C.byref(st)) == 0, what
        assert st.voxels == V and same_bits(out[:, :3].copy(), ref[0]) and same_bits(out[:, 3].view(np.uint32).copy(), ref[1])


@pytest.mark.gpu
def test_map_cloud_input_stage(capi_gpu, trk, synth):
    """one call over images of different sizes (the grid is sized by the largest), the smallest a pyramid can have, a width that
    is no multiple of 64, a w * h that is no multiple of 256, an all-NaN image between two valid ones, a BGR image with padded
    rows next to grey ones"""
    capi = capi_gpu
    rng = _rng(60)
    sizes = [(352, 264), (4, 2), (100, 7), (160, 120), (36, 30), (352, 264)]
    nan_image, padded = 3, {2: 305, 5: 352 * 3 + 64}
    assert 100 % 64 and (100 * 7) % 256 and (36 * 30) % 256 and 305 > 100 * 3
    pyrs, poses, bgrs, rows, strides = [], [], [], [], []
    for k, (w, h) in enumerate(sizes):
        Z = rng.uniform(0.4, 4.0, size=(h, w)).astype(np.float32)
        Z[rng.random((h, w)) < 0.1] = np.nan
        if k == nan_image:
            Z[:] = np.nan
        I = rng.uniform(-20.0, 280.0, size=(h, w)).astype(np.float32)
        pyrs.append(capi.RgbdImagePyramid(I, Z, (0.9 * w, 0.9 * w, 0.5 * w - 0.5, 0.5 * h - 0.5), 1))
        poses.append(synth.se3_exp(np.r_[rng.normal(scale=0.3, size=3), rng.normal(scale=0.2, size=3)]))
        if k in padded:
            buf = rng.integers(0, 256, size=(h, padded[k]), dtype=np.uint8)
            rows.append(buf)
            bgrs.append(buf[:, :w * 3].reshape(h, w, 3).copy())
            strides.append(padded[k])
        else:
            rows.append(None), bgrs.append(None), strides.append(0)
    for leaf in (0.05, 0.5):
        rx, rr, rst = _restate_map((pyrs, poses, bgrs), leaf)
        assert rst["points_in"] == sum(w * h for w, h in sizes) and 0 < rst["voxels"] < rst["finite"]
        n = len(pyrs)
        hs = (C.c_void_p * n)(*[p._h for p in pyrs])
        T = np.ascontiguousarray(np.stack([capi._pose_cm(P) for P in poses]))
        bp = (C.c_void_p * n)(*[None if b is None else b.ctypes.data for b in rows])
        sp = (C.c_int * n)(*strides)
        out = np.zeros((rst["voxels"], 4), np.float32)
        st = capi.CCloudStats()
        capi._check(capi.lib().dvo_amd_map_cloud(trk._h, n, hs, T.ctypes.data_as(C.POINTER(C.c_double)), bp, sp, leaf,
                                                 out.ctypes.data, len(out), C.byref(st)), "dvo_amd_map_cloud")
        got = {"points_in": st.points_in, "finite": st.finite, "out_of_range": st.out_of_range, "voxels": st.voxels}
        assert got == rst, (leaf, got, rst)
        xyz, rgb = capi._split_points(out)
        assert same_bits(xyz, rx) and same_bits(rgb, rr), leaf
        # the same through the binding (tight rows), in another image order
        order = [4, 3, 0, 5, 1, 2]
        a = trk.map_cloud([pyrs[i] for i in order], [poses[i] for i in order], [bgrs[i] for i in order], leaf=leaf)
        assert a[2] == rst and same_bits(a[0], rx) and same_bits(a[1], rr), leaf


@pytest.mark.gpu
def test_keyframe_map_equals_the_restatement(capi_gpu, trk, synth):
    """insert -> move -> remove -> insert: after every step the map equals numpy's aggregate over its keyframes (not a rebuild on
    the device, which shares the sort and k_accum with the map)"""
    capi = capi_gpu
    leaf = 0.02
    kfs = [_keyframe(capi, synth, 160, 120, k) for k in range(4)]
    pyrs, bgrs = [p for p, _ in kfs], [b for _, b in kfs]
    pose = [_step_pose(synth, k) for k in range(4)]
    moved = synth.se3_exp([0.01, 0.02, -0.01, 0.003, 0.01, -0.004]) @ pose[1]
    m = capi.KeyframeMap(trk, leaf)
    cur = {}

    def check(what):
        ids = sorted(cur)
        if ids:
            rx, rr, rst = _restate_map(([pyrs[i] for i in ids], [cur[i] for i in ids], [bgrs[i] for i in ids]), leaf)
        else:
            rx, rr, rst = _ref(np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), leaf)
        st = m.stats()
        assert st.pop("keyframes") == len(ids) and st == rst, (what, st, rst)
        xyz, rgb = m.extract()
        assert same_bits(xyz, rx) and same_bits(rgb, rr), what
        return rst["voxels"]

    check("empty")
    for k in range(3):
        m.insert(k, pyrs[k], pose[k], bgrs[k])
        cur[k] = pose[k]
        check(("insert", k))
    m.set_poses([1], [moved])
    cur[1] = moved
    assert m.timing()[2] == 2 * 160 * 120         # a delta of the old and the new contribution, not a rebuild
    check("move")
    m.remove([0])
    del cur[0]
    check("remove")
    m.insert(3, pyrs[3], pose[3], bgrs[3])
    cur[3] = pose[3]
    check("insert after remove")
    m.remove([1, 2, 3])
    cur.clear()
    assert check("all removed") == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MERGE_CASES))
def test_merge_probe(trk, name):
    ka, va, kb, vb, facts = MERGE_CASES[name]
    rk, rv = vc.merge_reference(ka, va, kb, vb)
    k, v = trk.debug_map_merge(ka, va, kb, vb)
    assert len(k) == len(rk), (name, len(k), len(rk))          # n_out
    assert same_bits(k, rk), name
    assert same_bits(v, rv), name                               # all eight words of every entry


@pytest.mark.gpu
def test_merge_probe_arguments(capi_gpu, trk, synth):
    capi = capi_gpu
    L = capi.lib()
    k, v, n = np.array([3, 5], np.uint64), np.ones((2, 8), np.uint64), C.c_longlong(-1)
    ko, vo = np.zeros(4, np.uint64), np.zeros((4, 8), np.uint64)

    def call(ctx=None, na=2, ka=k, va=v, nb=2, kb=k, vb=v, keys_out=ko, acc_out=vo, n_out=n):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.dvo_amd_debug_map_merge(trk._h if ctx is None else ctx, na, p(ka), p(va), nb, p(kb), p(vb), p(keys_out), p(acc_out),
                                         None if n_out is None else C.byref(n_out))

    assert capi.KeyframeMap(trk, 1.0).timing()[4] == vc.MERGE_TILE      # the tile the merge cases are laid out for
    assert call() == 0 and n.value == 2 and ko[:2].tolist() == [3, 5] and vo[:2].tolist() == [[2] * 8] * 2
    assert L.dvo_amd_debug_map_merge(None, 2, k.ctypes.data, v.ctypes.data, 0, None, None, ko.ctypes.data, vo.ctypes.data, C.byref(n)) == 1
    for bad in (dict(na=-1), dict(nb=-1), dict(ka=None), dict(va=None), dict(kb=None), dict(vb=None), dict(keys_out=None),
                dict(acc_out=None), dict(n_out=None), dict(na=1 << 31), dict(ka=np.array([5, 3], np.uint64)),
                dict(kb=np.array([5, 5], np.uint64)), dict(ka=np.array([3, 1 << 63], np.uint64))):
        assert call(**bad) == 1, bad
    # an empty side needs no arrays; nothing at all is an empty store
    assert call(nb=0, kb=None, vb=None) == 0 and n.value == 2
    assert call(na=0, ka=None, va=None) == 0 and n.value == 2
    assert call(na=0, ka=None, va=None, nb=0, kb=None, vb=None, keys_out=None, acc_out=None) == 0 and n.value == 0
    # refused while pairs are queued on the context
    K = synth.intrinsics_for(320, 240)
    ref = capi.RgbdImagePyramid.from_raw(*synth.sensor_frame(320, 240, None, frame_id=0), K, 4)
    nxt = capi.RgbdImagePyramid.from_raw(*synth.sensor_frame(320, 240, synth.se3_exp(synth.XI_GT_PAIR * 0.5), frame_id=1), K, 4)
    sub = trk.submit([ref] * 4, [nxt] * 4, in_flight=4)
    with pytest.raises(capi.DvoAmdError) as e:
        trk.debug_map_merge(k, v, k, v)
    assert e.value.status == 1
    trk.wait(sub)
    assert call() == 0 and n.value == 2
