"""Crafted inputs for the voxel pipeline (tests/test_voxel_edges.py): point sets that put the radix sort, the head scan, k_accum
and the index rule on their edges, and store / delta pairs that put k_merge on its three border rules.

The oracle stays tests/test_map_cloud.py (voxel_ref, voxel_brute: imported, unchanged).  `voxel_brute_wrapped` restates the
header's rule for sums beyond 2^63 -- reduced modulo 2^64, read as int64 before the division -- in Python integers, which
voxel_brute (no wrap) does not.  `census` counts what a point set actually exercises, from the points alone: the CPU tests
assert it per family, so a generator that stops hitting its edge fails there."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_map_cloud import BIAS, FIX  # noqa: E402

M64 = (1 << 64) - 1
RADIX_BITS = 8         # bits the sort consumes per pass
CHUNK = 16             # sorted positions one k_accum thread sums
TILE = 4096            # a radix tile, a scan tile and the positions of one k_accum block
MERGE_TILE = 2048      # merged entries per k_merge block (KeyframeMap.timing()[4])

COUNTS = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 65536, 65537]
WIDTHS = [(0, 0, 0), (1, 0, 0), (0, 0, 1), (7, 0, 0), (8, 0, 0), (3, 3, 3), (0, 8, 8), (6, 6, 5), (8, 8, 8), (9, 8, 8),
          (11, 11, 10), (11, 11, 11), (16, 16, 8), (16, 16, 16), (19, 19, 18), (19, 19, 19), (21, 0, 0), (0, 21, 0), (0, 0, 21),
          (21, 21, 21)]
RANGE_LEAVES = [1.0, 0.01, 65536.0]
BAD_LEAVES = [0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf"), float(np.nextafter(np.float32(65536.0), np.float32(np.inf)))]
LEAF_MIN_DENORMAL = float(np.float32(1e-45))            # the smallest float above 0: 1 / leaf is +inf
LEAF_MIN_NORMAL = float(np.finfo(np.float32).tiny)      # 2^-126: 1 / leaf = 2^126
LEAF_MAX = 65536.0


def _signed(v):
    return v - (1 << 64) if v >> 63 else v


def voxel_brute_wrapped(xyz, rgb, leaf):
    """voxel_brute with the header's wrap: every sum reduced modulo 2^64 and read as int64 before the division"""
    inv = np.float32(1.0) / np.float32(leaf)
    vox, finite, oor = {}, 0, 0
    for P, col in zip(np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(rgb, np.uint32).reshape(-1)):
        if not all(np.isfinite(P)):
            continue
        finite += 1
        with np.errstate(invalid="ignore", over="ignore"):
            ijk = [np.floor(np.float32(v) * inv) for v in P]
        if not all(-BIAS <= v < BIAS for v in ijk):
            oor += 1
            continue
        key = ((int(ijk[0]) + BIAS) << 42) | ((int(ijk[1]) + BIAS) << 21) | (int(ijk[2]) + BIAS)
        e = vox.setdefault(key, [0] * 7)
        col = int(col)
        d = [1] + [int(np.rint(float(P[a]) * FIX)) for a in range(3)] + [(col >> 16) & 0xFF, (col >> 8) & 0xFF, col & 0xFF]
        for a in range(7):
            e[a] = (e[a] + d[a]) & M64
    keys = sorted(vox)
    out = np.zeros((len(keys), 3), np.float32)
    cols = np.zeros(len(keys), np.uint32)
    for n, k in enumerate(keys):
        e = vox[k]
        for a in range(3):
            out[n, a] = np.float32(float(_signed(e[1 + a])) / (float(e[0]) * FIX))
        r, g, b = [(e[4 + a] + e[0] // 2) // e[0] for a in range(3)]
        cols[n] = (r << 16) | (g << 8) | b
    return out, cols, {"finite": finite, "out_of_range": oor, "voxels": len(keys)}


def bits_for(span):
    """bits of the field of an axis whose kept indices span `span`: the smallest b with 2^b > span"""
    return int(span).bit_length()


def census(xyz, leaf):
    """what a point set exercises, counted from the points: kept / out-of-range / non-finite points, the field widths and the
    pass count of the sort, the voxels, and the runs of equal keys (in sorted order) that end on a multiple of 16 and of 4096"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    finite = np.isfinite(xyz).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        inv = np.float32(1.0) / np.float32(leaf)
        f = np.floor(xyz * inv)
        inr = finite & ((f >= -BIAS) & (f < BIAS)).all(axis=1)
    c = {"points": len(xyz), "kept": int(inr.sum()), "out_of_range": int((finite & ~inr).sum()), "non_finite": int((~finite).sum())}
    if c["kept"] == 0:
        c.update(bits=(0, 0, 0), passes=0, voxels=0, ends_16=0, ends_4096=0, longest_run=0, index_min=None, index_max=None)
        return c
    idx = f[inr].astype(np.int64)
    mn, mx = idx.min(axis=0), idx.max(axis=0)
    bits = tuple(bits_for(s) for s in (mx - mn))
    key = np.sort(((idx[:, 0] + BIAS) << 42) | ((idx[:, 1] + BIAS) << 21) | (idx[:, 2] + BIAS))
    ends = np.r_[np.flatnonzero(key[1:] != key[:-1]) + 1, len(key)]  # one past the last position of every run
    c.update(bits=bits, passes=-(-sum(bits) // RADIX_BITS), voxels=len(ends), ends_16=int((ends % CHUNK == 0).sum()),
             ends_4096=int((ends % TILE == 0).sum()), longest_run=int(np.diff(np.r_[0, ends]).max()),
             index_min=tuple(int(v) for v in mn), index_max=tuple(int(v) for v in mx))
    return c


# ---- point sets at chosen voxel indices: leaf 1.0 ----------------------------------------------------------------------------

def points_at(ijk, rng):
    """one point in every given voxel at leaf 1.0: index + an eighth (1/8 .. 7/8), exact in fp32 for |index| <= 2^20; colours
    random"""
    ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
    frac = rng.integers(1, 8, size=ijk.shape).astype(np.float64) / 8.0
    xyz = (ijk + frac).astype(np.float32)
    assert np.array_equal(np.floor(xyz).astype(np.int64), ijk)
    return xyz, rng.integers(0, 1 << 24, size=len(ijk), dtype=np.uint32)


def _shuffled(rng, xyz, rgb):
    p = rng.permutation(len(xyz))
    return xyz[p], rgb[p]


def _voxel_of_rank(v):
    """distinct voxels whose key order is the order of v: spread over the three axes, negative indices included"""
    v = np.asarray(v, np.int64)
    return np.stack([v // (61 * 67) - 3, (v // 67) % 61 - 30, v % 67 - 33], axis=1)


def counts_distinct(n, rng):
    """n points, all voxels distinct"""
    return _shuffled(rng, *points_at(_voxel_of_rank(np.arange(n)), rng))


def counts_runs(n, rng):
    """n points in runs of exactly 16 and 17 laid end to end in key order: four runs of 16 (each ends on a chunk border), then
    sixteen runs of 17 (each straddles one, at every offset), and again; the last run is cut at n"""
    lengths = []
    while sum(lengths) < n:
        lengths += [16] * 4 + [17] * 16
    lengths = np.array(lengths)
    rank = np.repeat(np.arange(len(lengths)), lengths)[:n]
    return _shuffled(rng, *points_at(_voxel_of_rank(rank), rng))


def counts_big_run(n, rng):
    """one run of 4096 (or n, if smaller) in the first voxel, then distinct voxels: the run ends exactly on a k_accum block
    and on a radix tile"""
    rank = np.r_[np.zeros(min(n, TILE), np.int64), np.arange(1, max(1, n - TILE + 1))][:n]
    return _shuffled(rng, *points_at(_voxel_of_rank(rank), rng))


COUNT_FAMILIES = {"distinct": counts_distinct, "runs": counts_runs, "big_run": counts_big_run}


def key_width(bits, rng, n=3000):
    """about n points whose kept indices span exactly 2^b - 1 on every axis (b = bits of the axis, up to 21: the whole range),
    the eight extreme corners present, most voxels holding several points"""
    lo = np.array([-BIAS if b == 21 else -(1 << b) // 2 - 5 for b in bits], np.int64)
    hi = lo + np.array([(1 << b) - 1 for b in bits], np.int64)
    corners = np.array([[(hi if (c >> a) & 1 else lo)[a] for a in range(3)] for c in range(8)], np.int64)
    pool = np.stack([lo[a] + rng.integers(0, 1 << bits[a], size=n // 3) for a in range(3)], axis=1)
    ijk = np.concatenate([corners, pool, pool[rng.integers(0, len(pool), size=n - len(pool))]])
    return _shuffled(rng, *points_at(ijk, rng))


# ---- the index range and special values ----------------------------------------------------------------------------------------

def _index_of(x, leaf):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.floor(np.float32(x) * (np.float32(1.0) / np.float32(leaf)))


def coordinate_for_index(index, leaf):
    """a float whose voxel index at `leaf` is `index` under the fp32 rule floorf(x * (1.0f / leaf)): the middle of the voxel,
    moved float by float where fp32 rounding puts the middle next door"""
    x = np.float32((index + 0.5) * float(np.float32(leaf)))
    for _ in range(64):
        got = _index_of(x, leaf)
        if got == index:
            return x
        x = np.nextafter(x, np.float32(np.inf if got < index else -np.inf))
    raise AssertionError(f"no float lands in voxel {index} at leaf {leaf}")


def border_floats(leaf):
    """(the smallest float with index >= -2^20, its predecessor, the largest float with index < 2^20, its successor) at `leaf`:
    the four floats on the two borders of the range"""
    lo = coordinate_for_index(-BIAS, leaf)
    while _index_of(np.nextafter(lo, np.float32(-np.inf)), leaf) >= -BIAS:
        lo = np.nextafter(lo, np.float32(-np.inf))
    hi = coordinate_for_index(BIAS - 1, leaf)
    while _index_of(np.nextafter(hi, np.float32(np.inf)), leaf) < BIAS:
        hi = np.nextafter(hi, np.float32(np.inf))
    return lo, np.nextafter(lo, np.float32(-np.inf)), hi, np.nextafter(hi, np.float32(np.inf))


def range_edges(axis, leaf, rng):
    """points on one axis at the indices -2^20 and 2^20 - 1 (kept), -2^20 - 1 and 2^20 (out of range), the four floats on the
    two borders, a few points around 0 -- the other two axes stay near 0.  Returns (xyz, rgb, kept, out_of_range) with the
    counts the generator intends."""
    inside = [coordinate_for_index(-BIAS, leaf), coordinate_for_index(BIAS - 1, leaf)]
    outside = [coordinate_for_index(-BIAS - 1, leaf), coordinate_for_index(BIAS, leaf)]
    lo, below, hi, above = border_floats(leaf)
    inside += [lo, lo, hi]       # (lo twice: a run of two in the first voxel of the range)
    outside += [below, above]
    near = [coordinate_for_index(i, leaf) for i in (-2, -1, 0, 0, 1)]
    vals = np.array(inside + outside + near, np.float32)
    xyz = np.zeros((len(vals), 3), np.float32)
    for a in range(3):
        xyz[:, a] = coordinate_for_index(int(rng.integers(-3, 3)), leaf)
    xyz[:, axis] = vals
    rgb = rng.integers(0, 1 << 24, size=len(vals), dtype=np.uint32)
    return (*_shuffled(rng, xyz, rgb), len(inside) + len(near), len(outside))


def special_values(axis, leaf, rng):
    """+inf, -inf, NaN (dropped), -0.0, +0.0, the smallest denormal of either sign, and 3e38 of either sign (finite; x / leaf
    overflows to infinity at a leaf below 1: out of range) on one axis.  Returns (xyz, rgb, non_finite, intended out_of_range
    at a leaf of 0.01)."""
    tiny = np.float32(1e-45)
    vals = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, tiny, -tiny, 3e38, -3e38, 0.3, 0.7], np.float32)
    xyz = np.zeros((len(vals), 3), np.float32)
    for a in range(3):
        xyz[:, a] = coordinate_for_index(int(rng.integers(-3, 3)), leaf)
    xyz[:, axis] = vals
    return (*_shuffled(rng, xyz, rng.integers(0, 1 << 24, size=len(vals), dtype=np.uint32)), 3, 2)


def smallest_leaf_points(rng):
    """points for the two smallest leaves: multiples of 2^-120 (indices of a few hundred at the leaf 2^-126, every one out of
    range at the denormal leaf, whose reciprocal is infinite), zeros (0 * inf is NaN: finite points, out of range), ordinary
    coordinates (out of range at both) and a NaN"""
    m = rng.integers(-9, 10, size=(40, 3)).astype(np.float64)
    xyz = np.concatenate([(m * 2.0 ** -120).astype(np.float32), np.zeros((3, 3), np.float32),
                          np.array([[0.5, -0.25, 1.0], [np.nan, 0.0, 0.0]], np.float32)])
    return _shuffled(rng, xyz, rng.integers(0, 1 << 24, size=len(xyz), dtype=np.uint32))


# ---- sums ----------------------------------------------------------------------------------------------------------------------

WRAP_LEAF = 65536.0


def wrapping_voxel(sign, rng, n=1000):
    """one voxel of n points near x = sign * 6e10 at leaf 65536: q = x * 2^24 is about 1e18 a point, the x sum passes 2^63 after
    ten points and wraps modulo 2^64 some fifty times.  fp32 spacing there is 4096: 15 distinct x inside the voxel."""
    k = int(6e10 // 65536)
    x = (k * 65536 + 4096 * rng.integers(1, 16, size=n)).astype(np.float64) * sign
    xyz = np.stack([x, rng.integers(0, 32768, size=n) * 2.0 + 300 * 65536, rng.integers(1, 65536, size=n) * -1.0], axis=1)
    assert np.array_equal(xyz.astype(np.float32).astype(np.float64), xyz)
    xyz = xyz.astype(np.float32)
    return xyz, rng.integers(0, 1 << 24, size=n, dtype=np.uint32)


def wraps_of(xyz):
    """how often the exact sum of q over all points exceeds the int64 range: |sum| // 2^63 per axis (Python integers)"""
    q = np.rint(np.asarray(xyz, np.float32).astype(np.float64) * FIX)
    return [abs(sum(int(v) for v in q[:, a])) >> 63 for a in range(3)]


def llrint_ties(rng):
    """coordinates whose x * 2^24 lies on a .5: odd multiples of 2^-25 in [0.25, 0.5) and (-0.5, -0.25], where fp32 spacing is
    2^-25; half of them round up to even, half down.  Leaf 1.0: the voxels 0 and -1 on every axis, several points each."""
    m = rng.integers(1 << 22, 1 << 23, size=(64, 3)) * 2 + 1                  # odd, in [2^23, 2^24): m * 2^-25 in [0.25, 0.5)
    m[:8, 0] = (1 << 23) + 1 + 2 * np.arange(8)                               # both parities of (m - 1) / 2 for certain
    x = m.astype(np.float64) * 2.0 ** -25 * rng.choice([-1.0, 1.0], size=m.shape)
    xyz = x.astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), x)
    return xyz, rng.integers(0, 1 << 24, size=len(xyz), dtype=np.uint32)


def ties_census(xyz):
    """(points whose q is a tie with an even floor, with an odd floor): half-to-even rounds the first down, the second up"""
    v = np.asarray(xyz, np.float32).astype(np.float64)[:, 0] * FIX
    fl = np.floor(v)
    tie = (v - fl) == 0.5
    return int((tie & (fl % 2 == 0)).sum()), int((tie & (fl % 2 == 1)).sum())


COLOUR_COUNTS = [1, 2, 3, 255]


def colour_rounding(rng):
    """two voxels for every count in COLOUR_COUNTS whose channel sums sit on both sides of the count / 2 rounding: the first has
    r = the smallest remainder that rounds up, g = the largest that rounds down, b = remainder 0; the second swaps r and g and
    takes b = 255 on every point (the largest sum).  Returns (xyz, rgb, expected colour per voxel in key order)."""
    ijk, cols, expect = [], [], []
    for n, c in enumerate(COLOUR_COUNTS):
        up, down = -(-c // 2), -(-c // 2) - 1       # (sum + c // 2) // c rounds up from a remainder of ceil(c / 2) on
        if c == 1:
            up = down = 0                           # one point: the value itself
        for second in (0, 1):
            base = np.array([100, 7, 255 if second else 0], np.int64)
            rem = [down, up, 0] if second else [up, down, 0]
            ch = np.tile(base, (c, 1))
            for a in range(3):
                ch[:rem[a], a] += 1
            ijk += [[n, second, -n]] * c
            cols += [(int(r) << 16) | (int(g) << 8) | int(b) for r, g, b in ch]
            e = [(c * int(base[a]) + rem[a] + c // 2) // c for a in range(3)]
            expect.append(((n, second), (int(e[0]) << 16) | (int(e[1]) << 8) | int(e[2])))
    xyz, _ = points_at(np.array(ijk), rng)
    rgb = np.array(cols, np.uint32)
    p = rng.permutation(len(xyz))
    return xyz[p], rgb[p], np.array([v for _, v in sorted(expect)], np.uint32)


# ---- store / delta pairs for the merge probe -----------------------------------------------------------------------------------

def merge_reference(ka, va, kb, vb):
    """the merge as a dict: sums of equal keys added word by word modulo 2^64, entries whose count (word 0) is 0 dropped"""
    d = {int(k): [int(x) for x in v] for k, v in zip(ka, va)}
    for k, v in zip(kb, vb):
        e = d.setdefault(int(k), [0] * 8)
        for a in range(8):
            e[a] = (e[a] + int(v[a])) & M64
    keys = sorted(k for k, e in d.items() if e[0] != 0)
    return np.array(keys, np.uint64), np.array([d[k] for k in keys], np.uint64).reshape(-1, 8)


def _sums(rng, n, counts=None):
    v = rng.integers(0, 1 << 63, size=(n, 8), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 8), dtype=np.uint64)
    v[:, 0] = rng.integers(1, 1000, size=n, dtype=np.uint64) if counts is None else counts
    return v


def negated(v):
    """-v modulo 2^64, word by word"""
    return (~np.asarray(v, np.uint64)) + np.uint64(1)


def merge_case(tokens, rng, base=1 << 30, cancel=()):
    """A store / delta pair from the merged sequence it shall produce.  tokens: 'a' (a store entry), 'b' (a delta entry), 'ab'
    (a store entry and the delta entry of the same key: two merged positions, the store's first).  Keys ascend by random steps
    from `base`.  cancel: indices of 'ab' tokens whose delta is the negated store entry.  Returns (ka, va, kb, vb, pos) with
    pos[t] = the merged position of token t (of its store entry, for 'ab')."""
    steps = rng.integers(1, 1000, size=len(tokens)).astype(np.uint64)
    keys = np.uint64(base) + np.cumsum(steps, dtype=np.uint64)
    is_a = np.array([t in ("a", "ab") for t in tokens], bool)
    is_b = np.array([t in ("b", "ab") for t in tokens], bool)
    pos = np.cumsum(np.r_[0, (is_a.astype(np.int64) + is_b)[:-1]]) if len(tokens) else np.zeros(0, np.int64)
    ka, kb = keys[is_a], keys[is_b]
    va, vb = _sums(rng, len(ka)), _sums(rng, len(kb))
    a_at, b_at = np.cumsum(is_a) - 1, np.cumsum(is_b) - 1
    for t in cancel:
        assert tokens[t] == "ab"
        vb[b_at[t]] = negated(va[a_at[t]])
    return ka, va, kb, vb, pos


def random_tokens(rng, total):
    """a random mix of 'a', 'b' and 'ab' whose entries (an 'ab' is two) add up to exactly `total`"""
    out, n = [], 0
    while n < total:
        t = ("a", "b", "ab")[int(rng.integers(0, 3))] if total - n >= 2 else ("a", "b")[int(rng.integers(0, 2))]
        out.append(t)
        n += 2 if t == "ab" else 1
    return out
