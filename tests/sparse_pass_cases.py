"""Shared pieces of tests/test_sparse_passes.py: residual passes over sparse selections and gappy valid streams, held to the oracle
through its keep plane (oracle.Pyramid.set_keep) and to the library through a selection mask.

Geometry: level 1 of the 160x120 small pair, as tests/counted_selection_cases.py -- 80 x 60 pixels walked in 4-step wave segments,
so point p of the compacted selection sits in segment p // 256 (step p % 256 // 64, lane p % 64) and block p // 1024.

Counted cases keep exactly n selected points (counted_selection_cases.count_mask_planes) against the pair's own current frame.

Gappy cases decide, point by point, which walked points are VALID constraints.  The current frame's depth is NaN in column
stripes, so at the scene pose (identity: where a match starts) about a third of the reference's selected pixels warp to a valid
constraint and the rest do not, the two kinds interleaved along every row.  A scene is a list of segments, each a length (256 but for
the last), a count of valid points and, where the place matters, the wanted flags; the builder walks the oracle's own out_valid
flags of the unmasked selection in scan order and keeps the selected pixels that fill the segments (keep_plane_for).  Validity is
a property of the point alone, so the kept points carry the wanted counts -- which tests/test_sparse_passes.py asserts again on the
oracle's flags under the keep plane, per scene, with the predicate the scene is named for."""
import numpy as np

import counted_selection_cases as counted

W, H, LEVELS, LEVEL = counted.W, counted.H, counted.LEVELS, counted.LEVEL
SEG, BLOCK = 64 * counted.STEPS, counted.BLOCK_POINTS  # points per wave segment, per block
COUNTS_ADDED = (2, 5, 6, 7, 49, 50, 51, 99, 100, 101, 255, 256, 257)  # the six-constraint rule, the Q6 group, a segment
COUNTS = tuple(sorted(counted.COUNTS + COUNTS_ADDED))
STRIPE_PERIOD, STRIPE_KEPT = 16, 9  # level-1 columns: depth stays in the first 9 of every 16


def seg(n_valid=0, at="any", length=SEG):
    """one segment of a scene: (length, valid count, wanted flags or None).  at = "any": the builder places the n_valid valid points
    where the frame has them; "head" / "tail" / a list of positions: exactly there"""
    if at == "any":
        return length, n_valid, None
    f = np.zeros(length, bool)
    if at == "head":
        f[:n_valid] = True
    elif at == "tail":
        f[length - n_valid:] = True
    else:
        f[list(at)] = True
    assert int(f.sum()) == n_valid
    return length, n_valid, f


# ---- the scenes: name -> segments.  Every segment but the last is full; the total is even (an odd trailing point is not walked).
# Where a segment is empty, the valid count before it is odd in most scenes: the segment behind it then starts on an odd rank and
# its first point pairs with the last residual from BEFORE the gap (Q5) -- the carry an empty segment must not disturb.
SCENES = {
    # 1: an empty segment between two that hold valid points, inside one block
    "empty_segment_in_block": [seg(37), seg(0), seg(21), seg(10, length=40)],
    # 2: a whole empty block between two blocks that hold valid points
    "empty_block": [seg(40), seg(33), seg(27), seg(19)] + [seg(0)] * 4 + [seg(25), seg(14, length=60)],
    # 3 + 4: a one-point segment behind an odd one (7) and behind an even one (12); then 1, 9, 11, 3: four odd segments in a row
    "single_points_and_odd_runs": [seg(7), seg(1), seg(12), seg(1), seg(9), seg(11), seg(3, length=30)],
    # 5: the level's first valid point in the last lane of the last step of its segment, its last one in a segment's first lane
    "edge_lanes": [seg(1, [SEG - 1]), seg(20), seg(1, [0], length=2)],  # (V 22)
    # 6: the likelihood cut at 50 floor(V / 50)
    "v_multiple_of_50": [seg(60), seg(40, length=128)],
    "v_49_mod_50": [seg(60), seg(39, length=128)],
    "cut_at_segment_start": [seg(100), seg(30, length=128)],             # V 130: the cut, 100, is the rank seg 1 starts at
    "cut_behind_empty_segment": [seg(71), seg(0), seg(49, length=128)],  # V 120: the cut, 100, falls in seg 2 (ranks 71 ..)
    # 7: V on both sides of the six-constraint rule with hundreds of selected points
    "v5": [seg(3), seg(0), seg(2, length=100)],
    "v6": [seg(3), seg(1), seg(2, length=100)],
    "v7": [seg(3), seg(0), seg(4, length=100)],
    # 8: the last V mod 4 valid points (Q7) across a segment boundary
    "tail1_alone_behind_boundary": [seg(40), seg(1, length=64)],           # V 41
    "tail2_split_by_boundary": [seg(41, "tail"), seg(1, "head", length=64)],  # V 42
    "tail3_split_by_empty_segment": [seg(42), seg(0), seg(1, length=64)],  # V 43: two in seg 0, none in seg 1, one in seg 2
}
TAIL_SCENES = ("tail1_alone_behind_boundary", "tail2_split_by_boundary", "tail3_split_by_empty_segment")


def scene_rcp(orc, name):
    """the reciprocal mode whose validity flags a scene is built from and has its property under: Q7 exists in the host-rcpps mode
    alone, and that mode's projection moves a few points across the validity bounds, so the tail scenes are built from the
    oracle's RCP_SSE flags on the host that runs them; every other scene from the exact mode's"""
    return orc.RCP_SSE if name in TAIL_SCENES else orc.RCP_EXACT


def wanted(name):
    """(points walked, valid points per segment) of a scene"""
    segs = SCENES[name]
    assert all(length == SEG for length, _, _ in segs[:-1]) and sum(length for length, _, _ in segs) % 2 == 0, name
    return sum(length for length, _, _ in segs), [n for _, n, _ in segs]


def segment_counts(valid):
    """valid points per 256-point segment of a walked stream"""
    v = np.asarray(valid, bool)
    return [int(v[i:i + SEG].sum()) for i in range(0, len(v), SEG)]


def _between(c, width, empty_only_inside):
    """some run of `width` empty segments has a non-empty segment before and behind it (inside one block if asked)"""
    for i in range(1, len(c) - width):
        if all(x == 0 for x in c[i:i + width]) and c[i - 1] > 0 and c[i + width] > 0:
            if not empty_only_inside or (i - 1) // 4 == (i + width) // 4:
                return True
    return False


def _empty_block_between(c):
    blocks = [sum(c[i:i + 4]) for i in range(0, len(c), 4)]
    return any(blocks[i] == 0 and blocks[i - 1] > 0 and blocks[i + 1] > 0 for i in range(1, len(blocks) - 1))


def _single_after(c, parity):
    return any(c[i] == 1 and c[i - 1] > 0 and c[i - 1] % 2 == parity for i in range(1, len(c)))


def _odd_run(c):
    best = run = 0
    for x in c:
        run = run + 1 if x % 2 else 0
        best = max(best, run)
    return best


def _rank_starts(c):
    return list(np.cumsum([0] + c[:-1]))


def _cut_segment(c):
    """the segment that holds the valid point of rank 50 floor(V / 50) (the first one the likelihood drops), or None"""
    V, starts = sum(c), _rank_starts(c)
    cut = 50 * (V // 50)
    return next((i for i in range(len(c)) if starts[i] <= cut < starts[i] + c[i]), None)


def _tail_segments(v):
    """the segments of the last V mod 4 valid points"""
    at = np.flatnonzero(v)
    t = len(at) % 4
    return [int(p) // SEG for p in at[len(at) - t:]] if t else []


# name -> predicate(valid flags of the walked stream, segment counts): the property the scene is named for
PROPERTIES = {
    "empty_segment_in_block": lambda v, c: _between(c, 1, True),
    "empty_block": lambda v, c: _empty_block_between(c),
    "single_points_and_odd_runs": lambda v, c: _single_after(c, 1) and _single_after(c, 0) and _odd_run(c) >= 3,
    "edge_lanes": lambda v, c: np.flatnonzero(v)[0] % SEG == SEG - 1 and np.flatnonzero(v)[-1] % SEG == 0 and sum(c) > 6,
    "v_multiple_of_50": lambda v, c: sum(c) > 0 and sum(c) % 50 == 0,
    "v_49_mod_50": lambda v, c: sum(c) % 50 == 49,
    "cut_at_segment_start": lambda v, c: 0 < 50 * (sum(c) // 50) < sum(c) and 50 * (sum(c) // 50) in _rank_starts(c)[1:],
    "cut_behind_empty_segment": lambda v, c: _cut_segment(c) is not None and _cut_segment(c) >= 2 and c[_cut_segment(c) - 1] == 0
    and sum(c[:_cut_segment(c) - 1]) > 0,
    "v5": lambda v, c: sum(c) == 5 and len(v) > 100,
    "v6": lambda v, c: sum(c) == 6 and len(v) > 100,
    "v7": lambda v, c: sum(c) == 7 and len(v) > 100,
    # (one tail point cannot be split: it is the only valid point of its segment, the body ends in the segment before)
    "tail1_alone_behind_boundary": lambda v, c: sum(c) % 4 == 1 and c[_tail_segments(v)[0]] == 1 and c[_tail_segments(v)[0] - 1] > 0,
    "tail2_split_by_boundary": lambda v, c: sum(c) % 4 == 2 and _tail_segments(v)[1] == _tail_segments(v)[0] + 1,
    "tail3_split_by_empty_segment": lambda v, c: sum(c) % 4 == 3 and _tail_segments(v)[2] == _tail_segments(v)[1] + 2
    and c[_tail_segments(v)[1] + 1] == 0,
}
assert sorted(PROPERTIES) == sorted(SCENES)


def frames(synth):
    """((Ir, Zr), (Ic, Zc), (Ic, Zc with the stripes), K, ground-truth pose): the small pair -- a small real motion, never a frame against itself --
    and its current frame with the depth of 7 of every 16 level-1 columns removed"""
    (Ir, Zr), (Ic, Zc), Tgt = synth.make_pair(W, H, xi_gt=synth.XI_GT_PAIR * 0.5)
    Zg = Zc.copy()
    Zg[:, (np.arange(W) >> LEVEL) % STRIPE_PERIOD >= STRIPE_KEPT] = np.nan
    return (Ir, Zr), (Ic, Zc), (Ic, Zg), synth.intrinsics_for(W, H), Tgt


def keep_plane_for(index, valid, segments):
    """the level's keep plane (h x w, uint8) whose kept pixels, in scan order, form the scene's segments: index = pixel of every
    selected point in scan order, valid = the oracle's flag of each (the unmasked selection's walked points).  One walk over the
    selection: a segment takes the next points it still has room for -- n_valid valid ones and length - n_valid others --, or, where
    it wants its flags in exact places, for every wanted flag the next point that has it."""
    index, valid = np.asarray(index)[: len(valid)], np.asarray(valid, bool)
    cursor, taken = 0, []
    for length, n_valid, flags in segments:
        room = {True: n_valid, False: length - n_valid}
        placed = 0
        while placed < length:
            assert cursor < len(valid), "the striped frame runs out of points: %d placed" % len(taken)
            f = bool(valid[cursor])
            if room[f] and (flags is None or bool(flags[placed]) == f):
                taken.append(cursor)
                room[f] -= 1
                placed += 1
            cursor += 1
    keep = np.zeros((H >> LEVEL) * (W >> LEVEL), np.uint8)
    keep[index[taken]] = 1
    return keep.reshape(H >> LEVEL, W >> LEVEL)


class Oracle:
    """the oracle's side of every case: pyramids with their keep planes, built once and left unchanged.
    counted[n] / gappy[name] = (reference pyramid with its keep plane, current pyramid, the level's keep plane)"""

    def __init__(self, orc, synth):
        (Ir, Zr), (Ic, Zc), (_, Zg), K, self.Tgt = frames(synth)
        self.cur, self.cur_gappy = orc.Pyramid(Ic, Zc, K, LEVELS), orc.Pyramid(Ic, Zg, K, LEVELS)
        probe = orc.Pyramid(Ir, Zr, K, LEVELS)
        _, index = probe.select(LEVEL)
        selected = np.zeros((H >> LEVEL) * (W >> LEVEL), np.uint8)
        selected[index] = 1
        self.selected = selected.reshape(H >> LEVEL, W >> LEVEL)
        valid = {rcp: orc.compute_residuals(probe, self.cur_gappy, LEVEL, np.eye(4), rcp)[2] for rcp in (orc.RCP_EXACT, orc.RCP_SSE)}
        self.counted, self.gappy = {}, {}
        for n in COUNTS:
            keep = counted.count_mask_planes(self.selected, n)[LEVEL]
            self.counted[n] = (self._reference(orc, Ir, Zr, K, keep), self.cur, keep)
        for name in SCENES:
            keep = keep_plane_for(index, valid[scene_rcp(orc, name)], SCENES[name])
            self.gappy[name] = (self._reference(orc, Ir, Zr, K, keep), self.cur_gappy, keep)

    @staticmethod
    def _reference(orc, Ir, Zr, K, keep):
        p = orc.Pyramid(Ir, Zr, K, LEVELS)
        p.set_keep(LEVEL, keep)
        return p

    def cases(self):
        """[(case name, reference, current, keep plane)]: the counted cases, then the gappy ones"""
        return [(f"n{n}",) + self.counted[n] for n in COUNTS] + [(name,) + self.gappy[name] for name in SCENES]


def case_names():
    return [f"n{n}" for n in COUNTS] + list(SCENES)


class Device:
    """the library's side: one reference pyramid per case (a pyramid caches at most eight masked selections), the two current
    pyramids, and each case's selection mask from the oracle side's keep plane"""

    def __init__(self, capi, synth, oracle_side):
        (Ir, Zr), (Ic, Zc), (_, Zg), K, _ = frames(synth)
        cur, cur_gappy = capi.RgbdImagePyramid(Ic, Zc, K, LEVELS), capi.RgbdImagePyramid(Ic, Zg, K, LEVELS)
        self.cases = {}
        for name, _, o_cur, keep in oracle_side.cases():
            mask = capi.SelectionMask.from_levels([np.ones((H, W), np.uint8), keep])
            self.cases[name] = (capi.RgbdImagePyramid(Ir, Zr, K, LEVELS), cur_gappy if o_cur is oracle_side.cur_gappy else cur, mask)
