"""Shared pieces of tests/test_counted_selections.py and scripts/record_counted_selections_fixture.py: the cases -- alignments whose residual
pass walks an exactly known number of selected points --, and what of a result the parent fixture keeps.

A selection mask fixes the point count.  The counted cases track level 1 of a 160x120 pair alone: 80 x 60 = 4 800 pixels are 75
wave steps, which the default segment geometry walks in 4-step segments, so a block holds 4 x 4 x 64 = 1 024 points and the counts
sit on both sides of a wave step (63 / 64 / 65) and of a block (1 023 / 1 024 / 1 025).  An odd count's last point is never walked
(the reference's Q3 rule), so 1 walks nothing and 65 walks one full step.  The 80x48 pair runs three levels unmasked; its top level,
20 x 12, is less than a quarter of one block: nearly all of the block is padding."""
import numpy as np

W, H, LEVELS, LEVEL = 160, 120, 2, 1
COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025)
STEPS, BLOCK_POINTS = 4, 1024  # steps per wave segment of LEVEL, points per block (checked on the device by the test)
SMALL = (80, 48, 3)
FIXTURE = "counted_selections_parent.npz"
FIELDS = ("transformation", "information", "log_likelihood", "iterations", "valid_pixels")


def case_names():
    return [f"n{n}" for n in COUNTS] + ["w%dh%d" % SMALL[:2]]


def count_mask_planes(selected: np.ndarray, n: int):
    """mask planes (level 0: keep all, level 1: n pixels) that keep n of level 1's selected pixels, spread evenly over the scan order"""
    at = np.flatnonzero(selected.ravel())
    assert at.size >= n, (at.size, n)
    keep = np.zeros(selected.size, np.uint8)
    if n:
        keep[at[np.round(np.linspace(0, at.size - 1, n)).astype(np.int64)]] = 1
    assert int(keep.sum()) == n
    return [np.ones((H, W), np.uint8), keep.reshape(selected.shape)]


class Scene:
    """the pyramids, masks and trackers of every case on one device; reference pyramids are per case (a pyramid caches at most
    eight masked selections)"""

    def __init__(self, capi, synth):
        self.capi = capi
        (Ir, Zr), (Ic, Zc), _ = synth.make_pair(W, H, xi_gt=synth.XI_GT_PAIR * 0.5)
        K = synth.intrinsics_for(W, H)
        self.cur = capi.RgbdImagePyramid(Ic, Zc, K, LEVELS)
        probe = capi.RgbdImagePyramid(Ir, Zr, K, LEVELS)
        n_sel, selected = probe.select(LEVEL)
        assert n_sel >= max(COUNTS), n_sel
        self.refs, self.masks = {}, {}
        for n in COUNTS:
            self.refs[n] = capi.RgbdImagePyramid(Ir, Zr, K, LEVELS)
            self.masks[n] = capi.SelectionMask.from_levels(count_mask_planes(selected, n))
            assert self.refs[n].select(LEVEL, mask=self.masks[n])[0] == n
        w, h, levels = SMALL
        (Ir, Zr), (Ic, Zc), _ = synth.make_pair(w, h, xi_gt=synth.XI_GT_PAIR * 0.5)
        K = synth.intrinsics_for(w, h)
        self.small_ref, self.small_cur = capi.RgbdImagePyramid(Ir, Zr, K, levels), capi.RgbdImagePyramid(Ic, Zc, K, levels)

    def trackers(self, mode="exact"):
        """(the tracker of the counted cases, the tracker of the 80x48 pair)"""
        out = (self.capi.DenseTracker(self.capi.Config(FirstLevel=LEVEL, LastLevel=LEVEL)),
               self.capi.DenseTracker(self.capi.Config(FirstLevel=SMALL[2] - 1, LastLevel=0)))
        for t in out:
            t.set_reciprocal_mode(mode)
        return out

    def pairs(self):
        """[(case name, reference, current, mask or None, which tracker)]"""
        out = [(f"n{n}", self.refs[n], self.cur, self.masks[n], 0) for n in COUNTS]
        out.append(("w%dh%d" % SMALL[:2], self.small_ref, self.small_cur, None, 1))
        return out

    def singles(self, mode="exact"):
        """{case name: Result of a single match()}"""
        trk = self.trackers(mode)
        return {name: trk[which].match(ref, cur, mask=mask) for name, ref, cur, mask, which in self.pairs()}


def summary(result):
    """what the parent fixture keeps of a result, as arrays"""
    return {
        "transformation": np.asarray(result.Transformation, np.float64),
        "information": np.asarray(result.Information, np.float64),
        "log_likelihood": np.asarray([result.LogLikelihood], np.float64),
        "iterations": np.asarray([len(lv["Iterations"]) for lv in result.Levels], np.int64),
        "valid_pixels": np.asarray([lv["ValidPixels"] for lv in result.Levels], np.int64),
    }


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
