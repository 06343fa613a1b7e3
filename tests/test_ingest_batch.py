"""dvo_amd_pyramid_create_raw_batch on the GPU: N pyramids from one call are, bit for bit, the N pyramids of N
dvo_amd_pyramid_create_raw calls -- planes, first selection, and everything a tracker computes from them -- and the call's launch
count does not depend on N.

Frames are synth.sensor_frame's (8-bit image, uint16 depth), every frame of a batch a different one, so a mix-up of frame indices
shows.  Shapes (tests/ingest_batch_cases.py): 8x4 with 2 levels (the smallest pyramid there is; everything in a fraction of one
block), 320x24 with 3 (rows longer than a 256-pixel block), 528x40 with 3 (level 0's 21 120 pixels cross one 16 384-pixel pad unit).
The yardstick throughout is the single-frame path in the same process: no tolerance anywhere, np.array_equal with NaNs at equal
positions."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ingest_batch_cases import SCALE, SHAPES, compile_example, create_raw_batch, frames, wide  # noqa: E402

pytestmark = pytest.mark.gpu
SEL = (3.0, 0.02)  # selection thresholds that leave some pixels out at every level
INVALID = 1


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c

    if c.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return c


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def planes_of(p, levels):
    return [[p.plane(l, k) for k in range(6)] for l in range(levels)]


def selection_of(p, levels, sel=SEL):
    return [p.select(l, *sel) for l in range(levels)]


@pytest.fixture(scope="module")
def singles(capi):
    """(shape, channels) -> per frame what the single-frame path makes of it: (the pyramid, its planes, its selection for SEL).
    Computed once per case and left alone: every test below compares against it."""
    cache = {}

    def get(shape, channels):
        if (shape, channels) not in cache:
            fr, K = frames(shape, channels)
            out = []
            for f, (image, depth) in enumerate(fr):
                p = capi.RgbdImagePyramid.from_raw(image, depth, K, SHAPES[shape], depth_scale=SCALE, timestamp=0.25 * f)
                out.append((p, planes_of(p, SHAPES[shape]), selection_of(p, SHAPES[shape])))
            cache[shape, channels] = out
        return cache[shape, channels]

    return get


def assert_equals_single(batched, single, levels, with_selection, what):
    for f, (p, (_, planes, selection)) in enumerate(zip(batched, single)):
        assert p.levels() == levels and p.timestamp() == 0.25 * f, (what, f)
        got = planes_of(p, levels)
        for l in range(levels):
            for k in range(6):
                assert same(got[l][k], planes[l][k]), (what, "frame", f, "level", l, "plane", k)
            if with_selection:
                count, mask = p.select(l, *SEL)
                assert count == selection[l][0] and np.array_equal(mask, selection[l][1]), (what, "frame", f, "level", l, "selection")


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("count", [1, 3, 5])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_batched_pyramids_and_selections_equal_the_single_path(capi, singles, shape, count, channels):
    fr, K = frames(shape, channels)
    levels = SHAPES[shape]
    stamps = [0.25 * f for f in range(count)]
    images, depths = [a for a, _ in fr[:count]], [z for _, z in fr[:count]]
    for selection in (SEL, None):
        batched = capi.RgbdImagePyramid.from_raw_batch(images, depths, K, levels, depth_scale=SCALE, timestamps=stamps, selection=selection)
        assert len(batched) == count
        # (without build_selection the select() inside builds the selection as the single path does: same answer either way)
        assert_equals_single(batched, singles(shape, channels), levels, True, (shape, count, channels, selection))


def test_the_selection_cases_hold_an_odd_an_even_and_an_empty_count(capi, singles):
    """Q3 drops an odd trailing point and an all-zero depth frame selects nothing: the single path's own counts say that the
    frames below take both branches of the rule and the empty case, so the comparison cannot pass by missing them"""
    shape, channels = (320, 24), 1
    levels = SHAPES[shape]
    fr, K = frames(shape, channels)
    images, depths = [a for a, _ in fr], [z for _, z in fr[:4]] + [np.zeros_like(fr[4][1])]
    single = [capi.RgbdImagePyramid.from_raw(a, z, K, levels, depth_scale=SCALE) for a, z in zip(images, depths)]
    want = [selection_of(p, levels) for p in single]
    counts = [[want[f][l][0] for l in range(levels)] for f in range(5)]
    print("single-path counts per frame and level:", counts)
    assert any(c % 2 == 1 for row in counts[:4] for c in row), counts
    assert any(c % 2 == 0 and c > 0 for row in counts[:4] for c in row), counts
    assert counts[4] == [0] * levels
    batched = capi.RgbdImagePyramid.from_raw_batch(images, depths, K, levels, depth_scale=SCALE, selection=SEL)
    for f in range(5):
        for l in range(levels):
            count, mask = batched[f].select(l, *SEL)
            assert count == counts[f][l] and np.array_equal(mask, want[f][l][1]), (f, l)
            assert mask.sum() == count  # (the mask keeps an odd trailing point; the passes do not walk it)
            assert same(batched[f].plane(l, 1), single[f].plane(l, 1))


def _on_device(torch, a, pad, fill, view=None):
    """rows of `a` with `pad` elements behind each in device memory, one element past an aligned address when pad > 0:
    (owner, pointer, row length in elements)"""
    rows, length = wide(a, pad, fill)
    flat = rows.reshape(-1) if view is None else rows.view(view).reshape(-1)
    lead = 1 if pad else 0
    buf = torch.zeros(flat.size + lead, dtype=torch.from_numpy(flat[:1].copy()).dtype, device="cuda")
    buf[lead:] = torch.from_numpy(flat.copy()).cuda()
    return buf, buf.data_ptr() + lead * flat.itemsize, length


@pytest.mark.parametrize("pad", [0, 1], ids=["packed", "strided"])
def test_host_and_device_sources_and_strides_give_the_single_path_pyramids(capi, singles, pad):
    """320x24 BGR, three frames: packed rows, and rows of 3 w + 1 bytes / w + 1 depth words (every row but each fourth starts off a
    word boundary, and the device frames start one element past an aligned address: the kernels' unaligned load paths)"""
    torch = pytest.importorskip("torch")
    shape, channels, count = (320, 24), 3, 3
    levels = SHAPES[shape]
    fr, K = frames(shape, channels)
    host_i = [wide(a, pad, 201) for a, _ in fr[:count]]
    host_z = [wide(z, pad, 40000) for _, z in fr[:count]]
    dev_i = [_on_device(torch, a, pad, 201) for a, _ in fr[:count]]
    dev_z = [_on_device(torch, z, pad, 40000, np.int16) for _, z in fr[:count]]
    torch.cuda.synchronize()
    if pad:
        assert all(p % 4 == 1 for _, p, _ in dev_i) and all(p % 8 == 2 for _, p, _ in dev_z)
    istride, zstride = host_i[0][1], host_z[0][1]
    assert (istride, zstride) == (3 * shape[0] + pad, shape[0] + pad)
    stamps = [0.25 * f for f in range(count)]
    for on_device, ip, zp in ((0, [a.ctypes.data for a, _ in host_i], [z.ctypes.data for z, _ in host_z]),
                              (1, [p for _, p, _ in dev_i], [p for _, p, _ in dev_z])):
        rc, batched = create_raw_batch(capi, ip, zp, channels, istride, zstride, on_device, shape, K, levels, SEL, stamps)
        assert rc == 0
        assert_equals_single(batched, singles(shape, channels), levels, True, ("on_device", on_device, "pad", pad))
    if not pad:  # the binding's device form is the same call
        batched = capi.RgbdImagePyramid.from_raw_batch([p for _, p, _ in dev_i], [p for _, p, _ in dev_z], K, levels, depth_scale=SCALE,
                                                       timestamps=stamps, size=shape, channels=channels)
        assert_equals_single(batched, singles(shape, channels), levels, False, "binding, device pointers")


def _same_result(a, b):
    assert np.array_equal(a.Transformation, b.Transformation) and np.array_equal(a.Information, b.Information)
    assert a.LogLikelihood == b.LogLikelihood and a.isNaN() == b.isNaN() and len(a.Levels) == len(b.Levels)
    for la, lb in zip(a.Levels, b.Levels):
        assert (la["Id"], la["ValidPixels"], la["MaxValidPixels"], la["TerminationCriterion"], len(la["Iterations"])) == \
               (lb["Id"], lb["ValidPixels"], lb["MaxValidPixels"], lb["TerminationCriterion"], len(lb["Iterations"]))
        for ia, ib in zip(la["Iterations"], lb["Iterations"]):
            assert ia["ValidConstraints"] == ib["ValidConstraints"] and ia["TDistributionLogLikelihood"] == ib["TDistributionLogLikelihood"]
            assert np.array_equal(ia["EstimateInformation"], ib["EstimateInformation"]) and np.array_equal(ia["estimate"], ib["estimate"])


@pytest.mark.parametrize("with_selection", [True, False])
def test_a_tracker_computes_the_same_from_batched_and_single_pyramids(capi, synth, singles, with_selection):
    """match on pairs, match_batch over the consecutive pairs and residuals at a pose that is not the identity, on five batched
    528x40 pyramids and on the five singly created ones: pose, information matrix and per-level statistics bit for bit"""
    shape, channels, count = (528, 40), 1, 5
    levels = SHAPES[shape]
    fr, K = frames(shape, channels)
    cfg = capi.Config(FirstLevel=levels - 1, LastLevel=0, IntensityDerivativeThreshold=SEL[0], DepthDerivativeThreshold=SEL[1])
    trk = capi.DenseTracker(cfg)
    batched = capi.RgbdImagePyramid.from_raw_batch([a for a, _ in fr], [z for _, z in fr], K, levels, depth_scale=SCALE,
                                                   selection=SEL if with_selection else None)
    single = [capi.RgbdImagePyramid.from_raw(a, z, K, levels, depth_scale=SCALE) for a, z in fr]
    for r, c in ((0, 1), (3, 2), (4, 0)):
        _same_result(trk.match(batched[r], batched[c]), trk.match(single[r], single[c]))
    got = trk.match_batch(batched[:-1], batched[1:])
    want = trk.match_batch(single[:-1], single[1:])
    assert len(got) == len(want) == count - 1
    for a, b in zip(got, want):
        _same_result(a, b)
    assert not any(r.isNaN() for r in want)
    T = synth.se3_exp(np.array([0.01, -0.004, 0.006, 0.003, -0.002, 0.004]))
    for level in range(levels):
        (res_b, n_b), (res_s, n_s) = trk.residuals(batched[1], batched[2], level, T), trk.residuals(single[1], single[2], level, T)
        assert n_b == n_s and n_s > 0 and same(res_b, res_s), level


def test_launches_do_not_depend_on_the_frame_count_and_the_call_synchronises_once(capi):
    shape, channels = (320, 24), 3
    levels = SHAPES[shape]
    fr, K = frames(shape, channels)
    seen = {}
    for selection in (None, SEL):
        for count in (1, 5):
            capi.RgbdImagePyramid.from_raw_batch([a for a, _ in fr[:count]], [z for _, z in fr[:count]], K, levels, depth_scale=SCALE,
                                                 selection=selection)
            seen[selection is not None, count] = capi.batch_build_stats()
    print("batch build stats:", seen)
    for with_selection in (False, True):
        one, five = seen[with_selection, 1], seen[with_selection, 5]
        assert one["kernel_launches"] == five["kernel_launches"]
        assert one["synchronisations"] == five["synchronisations"] == 1
        # ingest, a pyr_down per further level, a level_planes per level, the descriptors; select, its finish, the prefix and the
        # compaction per level: a function of the level count alone
        assert one["kernel_launches"] == 1 + (levels - 1) + levels + 1 + (4 * levels if with_selection else 0)
        # copies: two per host frame and the frame table; with a selection, the counters of every frame and level in ONE copy
        assert five["copies"] == 2 * 5 + 1 + (1 if with_selection else 0) and one["copies"] == 2 + 1 + (1 if with_selection else 0)
    other_levels = capi.RgbdImagePyramid.from_raw_batch([fr[0][0]], [fr[0][1]], K, levels - 1, depth_scale=SCALE, selection=SEL)
    assert capi.batch_build_stats()["kernel_launches"] == 6 * (levels - 1) + 1 and len(other_levels) == 1


def test_a_match_with_the_batch_thresholds_builds_no_selection(capi):
    """dvo_amd_debug_ingest_timing brackets every pyramid build and every selection build.  After a batch with build_selection the
    bracket still holds the batch's time when a match with those thresholds has run: the match found the selection in the cache.
    After a batch without, the match builds it and the bracket moves (two fresh batches: two device times that happen to be
    equal to the last bit would hide one move, not two)."""
    shape, channels = (320, 24), 1
    levels = SHAPES[shape]
    fr, K = frames(shape, channels)
    trk = capi.DenseTracker(capi.Config(FirstLevel=levels - 1, LastLevel=0, IntensityDerivativeThreshold=SEL[0],
                                        DepthDerivativeThreshold=SEL[1]))
    images, depths = [a for a, _ in fr[:2]], [z for _, z in fr[:2]]
    capi.ingest_timing(True)
    try:
        moved = []
        for selection in (SEL, None, None):
            ref, cur = capi.RgbdImagePyramid.from_raw_batch(images, depths, K, levels, depth_scale=SCALE, selection=selection)
            before = capi.ingest_timing(True)
            assert before > 0.0
            result = trk.match(ref, cur)
            after = capi.ingest_timing(True)
            assert not result.isNaN()
            if selection is not None:
                assert after == before
            else:
                moved.append(after != before)
        assert any(moved)
    finally:
        capi.ingest_timing(False)


def test_a_refused_call_leaves_earlier_pyramids_alone(capi, singles):
    shape, channels, count = (528, 40), 3, 3
    levels = SHAPES[shape]
    fr, K = frames(shape, channels)
    stamps = [0.25 * f for f in range(count)]
    ip, zp = [a.ctypes.data for a, _ in fr[:count]], [z.ctypes.data for _, z in fr[:count]]
    rc, batched = create_raw_batch(capi, ip, zp, channels, 3 * shape[0], shape[0], 0, shape, K, levels, SEL, stamps)
    assert rc == 0
    for bad in (dict(channels=2), dict(levels=9), dict(selection=(float("nan"), 0.0))):
        a = dict(channels=channels, levels=levels, selection=SEL)
        a.update(bad)
        rc, none = create_raw_batch(capi, ip, zp, a["channels"], 3 * shape[0], shape[0], 0, shape, K, a["levels"], a["selection"], stamps)
        assert rc == INVALID and none is None, bad  # (create_raw_batch has looked at `out`: every entry NULL)
    assert_equals_single(batched, singles(shape, channels), levels, True, "after refused calls")


def _checksum(plane):
    words = np.ascontiguousarray(plane, np.float32).view(np.uint32).copy()
    words[np.isnan(plane)] = 0x7FC00000
    h = 0
    for word in words.reshape(-1).tolist():
        h = (h * 31 + word) & 0xFFFFFFFF
    return h


@pytest.mark.parametrize("kind", ["cpp", "mock"])
def test_adaptor_create_raw_batch_prints_the_single_paths_planes(capi, kind):
    """examples/batch_ingest_adaptor_example.cpp: RgbdImagePyramid::createRawBatch on three frames; the checksums of every level's
    intensity and depth plane are those of the Python binding's single-frame pyramids of the same frames"""
    w, h, n, levels = 72, 50, 3, 2
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    lines = []
    for f in range(n):
        bgr = np.stack([(3 * u + 5 * v + 17 * f) % 256, (7 * u + v + 29 * f) % 256, (u + 11 * v + 5 * f) % 256], -1).astype(np.uint8)
        depth = np.where((u + 2 * v + f) % 9 == 0, 0, 5000 + 130 * u + 70 * v + 300 * f).astype(np.uint16)
        p = capi.RgbdImagePyramid.from_raw(bgr, depth, (60.0, 60.0, 35.5, 24.5), levels, depth_scale=SCALE)
        for l in range(levels):
            lw, lh, _ = p.level_info(l)
            lines.append("frame %d level %d: %d x %d intensity %08x depth %08x" % (f, l, lw, lh, _checksum(p.plane(l, 0)), _checksum(p.plane(l, 1))))
    res = subprocess.run([compile_example(kind)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.splitlines() == lines


def test_c_example_aligns_its_consecutive_pairs(capi):
    res = subprocess.run([compile_example("c")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == 5 and all(line.startswith("pair %d -> %d" % (k, k + 1)) and "isnan 0" in line for k, line in enumerate(lines))


def test_tum_load_batch_equals_load_of_each_entry(capi, tmp_path):
    """tum.load_batch: the PNGs of three association entries decoded on the host, one batched build; each pyramid is load()'s of
    that entry, with the entry's timestamp"""
    from dvo_slam_amd import tum
    from test_tum import write_png

    shape, levels = (320, 24), SHAPES[(320, 24)]
    fr, K = frames(shape, 3)
    os.makedirs(str(tmp_path / "rgb")), os.makedirs(str(tmp_path / "depth"))
    entries = []
    for f, (bgr, z) in enumerate(fr[:3]):
        write_png(str(tmp_path / "rgb" / f"{f}.png"), bgr[..., ::-1], 8, 2, filters=[1, 2, 4])
        write_png(str(tmp_path / "depth" / f"{f}.png"), z[..., None], 16, 0, filters=[2, 1])
        entries.append(tum.RgbdPair(10.0 + f, f"rgb/{f}.png", 10.0 + f, f"depth/{f}.png"))
    batched = tum.load_batch(entries, K, levels, base=str(tmp_path), selection=SEL)
    assert len(batched) == 3
    for f, e in enumerate(entries):
        one = tum.load(K, str(tmp_path / e.RgbFile), str(tmp_path / e.DepthFile), levels, timestamp=e.RgbTimestamp)
        assert batched[f].timestamp() == one.timestamp() == 10.0 + f
        for l in range(levels):
            for k in range(6):
                assert same(batched[f].plane(l, k), one.plane(l, k)), (f, l, k)
            assert batched[f].select(l, *SEL)[0] == one.select(l, *SEL)[0]
