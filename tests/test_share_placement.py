"""Where the blocks of a k_tick launch go (csrc/dvo_kernels.hip: tick_items_order, tick_args_layout, tick_locate) under the three
values of DVO_AMD_SHARE_PLACEMENT: 0 = every item placed on its own, 1 = the pairs of one keyframe level ("a set") next to each
other in the launch with one XCD rotation, 2 = ... and dispatched interleaved.  Host logic only, no GPU: the library lays
synthetic item lists out and restates the kernel's block -> (item, block) arithmetic (dvo_amd_debug_tick_layout).

Placement may only move work between XCDs and in time: every block of every item must still be run exactly once."""
import numpy as np
import pytest

SHARES = (0, 1, 2)
# (residual blocks, steps per wave segment) of the four levels of a 640x480 pyramid, as level_blocks / level_steps give them
LEVELS = [(271, 10), (43, 16), (11, 16), (3, 16)]


@pytest.fixture(scope="module")
def capi():
    from dvo_slam_amd import capi as c
    c.lib()
    return c


def tracker_like(n=62, n_refs=12, seed=0):
    """n resident pairs of a tracker: pair i = (keyframe i % n_refs, current frame i // n_refs), each somewhere in its descent
    through the levels, with a likelihood pass of the same or the previous level's size"""
    rng = np.random.default_rng(seed)
    rb, lb, st, rk, ck = [], [], [], [], []
    for i in range(n):
        lv = int(rng.integers(0, 4))
        blocks, steps = LEVELS[lv]
        ll_of = LEVELS[min(3, lv + int(rng.integers(0, 2)))][0]
        rb.append(blocks), st.append(steps), lb.append((ll_of + 3) // 4 if rng.random() < 0.9 else 0)
        rk.append((i % n_refs) * 4 + lv), ck.append((i // n_refs) * 4 + lv)
    return rb, lb, st, rk, ck


def random_items(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 63))
    steps = rng.choice([1, 2, 4, 8, 10, 16, 20, 32], size=n)
    rk = rng.integers(0, max(1, n // 3), size=n)
    # the pairs of one reference level have the same number of points, hence of blocks
    blocks_of_ref = rng.integers(0, 300, size=n)
    blocks_of_ref[0] = rng.integers(1200, 2049)  # one fine level among coarse ones, as in a tracker: the compact grid
    rb = [int(blocks_of_ref[k]) for k in rk]
    st = [int(steps[k]) for k in rk]
    lb = [int(x) for x in rng.integers(0, 80, size=n)]
    for i in range(n):
        if rb[i] + lb[i] == 0:
            lb[i] = 1
    return rb, lb, st, [int(k) for k in rk], [int(x) for x in rng.integers(0, 8, size=n)]


def biggest():
    """six pairs of one keyframe level at the largest block counts an item can carry, among 56 coarse ones"""
    n, m = 6, 56
    return [2048] * n + [3] * m, [2048 - (i % 5) for i in range(n)] + [1] * m, [10] * n + [16] * m, \
        [7] * n + [8 + i % 9 for i in range(m)], list(range(n + m))


def equal_items():
    """24 pairs of one shape: the two-dimensional grid (no block of it would be idle), which has no sets"""
    n = 24
    return [271] * n, [68] * n, [10] * n, [i % 4 for i in range(n)], list(range(n))


CASES = [tracker_like(62, 12, 0), tracker_like(62, 12, 1), tracker_like(31, 12, 2), tracker_like(40, 3, 3), biggest()] + \
        [random_items(s) for s in range(40)]
CASES.append(equal_items())


def goes_out_compact(rb, lb):
    """tick_args_layout's rule: the one-dimensional grid when more than half of (blocks of the largest item x items) would be idle"""
    own = sum((r + l + 7) >> 3 for r, l in zip(rb, lb))
    return 2 * 8 * own < ((max(r + l for r, l in zip(rb, lb)) + 7) & ~7) * len(rb)


COMPACT = [goes_out_compact(c[0], c[1]) for c in CASES]
assert COMPACT[:5] == [True] * 5 and not COMPACT[-1] and sum(COMPACT) > 30


def sets_of(lay, items):
    """the sets as the layout defines them: runs of launch neighbours with the same reference level and residual geometry"""
    rb, lb, st, rk, ck = items
    o = lay["order"]
    runs, k = [], 0
    while k < len(o):
        j = k + 1
        while j < len(o) and rb[o[k]] > 0 and (rk[o[j]], rb[o[j]], st[o[j]]) == (rk[o[k]], rb[o[k]], st[o[k]]):
            j += 1
        runs.append((k, j))
        k = j
    return runs


@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_every_block_of_every_item_runs_exactly_once(capi, case, share):
    items = CASES[case]
    rb, lb, st, rk, ck = items
    n = len(rb)
    lay = capi.tick_layout(*items, share)
    assert sorted(lay["order"]) == list(range(n))
    assert lay["compact"] == COMPACT[case]
    if not lay["compact"]:  # the two-dimensional grid: (block, item) is the map, and every item is placed on its own
        assert np.array_equal(lay["xcd_rot"], lay["tail_rot"]) and np.all(lay["set_size"] == 1)
        return
    assert lay["group_first"][n] < 65536 and lay["n_blocks"] == 8 * lay["group_first"][n]
    assert np.all(np.diff(lay["group_first"]) >= 0)
    bi, bx = lay["block_item"], lay["block_index"]
    assert len(bi) == lay["n_blocks"] and bi.max() < n and np.all((bi >= 0) == (bx >= 0))
    for k in range(n):
        mine = np.sort(bx[bi == k])
        want = rb[lay["order"][k]] + lb[lay["order"][k]]
        assert len(mine) == want and np.array_equal(mine, np.arange(want)), (k, want, len(mine))
    # a block keeps its place within its group of eight up to the rotation: block b does block (b & ~7 | (b + rot) & 7) of
    # its item's stretch, so blocks b and b + 8 of an item stay on one XCD
    own = bi >= 0
    b = np.arange(len(bi))[own]
    rot = np.where((bx[own] >> 3) < (np.array(rb)[lay["order"]][bi[own]] >> 3), lay["xcd_rot"][bi[own]], lay["tail_rot"][bi[own]])
    assert np.array_equal(bx[own] & 7, (b + rot) & 7)


@pytest.mark.parametrize("share", (1, 2))
@pytest.mark.parametrize("case", range(len(CASES)))
def test_members_of_a_set_are_neighbours_and_share_a_rotation(capi, case, share):
    items = CASES[case]
    rb, lb, st, rk, ck = items
    lay = capi.tick_layout(*items, share)
    o = lay["order"]
    # long blocks first between the classes; inside a class one reference level's items together, by current level
    key = [(-(st[i] if rb[i] else 0), rk[i], ck[i]) for i in o]
    assert key == sorted(key)
    for k0, k1 in sets_of(lay, items):
        if not lay["compact"]:
            break
        assert len(set(lay["xcd_rot"][k0:k1])) == 1, (k0, k1)
        if share == 2 and lay["compact"] and k1 - k0 > 1:
            m = k1 - k0
            assert lay["set_size"][k0] == m and np.all(lay["set_size"][k0 + 1:k1] == 1)
            # group g of the set is group g // m of member g % m
            g0 = lay["group_first"][k0]
            bi, bx = lay["block_item"], lay["block_index"]
            for k in range(k0, k1):
                blocks = np.flatnonzero(bi == k)
                g = (blocks >> 3) - g0
                assert np.array_equal(g % m, np.full(len(g), k - k0)) and np.array_equal(g // m, bx[blocks] >> 3)
        else:
            assert np.all(lay["set_size"][k0:k1] == 1)


def parent_layout(rb, lb, st):
    """the layout before share placement, restated: items in stable order of falling steps, one rotation per item chosen
    greedily for the smallest maximum XCD load (the first of the tied ones)"""
    n = len(rb)
    order = sorted(range(n), key=lambda i: -(st[i] if rb[i] else 0))
    first, rots, load, groups = [], [], [0] * 8, 0
    for i in order:
        first.append(groups)
        groups += (rb[i] + lb[i] + 7) >> 3
        w_res, w_ll = 33 + 21 * st[i], 40 + 7 * st[i]
        phase = []
        for f in range(8):
            n_res = (rb[i] >> 3) + (f < (rb[i] & 7))
            phase.append(w_res * n_res + w_ll * (((rb[i] + lb[i]) >> 3) + (f < ((rb[i] + lb[i]) & 7)) - n_res))
        best = min(range(8), key=lambda r: (max(load[x] + phase[(x + r) & 7] for x in range(8)), r))
        rots.append(best)
        load = [load[x] + phase[(x + best) & 7] for x in range(8)]
    return order, first + [groups], rots


@pytest.mark.parametrize("case", range(len(CASES)))
def test_share_0_is_the_layout_before_share_placement(capi, case):
    rb, lb, st, rk, ck = CASES[case]
    lay = capi.tick_layout(rb, lb, st, rk, ck, 0)
    order, first, rots = parent_layout(rb, lb, st)
    assert list(lay["order"]) == order and list(lay["group_first"]) == first
    assert list(lay["xcd_rot"]) == rots and list(lay["tail_rot"]) == rots and np.all(lay["set_size"] == 1)


@pytest.mark.parametrize("share", (1, 2))
@pytest.mark.parametrize("seed", range(12))
def test_sets_of_one_reproduce_the_layout_of_share_0(capi, seed, share):
    """every item reads a reference level of its own: nothing to place together.  (The launch order inside a class of equal
    steps is by reference level then; with the keys rising in slot order that is slot order, as under share 0.)"""
    rb, lb, st, _, ck = random_items(100 + seed)
    rk = list(range(len(rb)))
    a, b = capi.tick_layout(rb, lb, st, rk, ck, 0), capi.tick_layout(rb, lb, st, rk, ck, share)
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    order, first, rots = parent_layout(rb, lb, st)
    assert list(b["order"]) == order and list(b["group_first"]) == first and list(b["xcd_rot"]) == rots == list(b["tail_rot"])


def test_the_tracker_like_launch_is_compact_and_has_sets(capi):
    """the flagship's shape: 62 pairs of 12 keyframes; the assertions above must not pass on an empty premise"""
    items = CASES[0]
    for share in SHARES:
        lay = capi.tick_layout(*items, share)
        assert lay["compact"] == 1
        sizes = [k1 - k0 for k0, k1 in sets_of(lay, items)]
        assert (max(sizes) > 1) == (share > 0)
    # the model's XCD loads (the balancer's own weights) for the record: printed, not judged
    rb, lb, st, rk, ck = items
    for share in SHARES:
        lay = capi.tick_layout(*items, share)
        load = np.zeros(8)
        bi, bx = lay["block_item"], lay["block_index"]
        for b in np.flatnonzero(bi >= 0):
            i = lay["order"][bi[b]]
            load[b & 7] += 33 + 21 * st[i] if bx[b] < rb[i] else 40 + 7 * st[i]
        print(f"share {share}: model XCD loads max/min - 1 = {load.max() / load.min() - 1:.4f}, blocks {lay['n_blocks']}")


def test_bad_arguments_are_refused(capi):
    with pytest.raises(capi.DvoAmdError):
        capi.tick_layout([10], [2], [10], [0], [0], 3)
    with pytest.raises(capi.DvoAmdError):
        capi.tick_layout([10], [2], [11], [0], [0], 1)  # no level has eleven steps per segment
    with pytest.raises(capi.DvoAmdError):
        capi.tick_layout([10] * 63, [2] * 63, [10] * 63, [0] * 63, [0] * 63, 1)
