"""The pose-graph linear solvers held to a residual bar at their tile and front-tier edges: the tiled dense Cholesky
(k_potrf_panel, k_trsm, k_syrk, k_trsv), the multifrontal path (k_front_assemble / _factor / _forward / _backward and the tiled kernels on wide
fronts), the packed Cholesky of k_optimize_batch and the selected inversion behind the marginals.

The systems are the device's own H and b (H itself is held to the restatement elsewhere), so a bar here isolates the solve.  The
measures, their float64 Cholesky yardstick and the factor 8 between them are in pose_graph_solver_cases.py; the graphs are
dense-fill (complete graphs: every tile the kernels touch is populated) at sizes that put n = 6 m on, just under and just over
the tile (64) and front-tier (192 pivots, ld 1024) edges.  Every GPU test prints the device's and the yardstick's values."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_marginals_cases as M  # noqa: E402
import pose_graph_restatement as R  # noqa: E402
import pose_graph_solver_cases as K  # noqa: E402
from test_pose_graph import MARGIN, _compare, to_pose_graph  # noqa: E402
from test_pose_graph_batch import _batch, _bits, _check_one  # noqa: E402
from test_pose_graph_sparse import _H_from_blocks  # noqa: E402

DENSE_SIZES = [1, 10, 11, 21, 22, 32, 33, 64]  # n = 6, 60 | 66, 126 | 132, 192 | 198 | 384: one, two, three, four, six tiles
FRONT_NAMES = list(K.FRONT_GRAPHS)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", DENSE_SIZES)
def test_complete_graph_fills_every_block(m):
    g = K.complete_graph(m)
    assert len(g.free) == m and len(g.edges) == m * (m + 1) // 2
    H = R.linearise(g, K.DELTA)[0]
    peak = np.abs(H.reshape(m, 6, m, 6)).max(axis=(1, 3))
    assert np.all(peak > 0), "a zero 6 x 6 block"


@pytest.mark.parametrize("m", DENSE_SIZES)
def test_measures_on_the_restated_system(m):
    """the measures' self-test: the yardstick scores near one ulp, the tiled restatement is within the bars of it, an exact
    solution scores 0, a solution with one component off by 1e-10 of itself is caught, and the block-wise form is the dense
    one"""
    H, b = R.linearise(K.complete_graph(m), K.DELTA)[:2]
    xr = K.cholesky_reference(H, b)
    ref, tiled = K.measures(H, b, xr), K.measures(H, b, K.tiled_cholesky_solve(H, b))
    print(f"m={m}: yardstick eta {ref[0]:.2e} omega {ref[1]:.2e}; tiled restatement eta {tiled[0]:.2e} omega {tiled[1]:.2e}")
    assert ref[0] <= 4 * K.ULP and ref[1] <= 16 * K.ULP
    assert K.within_bars(tiled, ref)
    # the exact solution of a system built for it has residual 0 in long double: r is not a float64 artefact
    xe = np.round(xr * 2.0 ** 20) / 2.0 ** 20
    He = np.round(H * 2.0 ** 10) / 2.0 ** 10
    be = (np.asarray(He, K.LD) @ np.asarray(xe, K.LD))
    assert np.array_equal(be.astype(np.float64).astype(K.LD), be), "products of 31-bit by 21-bit numbers, summed: exact in fp64"
    assert K.measures(He, be.astype(np.float64), xe) == (0.0, 0.0)
    # one component off by 1e-10 of itself, the row of H whose share |H_ii x_i| of its (|H| |x|)_i is largest
    share = np.abs(np.diag(H) * xr) / (np.abs(H) @ np.abs(xr) + np.abs(b))
    i = int(np.argmax(share))
    xb = xr.copy()
    xb[i] *= 1.0 + 1e-10
    bad = K.measures(H, b, xb)
    assert not K.within_bars(bad, ref) and bad[1] > 1e-10 * share[i] / 2
    rc = np.array([(r, c) for r in range(m) for c in range(m)])
    blocks = H.reshape(m, 6, m, 6).transpose(0, 2, 1, 3).reshape(-1, 6, 6)
    got = K.measures_blocks(rc, blocks, b, xr)
    # the two forms sum the long double products in different orders: each r_i carries up to n 2^-64 (|H| |x|)_i of rounding,
    # 2^-11 n of a residual of float64 size -- sqrt(n) of that as a rule, a few per cent at n = 384 at the very worst
    assert np.allclose(got, ref, rtol=5e-2, atol=0)


@pytest.mark.parametrize("m,drop,orders", [(11, (0, 1, 1, 0, 3), 4), (11, (0, 1, 1, 0, 0), 1), (22, (0, 1, 1, 5, 7), 4),
                                           (22, (0, 2, 1, 3, 60), 4), (22, (1, 2, 2, 0, 63), 4), (33, (1, 3, 2, 2, 31), 4),
                                           (64, (4, 5, 5, 63, 17), 4)])
def test_seeded_defect_fails_the_bars(m, drop, orders):
    """one product term lost from the entries of one row of one trailing-update tile (a real row: padded rows are exempt
    below) fails the bars, by four orders and more as a rule; the intact factorization passes them.  The second case loses
    the weakest term there is (a translation column against a rotation row, n = 66): omega still fails by an order, while eta
    stays near its bar -- the reason both are held."""
    H, b = R.linearise(K.complete_graph(m), K.DELTA)[:2]
    k, i, j, row, term = drop
    assert i * K.TILE + row < 6 * m and j * K.TILE < 6 * m and k * K.TILE + term < 6 * m, "the lost term is not in the padding"
    ref = K.measures(H, b, K.cholesky_reference(H, b))
    good = K.measures(H, b, K.tiled_cholesky_solve(H, b))
    bad = K.measures(H, b, K.tiled_cholesky_solve(H, b, drop))
    print(f"m={m} drop {drop}: yardstick {ref[0]:.2e} {ref[1]:.2e}, intact {good[0]:.2e} {good[1]:.2e}, "
          f"defect {bad[0]:.2e} {bad[1]:.2e}")
    assert K.within_bars(good, ref)
    assert not K.within_bars(bad, ref)
    assert bad[1] > 10.0 ** orders * K.FACTOR * ref[1]
    assert orders < 4 or bad[0] > 1e4 * K.FACTOR * max(ref[0], K.ULP)


def test_seeded_defect_in_a_padded_row_changes_nothing():
    H, b = R.linearise(K.complete_graph(22), K.DELTA)[:2]  # n = 132: rows 4 .. 63 of tile 2 are padding
    x = K.tiled_cholesky_solve(H, b)
    assert K.tiled_cholesky_solve(H, b, (0, 2, 2, 10, 7)).tobytes() == x.tobytes()
    assert K.tiled_cholesky_solve(H, b, (0, 2, 2, 3, 7)).tobytes() != x.tobytes()  # row 3 is the last real one


def _is_wide(p, u):
    return K.front_layout(p, u)[0]


@pytest.mark.parametrize("name", FRONT_NAMES)
def test_front_census(name):
    k, pendants, want = K.FRONT_GRAPHS[name]
    g = K.front_graph(name)
    assert len(g.free) == k + sum(pendants) <= 180
    got = K.census(g)
    root = len(got) - 1
    assert sorted((p, u) for p, u, _ in got[:-1]) == sorted(want[:-1]) and got[-1][:2] == want[-1]
    assert [q for _, _, q in got] == [root] * root + [-1]
    if name == "ld1020-ld1026-under-p169":
        # the largest small front; a front wide by its ld alone, under a parent wide by its pivots, 6 p no multiple of 64
        assert K.front_layout(1, 169) == (False, 6, 1020)
        assert K.front_layout(2, 169) == (True, 64, 1088) and 6 * 2 <= K.WIDE_PIVOTS and 6 * (2 + 169) == 1026
        assert K.front_layout(169, 0) == (True, 1024, 1024) and 6 * 169 % K.TILE != 0
    elif name == "root-p32":
        assert K.front_layout(32, 0) == (False, 192, 192)
    elif name == "root-p33":
        assert K.front_layout(33, 0) == (True, 256, 256)
    else:
        assert K.front_layout(64, 0) == (True, 384, 384) and 6 * 64 % K.TILE == 0


@pytest.mark.parametrize("m,s,neighbours", [(22, 0, None), (22, 10, None), (22, 11, None), (22, 21, None),
                                            (22, 10, "all"), (40, 5, None), (40, 17, "all")])
def test_non_pd_graph_fails_at_the_fourth_pivot_of_its_vertex(m, s, neighbours):
    """on the restatement's H: the three rotation rows of slot s are exactly zero and every pivot before 6 s + 3 is positive,
    in the natural order (the dense solver's) -- the zero rows stay zero under any elimination order"""
    g = K.non_pd_graph(m, s, _neighbours(m, s, neighbours))
    H = R.linearise(g, K.DELTA)[0]
    rows = slice(6 * s + 3, 6 * s + 6)
    assert np.all(H[rows, :] == 0.0) and np.all(H[:, rows] == 0.0)
    np.linalg.cholesky(H[:6 * s + 3, :6 * s + 3])
    rest = np.delete(np.arange(6 * m), np.arange(6 * s + 3, 6 * s + 6))
    np.linalg.cholesky(H[np.ix_(rest, rest)])  # everything but the zero rows is positive definite


def _neighbours(m, s, neighbours):
    return [q for q in range(m) if q != s] if neighbours == "all" else neighbours


def test_debug_system_without_H_argument_path():
    """with_H=False hands the entry NULL for H and returns None for it; without a device the call is refused before anything
    is written (there is no CPU path)"""
    from dvo_slam_amd import capi, graph

    pg = to_pose_graph(K.complete_graph(2))
    if graph._lib().dvo_amd_device_count() > 0:
        t = capi.DenseTracker()
        H, b, x, F, fp = pg.debug_system(t)
        H0, b0, x0, F0, fp0 = pg.debug_system(t, with_H=False)
        assert H0 is None and H.shape == (12, 12) and (F0, fp0) == (F, fp)
        assert b0.tobytes() == b.tobytes() and x0.tobytes() == x.tobytes()
        return
    for with_H in (True, False):
        with pytest.raises(capi.DvoAmdError) as ei:
            pg.debug_system(types.SimpleNamespace(_h=None), with_H=with_H)
        assert ei.value.status == 2


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trk():
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    return capi.DenseTracker()


def _held(tag, got, ref):
    """print the device's and the yardstick's measures and the ratios DESIGN.md records, then hold the bars"""
    re, ro = K.ratios(got, ref)
    print(f"solver-edges {tag}: device eta {got[0]:.3e} omega {got[1]:.3e}; yardstick eta {ref[0]:.3e} omega {ref[1]:.3e}; "
          f"ratio eta {re:.2f} omega {ro:.2f}")
    assert K.within_bars(got, ref), (tag, got, ref)


def _both_systems(trk, g):
    """the dense and the sparse entry on g: (H, b, x dense, x sparse), after the bit-equality of the two systems"""
    pg = to_pose_graph(g)
    H, b, x, F, fp = pg.debug_system(trk, K.DELTA)
    rc, blocks, bs, xs, Fs, fps = pg.debug_system_sparse(trk, K.DELTA)
    assert fp < 0 and fps < 0 and F == Fs
    assert _H_from_blocks(rc, blocks, len(g.free)).tobytes() == H.tobytes() and bs.tobytes() == b.tobytes()
    return H, b, x, xs


@pytest.mark.gpu
@pytest.mark.parametrize("m", DENSE_SIZES)
def test_gpu_dense_fill_solves_at_the_tile_edges(trk, m):
    g = K.complete_graph(m)
    H, b, x, xs = _both_systems(trk, g)
    assert H.shape == (6 * m, 6 * m) and np.all(np.abs(H.reshape(m, 6, m, 6)).max(axis=(1, 3)) > 0)
    ref = K.measures(H, b, K.cholesky_reference(H, b))
    _held(f"complete m={m} dense", K.measures(H, b, x), ref)
    _held(f"complete m={m} sparse", K.measures(H, b, xs), ref)


@pytest.mark.gpu
def test_gpu_dense_solve_at_the_cap(trk):
    """1024 free vertices: n = 6144 = 96 tiles, no padding, k_trsv's LDS vector full.  H is left out of the dense entry (302 MB)
    and rebuilt from the sparse entry's blocks, whose bits test_gpu_sparse_system_matches_dense_bits proves equal the dense H;
    the residual is formed block-wise in long double; the yardstick is the dense float64 Cholesky of that H."""
    from dvo_slam_amd import graph

    g = K.ring_with_chords(graph.MAX_FREE_VERTICES)
    m = len(g.free)
    assert m == graph.MAX_FREE_VERTICES and 6 * m % K.TILE == 0
    pg = to_pose_graph(g)
    H0, b, x, F, fp = pg.debug_system(trk, K.DELTA, with_H=False)
    rc, blocks, bs, xs, Fs, fps = pg.debug_system_sparse(trk, K.DELTA)
    assert H0 is None and fp < 0 and fps < 0 and F == Fs and bs.tobytes() == b.tobytes()
    ref = K.measures_blocks(rc, blocks, b, K.cholesky_reference(_H_from_blocks(rc, blocks, m), b))
    _held("cap m=1024 dense", K.measures_blocks(rc, blocks, b, x), ref)
    _held("cap m=1024 sparse", K.measures_blocks(rc, blocks, b, xs), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FRONT_NAMES)
def test_gpu_solves_at_the_front_tier_edges(trk, name):
    g = K.front_graph(name)
    H, b, x, xs = _both_systems(trk, g)
    ref = K.measures(H, b, K.cholesky_reference(H, b))
    d, s = K.measures(H, b, x), K.measures(H, b, xs)
    _held(f"fronts {name} dense", d, ref)
    _held(f"fronts {name} sparse", s, ref)
    # two solutions with backward errors eta_d, eta_s are each within cond(H) eta |x| of the exact one
    cond = np.linalg.cond(H, np.inf)
    gap, bound = np.max(np.abs(x - xs)), cond * (d[0] + s[0]) * max(np.max(np.abs(x)), np.max(np.abs(xs)))
    print(f"solver-edges fronts {name}: cond_inf {cond:.2e}, |x_dense - x_sparse|_inf {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound


@pytest.fixture(scope="module")
def good_system():
    """a good system and its x from both entries on a fresh context each"""
    from dvo_slam_amd import capi

    if capi.lib().dvo_amd_device_count() < 1:
        pytest.skip("needs a GPU")
    g = K.complete_graph(22)
    x = to_pose_graph(g).debug_system(capi.DenseTracker(), K.DELTA)[2]
    xs = to_pose_graph(g).debug_system_sparse(capi.DenseTracker(), K.DELTA)[3]
    assert x is not None and xs is not None
    return g, x, xs


def _context_is_clean(trk, good_system):
    g, x, xs = good_system
    assert to_pose_graph(g).debug_system(trk, K.DELTA)[2].tobytes() == x.tobytes(), "the dense entry after a failed pivot"
    assert to_pose_graph(g).debug_system_sparse(trk, K.DELTA)[3].tobytes() == xs.tobytes(), "the sparse entry after it"


@pytest.mark.gpu
@pytest.mark.parametrize("s", [0, 10, 11, 21])
def test_gpu_dense_failed_pivot_is_the_index(trk, good_system, s):
    """m = 22, three tiles: index 3; 63, the last column of tile 0; 69, the first failure behind a k_trsm / k_syrk sweep; 129,
    in the last tile"""
    g = K.non_pd_graph(22, s)
    H, b, x, F, fp = to_pose_graph(g).debug_system(trk, K.DELTA)
    rows = slice(6 * s + 3, 6 * s + 6)
    assert np.all(H[rows, :] == 0.0) and np.all(H[:, rows] == 0.0)
    assert fp == 6 * s + 3 and x is None
    _context_is_clean(trk, good_system)


@pytest.mark.gpu
@pytest.mark.parametrize("m,s,neighbours", [(22, 10, None), (40, 5, None), (22, 10, "all"), (40, 17, "all")],
                         ids=["leaf-beside-small", "leaf-beside-wide", "inside-small-root", "inside-wide-root"])
def test_gpu_sparse_failed_pivot_is_the_index_within_its_front(trk, good_system, m, s, neighbours):
    """the failing vertex hangs on one edge (a leaf front of its own, beside the small or the wide front of the other vertices)
    or keeps an edge to every other vertex (it is then a pivot inside the root front: k_front_factor's index for m = 22,
    k_potrf_panel's for m = 40)"""
    g = K.non_pd_graph(m, s, _neighbours(m, s, neighbours))
    S = K.symbolic_of(g)
    front = [k for k, piv in enumerate(S["pivots"]) if s in piv.tolist()]
    assert len(front) == 1
    k = front[0]
    want = 6 * S["pivots"][k].tolist().index(s) + 3
    root = len(S["parent"]) - 1
    assert S["parent"][root] == -1
    assert any(_is_wide(len(p), len(u)) for p, u in zip(S["pivots"], S["updates"])) == (m == 40)
    if neighbours == "all":
        assert k == root and len(S["pivots"][k]) == m and want > 3
    rc, blocks, b, x, F, fp = to_pose_graph(g).debug_system_sparse(trk, K.DELTA)
    H = _H_from_blocks(rc, blocks, m)
    rows = slice(6 * s + 3, 6 * s + 6)
    assert np.all(H[rows, :] == 0.0) and np.all(H[:, rows] == 0.0)
    print(f"solver-edges failed pivot m={m} s={s}: front {k} of {root + 1} ({len(S['pivots'][k])} pivots), index {fp}")
    assert fp == want and x is None
    _context_is_clean(trk, good_system)


OPT_ITERATIONS = 3


@pytest.mark.gpu
@pytest.mark.parametrize("m", [10, 11, 32])
@pytest.mark.parametrize("solver", ["dense", "sparse"])
@pytest.mark.parametrize("algorithm", ["levenberg", "dogleg"])
def test_gpu_optimizers_on_dense_fill(trk, m, solver, algorithm):
    """the damped path on a fully populated H: k_damp_copy's lambda on the n real rows (a pad pivot stays 1) and
    k_front_assemble's on the pivots, one tile with 4 padded rows, two tiles with 62, three tiles with none.  Three
    iterations: Levenberg damps every one of them, and they take these consistent graphs to the rounding floor of F (the
    restatement's fourth iteration only counts trials there, a hundred of them for the dogleg)."""
    g = K.complete_graph(m)
    res = to_pose_graph(g).optimize(trk, algorithm, iterations=OPT_ITERATIONS, solver=solver)
    o = R.optimize(g, algorithm, iterations=OPT_ITERATIONS, follow=res.iterations, margin=MARGIN)
    _compare(res, o, g, o["F0"])
    assert res.cholesky_failures == 0 and res.final_objective < 1e-10 * res.initial_objective
    print(f"solver-edges optimize m={m} {solver} {algorithm}: {res.n_iterations} iterations, F {res.initial_objective:.3e} -> "
          f"{res.final_objective:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("algorithm", ["levenberg", "dogleg"])
def test_gpu_batch_on_dense_fill(trk, algorithm):
    """k_optimize_batch's packed LDS triangle fully populated: 1, 2, 31 and 32 free vertices in one call, and the 32-vertex
    graph's bits alone against its bits inside a batch"""
    from dvo_slam_amd import graph

    graphs = [K.complete_graph(m) for m in (1, 2, 31, 32)]
    res = _batch(trk, graphs, algorithm, OPT_ITERATIONS)
    for r, g in zip(res, graphs):
        _check_one(r, g, algorithm, OPT_ITERATIONS, consistent=True)
        assert r.cholesky_failures == 0 and r.final_objective < 1e-10 * r.initial_objective
    run = lambda gs: graph.optimize_batch(trk, [to_pose_graph(x) for x in gs], algorithm=algorithm,  # noqa: E731
                                          iterations=OPT_ITERATIONS)
    filler = [K.complete_graph(m) for m in (1, 2, 31, 10, 11, 21)] * 3
    alone = _bits(run([graphs[3]])[0])
    assert alone == _bits(res[3])
    assert _bits(run([graphs[3]] + filler)[0]) == alone, "index 0 of 19"
    assert _bits(run(filler + [graphs[3]])[-1]) == alone, "index 18 of 19"


def _inverse_held(tag, H, got, columns=None):
    """the columns `got` of the device's inverse against the same columns of the float64 Cholesky inverse of H, column by
    column; returns that inverse"""
    Zr = K.cholesky_inverse(H)
    cols = np.arange(H.shape[0]) if columns is None else np.asarray(columns)
    dev, ref = K.inverse_measure(H, got, cols), K.inverse_measure(H, Zr[:, cols], cols)
    ratio = dev / np.maximum(ref, K.ULP)
    print(f"solver-edges {tag}: {len(cols)} columns, device worst {dev.max():.3e}, yardstick worst {ref.max():.3e}, "
          f"worst ratio {ratio.max():.2f}")
    assert np.all(dev <= K.FACTOR * np.maximum(ref, K.ULP)), (tag, float(ratio.max()))
    return Zr


@pytest.mark.gpu
@pytest.mark.parametrize("m", [10, 11, 22, 32, 33])
@pytest.mark.parametrize("solver", ["dense", "sparse"])
def test_gpu_marginals_on_dense_fill(trk, m, solver):
    """the whole Z of a complete graph, every ordered pair of free vertices: one tile (no k_tile_zcol), two, three (its
    symmetric and transposed reads); on the sparse side k_front_selinv at m <= 32 and the tile path at m = 33"""
    g = K.complete_graph(m)
    pg = to_pose_graph(g)
    H = pg.debug_system(trk, K.DELTA)[0]
    pairs = [(a, b) for a in g.free for b in g.free]
    blocks, st = pg.marginals(trk, pairs, solver=solver)
    assert (st.factorized, st.n_free, st.fixed_blocks, st.inactive_blocks, st.solved_columns) == (1, m, 0, 0, 0)
    grid = blocks.reshape(m, m, 6, 6)
    assert grid.transpose(1, 0, 3, 2).tobytes() == grid.tobytes(), "block (b, a) is block (a, b) transposed, bit for bit"
    Z = grid.transpose(0, 2, 1, 3).reshape(6 * m, 6 * m)
    _inverse_held(f"marginals complete m={m} {solver}", H, Z)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FRONT_NAMES)
def test_gpu_sparse_marginals_at_the_front_tier_edges(trk, name):
    """every diagonal block and every edge pair, all from the fronts (k_front_gather_z22 under a wide parent and into a child
    wide by its ld alone).  A vertex of the big clique has an edge to every vertex, so its six columns of Z are complete and
    are held to the residual bar; at 169 clique vertices the long double product behind the bar takes six seconds for all of
    them, so there every fourth clique vertex and the last (two or more per tile column of the root) are scored.  Every
    block is within the marginals' bar of the Cholesky inverse of the device's H."""
    g = K.front_graph(name)
    k = K.FRONT_GRAPHS[name][0]
    pg = to_pose_graph(g)
    H = pg.debug_system(trk, K.DELTA)[0]
    pairs = [(v, v) for v in range(len(g.poses))]
    for f, t, _, _ in g.edges:
        pairs += [(f, t), (t, f)]
    blocks, st = pg.marginals(trk, pairs, solver="sparse")
    assert st.factorized == 1 and st.solved_columns == 0 and st.n_free == len(g.free)
    at = {p: i for i, p in enumerate(pairs)}
    clique = list(range(1, k + 1))
    scored = clique if k <= 64 else sorted(set(clique[::4] + clique[-1:]))
    Zc = np.concatenate([np.concatenate([blocks[at[(a, c)]] for a in g.free], axis=0) for c in scored], axis=1)
    columns = [6 * g.slot[c] + w for c in scored for w in range(6)]
    Zr = _inverse_held(f"marginals fronts {name}", H, Zc, columns)
    d = M.block_rel(blocks, M.expected(g, Zr, pairs))
    print(f"solver-edges marginals fronts {name}: {len(pairs)} blocks, worst distance to the Cholesky inverse {d:.2e}")
    assert d <= M.BAR
