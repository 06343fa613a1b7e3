"""The rules of "Mask components" (include/dvo_amd.h) restated with numpy and scipy.sparse.csgraph, for tests/test_mask_components.py.

Processing.  Each level is processed on its own, from the same level of its inputs.
Foreground.  A pixel is foreground iff (mask is None or mask != 0) and (depth is None or depth is finite).
Edges.  Two foreground pixels are adjacent under connectivity 4 (left/right, up/down) or 8 (plus the diagonals); nothing wraps at the
plane's border.  Without depth every adjacent foreground pair is an edge.  With depth, pair (a, b) is an edge iff, in float32, every
operation rounded on its own:
    zn = fminf(za, zb);  t = zn - 0.4f;  tol = max_step + depth_sigmas * (0.0012f + 0.0019f * (t * t));  fabsf(za - zb) <= tol
(depthStdDevZ at the nearer depth: symmetric).  Components are the connected components of that undirected graph; the relation is not
transitive pixel to pixel -- a ramp is one component.
Canonical names.  A component's root is its smallest linear pixel index y * w + x, its label root + 1, background 0.
Record.  (root, area, x0, y0, x1, y1, seeded): the inclusive box; seeded = 1 iff seeds is given and keeps a pixel of the component.
Filter.  Kept iff min_area <= area and (max_area < 0 or area <= max_area); and seeds is None or seeded; and keep_largest == 0 or the
component is among the first keep_largest of those that passed the two tests before, by (area descending, root ascending).
Counts.  foreground, components, kept_components, kept_pixels, largest_area (of all components), edges_cut (adjacent foreground pairs
under the connectivity that the depth rule refused, each once; 0 without depth).

numpy's float32 scalars and arrays round every operation on its own, which is the rule's arithmetic."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

F = np.float32
COUNTS = ("foreground", "components", "kept_components", "kept_pixels", "largest_area", "edges_cut")
RECORD = ("root", "area", "x0", "y0", "x1", "y1", "seeded")
RECORD_DTYPE = np.dtype([(name, np.int32) for name in RECORD])
MAX_LARGEST = 8
DEFAULTS = dict(connectivity=8, max_step=0.0, depth_sigmas=10.0, min_area=0, max_area=-1, keep_largest=0)
# (dy, dx) of the backward neighbours: every undirected pair appears once
BACKWARD = {4: ((0, -1), (-1, 0)), 8: ((0, -1), (-1, 0), (-1, -1), (-1, 1))}


def foreground(mask, depth):
    assert mask is not None or depth is not None
    fg = np.ones((mask if mask is not None else depth).shape, bool)
    if mask is not None:
        fg &= np.asarray(mask) != 0
    if depth is not None:
        fg &= np.isfinite(depth)
    return fg


def depth_edge(za, zb, max_step, depth_sigmas):
    """the edge rule on float32 arrays (or scalars) of finite depths"""
    za, zb = np.asarray(za, F), np.asarray(zb, F)
    zn = np.minimum(za, zb)
    t = zn - F(0.4)
    tol = F(max_step) + F(depth_sigmas) * (F(0.0012) + F(0.0019) * (t * t))
    return np.abs(za - zb) <= tol


def _shifted(a, dy, dx):
    """(own, neighbour) views of plane a for the neighbour at (y + dy, x + dx), dy in {-1, 0}, dx in {-1, 0, 1}"""
    h, w = a.shape
    ys = slice(-dy, h)
    yn = slice(0, h + dy)
    if dx < 0:
        xs, xn = slice(1, w), slice(0, w - 1)
    elif dx > 0:
        xs, xn = slice(0, w - 1), slice(1, w)
    else:
        xs = xn = slice(0, w)
    return a[ys, xs], a[yn, xn]


def edges(fg, depth, connectivity=8, max_step=0.0, depth_sigmas=10.0):
    """(a, b, cut): the linear indices of every edge's two ends, and the number of adjacent foreground pairs the depth rule refused"""
    assert connectivity in (4, 8)
    h, w = fg.shape
    index = np.arange(h * w).reshape(h, w)
    ea, eb, cut = [], [], 0
    for dy, dx in BACKWARD[connectivity]:
        fs, fn = _shifted(fg, dy, dx)
        pair = fs & fn
        if depth is not None:
            zs, zn = _shifted(np.where(fg, depth, F(0)).astype(F), dy, dx)
            ok = pair & depth_edge(zs, zn, max_step, depth_sigmas)
            cut += int(pair.sum()) - int(ok.sum())
            pair = ok
        i_s, i_n = _shifted(index, dy, dx)
        ea.append(i_s[pair]), eb.append(i_n[pair])
    return np.concatenate(ea), np.concatenate(eb), cut


def label(mask, depth=None, connectivity=8, max_step=0.0, depth_sigmas=10.0):
    """(labels int32 [h, w], edges_cut): root + 1 on a component's pixels, 0 on the background"""
    fg = foreground(mask, depth)
    h, w = fg.shape
    a, b, cut = edges(fg, depth, connectivity, max_step, depth_sigmas)
    graph = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(h * w, h * w))
    _, comp = connected_components(graph, directed=False)
    flat = fg.ravel()
    # the smallest pixel index of every scipy component that holds a foreground pixel
    root_of = np.full(comp.max() + 1, h * w, np.int64)
    np.minimum.at(root_of, comp[flat], np.flatnonzero(flat))
    labels = np.where(flat, root_of[comp] + 1, 0).astype(np.int32).reshape(h, w)
    return labels, cut


def records(labels, seeds=None):
    """the per-component records of a label plane, in ascending root order"""
    h, w = labels.shape
    roots = np.unique(labels[labels > 0]) - 1
    out = np.zeros(len(roots), RECORD_DTYPE)
    ys, xs = np.nonzero(labels > 0)
    which = np.searchsorted(roots, labels[ys, xs] - 1)
    out["root"] = roots
    out["area"] = np.bincount(which, minlength=len(roots))
    for name, values, fn, start in (("x0", xs, np.minimum, w), ("y0", ys, np.minimum, h), ("x1", xs, np.maximum, -1), ("y1", ys, np.maximum, -1)):
        acc = np.full(len(roots), start, np.int64)
        fn.at(acc, which, values)
        out[name] = acc
    if seeds is not None:
        hit = np.zeros(len(roots), np.int64)
        np.maximum.at(hit, which, (np.asarray(seeds)[ys, xs] != 0).astype(np.int64))
        out["seeded"] = hit
    return out


def kept_roots(recs, has_seeds, min_area=0, max_area=-1, keep_largest=0):
    assert 0 <= keep_largest <= MAX_LARGEST and min_area >= 0
    passed = [r for r in recs if min_area <= r["area"] and (max_area < 0 or r["area"] <= max_area) and (not has_seeds or r["seeded"])]
    if keep_largest:
        passed = sorted(passed, key=lambda r: (-int(r["area"]), int(r["root"])))[:keep_largest]
    return sorted(int(r["root"]) for r in passed)


def filter_components(mask, depth=None, seeds=None, connectivity=8, max_step=0.0, depth_sigmas=10.0, min_area=0, max_area=-1,
                      keep_largest=0):
    """one level: (plane uint8 of 0 / 1, counts dict)"""
    labels, cut = label(mask, depth, connectivity, max_step, depth_sigmas)
    recs = records(labels, seeds)
    keep = kept_roots(recs, seeds is not None, min_area, max_area, keep_largest)
    out = np.isin(labels, np.asarray(keep, np.int64) + 1).astype(np.uint8) if keep else np.zeros(labels.shape, np.uint8)
    counts = dict(foreground=int((labels > 0).sum()), components=len(recs), kept_components=len(keep), kept_pixels=int(out.sum()),
                  largest_area=int(recs["area"].max()) if len(recs) else 0, edges_cut=cut)
    return out, counts


def filter_levels(masks, depths=None, seeds=None, **options):
    """every level on its own: masks / depths / seeds are per-level lists (or None); min_area / max_area may be per-level lists"""
    n = len(masks if masks is not None else depths)
    planes, counts = [], []
    for l in range(n):
        opt = {k: (v[l] if k in ("min_area", "max_area") and hasattr(v, "__len__") else v) for k, v in options.items()}
        p, c = filter_components(None if masks is None else masks[l], None if depths is None else depths[l],
                                 None if seeds is None else seeds[l], **opt)
        planes.append(p), counts.append(c)
    return planes, counts


def level_areas(a0, levels):
    return [max(1, -(-int(a0) // 4 ** l)) for l in range(levels)]


def label_loop(mask, depth=None, connectivity=8, max_step=0.0, depth_sigmas=10.0):
    """label() as a plain Python pixel loop with its own union-find (small planes only): (labels, edges_cut)"""
    fg = foreground(mask, depth)
    h, w = fg.shape
    parent = list(range(h * w))

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i

    cut = 0
    for y in range(h):
        for x in range(w):
            if not fg[y, x]:
                continue
            for dy, dx in BACKWARD[connectivity]:
                yy, xx = y + dy, x + dx
                if yy < 0 or xx < 0 or xx >= w or not fg[yy, xx]:
                    continue
                if depth is not None:
                    za, zb = F(depth[y, x]), F(depth[yy, xx])
                    zn = za if za < zb else zb
                    t = F(zn - F(0.4))
                    tol = F(F(max_step) + F(F(depth_sigmas) * F(F(0.0012) + F(F(0.0019) * F(t * t)))))
                    if not abs(F(za - zb)) <= tol:
                        cut += 1
                        continue
                a, b = find(y * w + x), find(yy * w + xx)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    labels = np.zeros((h, w), np.int32)
    for y in range(h):
        for x in range(w):
            if fg[y, x]:
                labels[y, x] = find(y * w + x) + 1
    return labels, cut
