"""The mesh rule of the signed-distance volume (include/dvo_amd.h, "The mesh": naive surface nets) restated in numpy, twice:
vectorised in float32 over the active cells and the crossing edges (every numpy operation on float32 arrays rounds on its own), and
as a scalar loop over np.float32 values written independently (corners by their offsets, ranks in a dict).  The two must agree bit
for bit; dvo_amd_volume_mesh must agree with them bit for bit.  Records and options are those of tests/volume_ref.py.

Both return (xyz float32 [V, 3], rgb uint32 [V], normals float32 [V, 3], triangles int32 [T, 3], counts) with
counts = {vertices, triangles, open_edges, uncoloured, flat}."""
import numpy as np

import volume_ref as ref

F = ref.F
QUAD = ((-1, -1), (0, -1), (0, 0), (-1, 0))  # (db, dc) of q0..q3: counter-clockwise seen from +a


def _planes(rec, min_weight):
    pub = ref.public(rec)
    w_sum, sd_sum, iw_sum, i_sum = [pub[..., j] for j in range(4)]
    valid = w_sum >= min_weight
    Fv = sd_sum.astype(F) / np.where(valid, w_sum, 1).astype(F)
    col = iw_sum > 0
    Gv = i_sum.astype(F) / np.where(col, iw_sum, 1).astype(F)
    return valid, Fv, col, Gv


def _corner(a, k, nc):
    """the array of corner k = dx + 2*dy + 4*dz over all cells [ncz, ncy, ncx]"""
    dx, dy, dz = k & 1, (k >> 1) & 1, k >> 2
    return a[dz:dz + nc[2], dy:dy + nc[1], dx:dx + nc[0]]


def cells(opt, rec, min_weight=1):
    """(known, active) bool [nz-1, ny-1, nx-1]"""
    valid, Fv, _, _ = _planes(rec, min_weight)
    nc = (opt.nx - 1, opt.ny - 1, opt.nz - 1)
    known = np.ones((nc[2], nc[1], nc[0]), bool)
    n_in = np.zeros(known.shape, np.int32)
    for k in range(8):
        known &= _corner(valid, k, nc)
        n_in += _corner(Fv, k, nc) <= F(0)
    return known, known & (n_in > 0) & (n_in < 8)


def mesh(opt, rec, min_weight=1):
    """vectorised"""
    n = opt.dims
    nc = (opt.nx - 1, opt.ny - 1, opt.nz - 1)
    with np.errstate(all="ignore"):
        valid, Fv, col, Gv = _planes(rec, min_weight)
        known, active = cells(opt, rec, min_weight)
        A = np.flatnonzero(active.ravel())  # ascending Lc
        V = len(A)
        cc = [A % nc[0], (A // nc[0]) % nc[1], A // (nc[0] * nc[1])]
        Fk = [_corner(Fv, k, nc).ravel()[A] for k in range(8)]
        Ck = [_corner(col, k, nc).ravel()[A] for k in range(8)]
        Gk = [_corner(Gv, k, nc).ravel()[A] for k in range(8)]
        S = [np.zeros(V, F) for _ in range(3)]
        grad = [np.zeros(V, F) for _ in range(3)]
        gsum, m, mc = np.zeros(V, F), np.zeros(V, np.int32), np.zeros(V, np.int32)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for j in range(4):
                db, dc = j & 1, j >> 1
                lo = (db << b) | (dc << c)
                hi = lo | (1 << a)
                Fa, Fb = Fk[lo], Fk[hi]
                grad[a] = grad[a] + (Fb - Fa)
                cross = ((Fa > F(0)) & (Fb <= F(0))) | ((Fa <= F(0)) & (Fb > F(0)))
                s = Fa / (Fa - Fb)
                pt = [None] * 3
                pt[a], pt[b], pt[c] = s, np.full(V, db, F), np.full(V, dc, F)
                for t in range(3):
                    S[t] = np.where(cross, S[t] + pt[t], S[t])
                m += cross
                both = cross & Ck[lo] & Ck[hi]
                g = Gk[lo] + s * (Gk[hi] - Gk[lo])
                gsum = np.where(both, gsum + g, gsum)
                mc += both
        mf = m.astype(F)
        xyz = np.stack([opt.origin[a] + (cc[a].astype(F) + S[a] / mf) * opt.voxel for a in range(3)], axis=-1).astype(F).reshape(-1, 3)
        grey = np.minimum(np.maximum(np.rint((gsum / mc.astype(F)) * F(0.0625)), F(0.0)), F(255.0))
        grey = np.where(mc > 0, grey, 0).astype(np.uint32)
        rgb = ((grey << 16) | (grey << 8) | grey).astype(np.uint32)
        length = np.sqrt((grad[0] * grad[0] + grad[1] * grad[1]) + grad[2] * grad[2])
        flat = length == F(0)
        normals = np.stack([np.where(flat, F(0), grad[a] / length) for a in range(3)], axis=-1).astype(F).reshape(-1, 3)
        # faces: extract's candidates that cross, in ascending 3*L + a
        rank = np.cumsum(active.ravel()) - 1
        known_flat = known.ravel()
        keys, quads, ups, oks = [], [], [], []
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            ax = 2 - a
            sl_a, sl_b = [slice(None)] * 3, [slice(None)] * 3
            sl_a[ax], sl_b[ax] = slice(0, n[a] - 1), slice(1, n[a])
            sl_a, sl_b = tuple(sl_a), tuple(sl_b)
            Fa, Fb = Fv[sl_a], Fv[sl_b]
            cross = valid[sl_a] & valid[sl_b] & (((Fa > F(0)) & (Fb <= F(0))) | ((Fa <= F(0)) & (Fb > F(0))))
            iz, iy, ix = np.nonzero(cross)
            idx = [ix, iy, iz]
            ok = np.ones(len(ix), bool)
            q = np.zeros((len(ix), 4), np.int64)
            for k, (db, dc) in enumerate(QUAD):
                at = list(idx)
                at[b], at[c] = idx[b] + db, idx[c] + dc
                exists = np.ones(len(ix), bool)
                for t in range(3):
                    exists &= (at[t] >= 0) & (at[t] <= nc[t] - 1)
                Lc = np.where(exists, (at[2] * nc[1] + at[1]) * nc[0] + at[0], 0)
                ok &= exists & known_flat[Lc]
                q[:, k] = rank[Lc]
            keys.append(3 * ((iz * n[1] + iy) * n[0] + ix) + a)
            quads.append(q), ups.append(Fb[cross] > F(0)), oks.append(ok)
        keys, quads, ups, oks = np.concatenate(keys), np.concatenate(quads), np.concatenate(ups), np.concatenate(oks)
        order = np.argsort(keys, kind="stable")
        order = order[oks[order]]
        q, up = quads[order], ups[order][:, None]
        first = np.where(up, q[:, [0, 1, 2]], q[:, [0, 2, 1]])
        second = np.where(up, q[:, [0, 2, 3]], q[:, [0, 3, 2]])
        triangles = np.stack([first, second], axis=1).reshape(-1, 3).astype(np.int32)
    counts = dict(vertices=V, triangles=len(triangles), open_edges=int((~oks).sum()), uncoloured=int((mc == 0).sum()), flat=int(flat.sum()))
    return xyz, rgb, normals, triangles, counts


def mesh_scalar(opt, rec, min_weight=1):
    """the same, one cell, one edge and one operation at a time"""
    pub = ref.public(rec)
    nx, ny, nz = opt.dims
    origin, voxel = [F(v) for v in opt.origin], F(opt.voxel)
    zero = F(0.0)

    def value(ix, iy, iz):
        v = pub[iz, iy, ix]
        return None if v[0] < min_weight else F(F(v[1]) / F(v[0]))

    def crosses(Fa, Fb):
        return (Fa > 0 and Fb <= 0) or (Fa <= 0 and Fb > 0)

    # the twelve edges in the order e = 4*a + j, j = db + 2*dc: (axis, offset of the low corner)
    edges = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for dc in (0, 1):
            for db in (0, 1):
                off = [0, 0, 0]
                off[b], off[c] = db, dc
                edges.append((a, tuple(off)))
    rank, known_cells = {}, set()
    xyz, rgb, normals = [], [], []
    unc = flat = 0
    with np.errstate(all="ignore"):
        for cz in range(nz - 1):
            for cy in range(ny - 1):
                for cx in range(nx - 1):
                    corner = {(dx, dy, dz): value(cx + dx, cy + dy, cz + dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
                    if any(v is None for v in corner.values()):
                        continue
                    known_cells.add((cx, cy, cz))
                    n_inside = sum(1 for v in corner.values() if v <= 0)
                    if n_inside in (0, 8):
                        continue
                    rank[(cx, cy, cz)] = len(xyz)
                    S, G = [zero, zero, zero], [zero, zero, zero]
                    m = mc = 0
                    gsum = zero
                    for a, off in edges:
                        hi = list(off)
                        hi[a] = 1
                        Fa, Fb = corner[off], corner[tuple(hi)]
                        G[a] = F(G[a] + F(Fb - Fa))
                        if not crosses(Fa, Fb):
                            continue
                        s = F(Fa / F(Fa - Fb))
                        for t in range(3):
                            S[t] = F(S[t] + (s if t == a else F(off[t])))
                        m += 1
                        va = pub[cz + off[2], cy + off[1], cx + off[0]]
                        vb = pub[cz + hi[2], cy + hi[1], cx + hi[0]]
                        if va[2] > 0 and vb[2] > 0:
                            Ga, Gb = F(F(va[3]) / F(va[2])), F(F(vb[3]) / F(vb[2]))
                            gsum = F(gsum + F(Ga + F(s * F(Gb - Ga))))
                            mc += 1
                    cell = (cx, cy, cz)
                    xyz.append([F(origin[t] + F(F(F(cell[t]) + F(S[t] / F(m))) * voxel)) for t in range(3)])
                    if mc > 0:
                        grey = int(min(max(np.rint(F(F(gsum / F(mc)) * F(0.0625))), F(0.0)), F(255.0)))
                        rgb.append((grey << 16) | (grey << 8) | grey)
                    else:
                        rgb.append(0)
                        unc += 1
                    length = np.sqrt(F(F(F(G[0] * G[0]) + F(G[1] * G[1])) + F(G[2] * G[2])))
                    if length == 0:
                        normals.append([zero, zero, zero])
                        flat += 1
                    else:
                        normals.append([F(G[t] / length) for t in range(3)])
        triangles, n_open = [], 0
        for iz in range(nz):
            for iy in range(ny):
                for ix in range(nx):
                    Fa = value(ix, iy, iz)
                    if Fa is None:
                        continue
                    at = (ix, iy, iz)
                    for a in range(3):
                        if at[a] + 1 >= opt.dims[a]:
                            continue
                        Fb = value(ix + (a == 0), iy + (a == 1), iz + (a == 2))
                        if Fb is None or not crosses(Fa, Fb):
                            continue
                        b, c = (a + 1) % 3, (a + 2) % 3
                        q = []
                        for db, dc in QUAD:
                            cell = list(at)
                            cell[b] += db
                            cell[c] += dc
                            if tuple(cell) in known_cells:
                                q.append(rank[tuple(cell)])  # (a known cell around a crossing edge is active)
                        if len(q) < 4:
                            n_open += 1
                        elif Fb > 0:
                            triangles += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
                        else:
                            triangles += [[q[0], q[2], q[1]], [q[0], q[3], q[2]]]
    counts = dict(vertices=len(xyz), triangles=len(triangles), open_edges=n_open, uncoloured=unc, flat=flat)
    return (np.asarray(xyz, F).reshape(-1, 3), np.asarray(rgb, np.uint32), np.asarray(normals, F).reshape(-1, 3),
            np.asarray(triangles, np.int32).reshape(-1, 3), counts)
