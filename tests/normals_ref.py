"""The surface-normal rule of include/dvo_amd.h ("Surface normals") restated in numpy, operation by operation in fp32:
normals_ref is vectorised over the plane, normals_loop is the same rule as a plain pixel loop.  Both return
(normals float32 [h, w, 4], facing float32 [h, w], (defined, undefined)); every NaN they leave is the one quiet NaN 0x7FC00000."""
import numpy as np

F = np.float32
NAN = F(np.nan)
FACING_AXIS, FACING_RAY = 0, 1
MAX_RADIUS = 8
TINY = F(1e-30)


def rays(w, h, K):
    fx, fy, ox, oy = [F(k) for k in K]
    return (np.arange(w, dtype=F) - ox) / fx, (np.arange(h, dtype=F) - oy) / fy


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def normals_ref(Z, K, radius=0, ratio=0.0, facing=FACING_AXIS, toward_camera=0):
    Z = np.ascontiguousarray(Z, dtype=F)
    h, w = Z.shape
    r, ratio = int(radius), F(ratio)
    tx, ty = rays(w, h, K)
    with np.errstate(all="ignore"):
        P = (tx[None, :] * Z, ty[:, None] * Z, Z)
        up, um = np.minimum(np.arange(w) + 1, w - 1), np.maximum(np.arange(w) - 1, 0)
        vp, vm = np.minimum(np.arange(h) + 1, h - 1), np.maximum(np.arange(h) - 1, 0)
        a = [p[:, up] - p[:, um] for p in P]
        b = [p[vp, :] - p[vm, :] for p in P]
        c = _cross(a, b)
        usable = np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2])
        # the members of every pixel's window, dv outer, du inner: the planes shifted under the pixel
        pad = lambda A, fill: np.pad(A, r, constant_values=fill)  # noqa: E731
        cp, up_, zp = [pad(x, F(0)) for x in c], pad(usable, False), pad(Z, NAN)
        centre = np.isfinite(Z)
        have = np.zeros((h, w), bool)
        m = [np.zeros((h, w), F) for _ in range(3)]
        for dv in range(-r, r + 1):
            for du in range(-r, r + 1):
                win = (slice(r + dv, r + dv + h), slice(r + du, r + du + w))
                add = centre & up_[win]
                if ratio > 0:
                    add &= np.abs(zp[win] - Z) <= ratio * Z
                for k in range(3):
                    m[k] = np.where(add, np.where(have, m[k] + cp[k][win], cp[k][win]), m[k])
                have |= add
        s = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        defined = have & (s >= TINY)
        length = np.sqrt(s)
        n = [x / length for x in m]
        d = (n[0] * P[0] + n[1] * P[1]) + n[2] * P[2]
        if toward_camera:
            flip = d > 0
            n = [np.where(flip, -x, x) for x in n]
        if facing == FACING_AXIS:
            f = np.abs(n[2])
        else:
            pp = (P[0] * P[0] + P[1] * P[1]) + P[2] * P[2]
            f = np.where(pp > 0, np.abs(d) / np.sqrt(pp), NAN)
        f = np.where(defined & ~np.isnan(f), f, NAN).astype(F)
        N = np.stack([np.where(defined, x, NAN) for x in n] + [np.where(defined, F(0), NAN)], axis=-1).astype(F)
    return N, f, (int(defined.sum()), int((~defined).sum()))


def normals_loop(Z, K, radius=0, ratio=0.0, facing=FACING_AXIS, toward_camera=0):
    Z = np.ascontiguousarray(Z, dtype=F)
    h, w = Z.shape
    r, ratio = int(radius), F(ratio)
    tx, ty = rays(w, h, K)
    N, f = np.full((h, w, 4), NAN, F), np.full((h, w), NAN, F)

    def point(u, v):
        return (tx[u] * Z[v, u], ty[v] * Z[v, u], Z[v, u])

    def raw(u, v):
        p1, p0 = point(min(u + 1, w - 1), v), point(max(u - 1, 0), v)
        q1, q0 = point(u, min(v + 1, h - 1)), point(u, max(v - 1, 0))
        return _cross([p1[k] - p0[k] for k in range(3)], [q1[k] - q0[k] for k in range(3)])

    n_defined = 0
    with np.errstate(all="ignore"):
        for v in range(h):
            for u in range(w):
                z = Z[v, u]
                if not np.isfinite(z):
                    continue
                m = None
                for dv in range(-r, r + 1):
                    for du in range(-r, r + 1):
                        x, y = u + du, v + dv
                        if not (0 <= x < w and 0 <= y < h):
                            continue
                        c = raw(x, y)
                        if not all(np.isfinite(k) for k in c):
                            continue
                        if ratio > 0 and not (np.abs(Z[y, x] - z) <= ratio * z):
                            continue
                        m = c if m is None else tuple(m[k] + c[k] for k in range(3))
                if m is None:
                    continue
                s = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
                if not (s >= TINY):
                    continue
                length = np.sqrt(s)
                n = [m[k] / length for k in range(3)]
                P = point(u, v)
                d = (n[0] * P[0] + n[1] * P[1]) + n[2] * P[2]
                if toward_camera and d > 0:
                    n = [-k for k in n]
                if facing == FACING_AXIS:
                    val = np.abs(n[2])
                else:
                    pp = (P[0] * P[0] + P[1] * P[1]) + P[2] * P[2]
                    val = np.abs(d) / np.sqrt(pp) if pp > 0 else NAN
                N[v, u] = n + [F(0)]
                f[v, u] = NAN if np.isnan(val) else val
                n_defined += 1
    return N, f, (n_defined, w * h - n_defined)


def rotate_ref(N, pose=None):
    """the cloud's normals: every defined normal through R = (float)pose's rotation in the pinned order, the fourth component
    carried over; pose: 4x4 row-major (numpy), None = identity -- applied the same way"""
    R = (np.eye(4) if pose is None else np.asarray(pose, dtype=np.float64)).astype(F)
    defined = ~np.isnan(N[..., 3])
    out = np.empty_like(N)
    with np.errstate(all="ignore"):
        for k in range(3):
            out[..., k] = np.where(defined, (R[k, 0] * N[..., 0] + R[k, 1] * N[..., 1]) + R[k, 2] * N[..., 2], NAN)
    out[..., 3] = N[..., 3]
    return out


def mask_ref(Z, K, min_facing, undefined_keep=0, **opt):
    """one level of dvo_amd_mask_from_normals: (bytes [h, w], (defined, undefined, kept))"""
    N, f, (n_def, n_und) = normals_ref(Z, K, **opt)
    defined = ~np.isnan(N[..., 3])
    with np.errstate(invalid="ignore"):
        keep = np.where(defined, f >= F(min_facing), bool(undefined_keep))
    return keep.astype(np.uint8), (n_def, n_und, int(keep.sum()))


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- the room corner of dvo_slam_amd.synth seen from the origin: which plane a pixel shows, and that plane's normal ----------------

PLANE_NORMALS = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])  # floor y = 1.2, wall z = 3, wall x = -1.6


def corner_planes(w, h, K):
    """the plane index [h, w] synth.render(w, h) shows at the identity pose (its own ray casting, in float64)"""
    fx, fy, ox, oy = [float(k) for k in K]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dx, dy = (u - ox) / fx, (v - oy) / fy
    big = 1e30
    with np.errstate(divide="ignore"):
        t_floor = np.where(dy > 1e-9, 1.2 / dy, big)
        t_wz = np.full_like(t_floor, 3.0)
        t_wx = np.where(dx < -1e-9, -1.6 / dx, big)
    t = np.minimum(np.minimum(t_floor, t_wz), t_wx)
    return np.where(t == t_floor, 0, np.where(t == t_wz, 1, 2))


def erode(m, k):
    """true where the (2k+1)^2 square around a pixel lies inside the plane and is true everywhere"""
    h, w = m.shape
    p = np.pad(m, k, constant_values=False)
    out = np.ones_like(m)
    for dv in range(2 * k + 1):
        for du in range(2 * k + 1):
            out &= p[dv:dv + h, du:du + w]
    return out


def interior(Z, which):
    """the pixels whose one-pixel stencil (the pixel and its four neighbours, none clamped) has depth everywhere and stays on
    one plane: where the r = 0 rule sees a plane and nothing else"""
    def stencil(m):
        o = m.copy()
        o[1:] &= m[:-1]
        o[:-1] &= m[1:]
        o[:, 1:] &= m[:, :-1]
        o[:, :-1] &= m[:, 1:]
        o[0] = o[-1] = False
        o[:, 0] = o[:, -1] = False
        return o

    return stencil(np.isfinite(Z)) & (stencil(which == 0) | stencil(which == 1) | stencil(which == 2))


def angle_deg(N, which):
    """the angle in degrees [h, w] between a normal plane and the planes' analytic normals, sign ignored, in float64 by atan2 of
    the cross and dot products (an arccos would round every angle below 0.02 degrees to 0)"""
    n, t = N[..., :3].astype(np.float64), PLANE_NORMALS[which]
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(n, t), axis=-1), np.abs((n * t).sum(-1))))
