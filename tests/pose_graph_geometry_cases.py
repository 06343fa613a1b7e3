"""The edge geometry of the pose-graph kernels (dvo_slam_amd/csrc/dvo_graph_device.h) restated with mpmath at 60 digits, and the
seeded family of one-edge cases tests/test_pose_graph_geometry.py runs through the kernels.

The reference restates include/dvo_amd.h's wording: inverse and compose of isometries, Eigen's Shepperd Quaternion(Matrix3)
with its branch rule, the normalisation and the w >= 0 sign, e = (t, q_xyz), chi2 = e^T Omega e, the Cauchy rho0 / rho1 (and
the delta <= 0 form), J_from / J_to, the products Aff, Att, Aft, g_from, g_to, inc(d) with its identity rule and one Levenberg
trial.  It takes the float64 inputs the device gets as exact rationals and does not re-orthonormalise anything: the operation
under test is the formula applied to the given doubles.

A case's class is the branch of quaternion() its Delta = Z^-1 X_from^-1 X_to takes: "tr>0", or the largest diagonal i and the
sign of w before the normalisation ("i0+", "i0-", ... "i2-").  MARGIN_CLASS is how far the reference's deciding quantities must
be from their thresholds for the class to count (the device, 1e-16 from the reference, then cannot land elsewhere by rounding).
"""
from __future__ import annotations

import functools
import os
import sys

import mpmath
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_graph_restatement as R  # noqa: E402

mp = mpmath.mp.clone()
mp.dps = 60
F = mp.mpf
ZERO, ONE, HALF, TWO = F(0), F(1), F(1) / 2, F(2)

CLASSES = ("tr>0", "i0+", "i0-", "i1+", "i1-", "i2+", "i2-")
MARGIN_CLASS = 1e-9
DELTAS = (5.0, 0.5, 0.0)
LAMBDA = 1e-3      # initial_lambda of the one Levenberg trial
BAR = 1e-12        # block-relative bar on H and b, relative bar on F (tests/test_pose_graph.py)


# ---- small dense algebra on lists of mpf ------------------------------------------------------------------------------------------
def _mat(a):
    return [[F(float(x)) for x in row] for row in np.asarray(a, dtype=np.float64)]


def _T(A):
    return [list(r) for r in zip(*A)]


def _mm(A, B):
    Bt = _T(B)
    return [[mp.fdot(r, c) for c in Bt] for r in A]


def _mv(A, v):
    return [mp.fdot(r, v) for r in A]


def _skew(a):
    return [[ZERO, -a[2], a[1]], [a[2], ZERO, -a[0]], [-a[1], a[0], ZERO]]


def _scale(A, s):
    return [[s * x for x in r] for r in A]


def _add(A, B):
    return [[x + y for x, y in zip(r, q)] for r, q in zip(A, B)]


def _np(A):
    return np.array([[float(x) for x in r] for r in A]) if isinstance(A[0], list) else np.array([float(x) for x in A])


def solve(A, b):
    """A x = b by Gaussian elimination with partial pivoting"""
    n = len(b)
    M = [list(A[r]) + [b[r]] for r in range(n)]
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(M[r][c]))
        M[c], M[p] = M[p], M[c]
        for r in range(c + 1, n):
            f = M[r][c] / M[c][c]
            for k in range(c, n + 1):
                M[r][k] -= f * M[c][k]
    x = [ZERO] * n
    for r in range(n - 1, -1, -1):
        x[r] = (M[r][n] - mp.fdot(M[r][r + 1:n], x[r + 1:])) / M[r][r]
    return x


# ---- SE3 ----------------------------------------------------------------------------------------------------------------------
def pose(T):
    """(R, t) of a float64 4x4, exactly"""
    T = np.asarray(T, dtype=np.float64)
    return _mat(T[:3, :3]), [F(float(x)) for x in T[:3, 3]]


def pose_np(P):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _np(P[0]), _np(P[1])
    return T


def inverse(P):
    Rt = _T(P[0])
    return Rt, [-x for x in _mv(Rt, P[1])]


def compose(A, B):
    return _mm(A[0], B[0]), [x + y for x, y in zip(_mv(A[0], B[1]), A[1])]


def quaternion(m):
    """Eigen's Quaternion(Matrix3) (Shepperd), normalised, w >= 0: ((w, x, y, z), class, margin).  margin: the least distance
    of a deciding quantity from its threshold -- the trace from 0; below it the winning diagonal from the other two and the
    raw w from 0."""
    tr = m[0][0] + m[1][1] + m[2][2]
    v = [ZERO] * 3
    if tr > 0:
        t = mp.sqrt(tr + 1)
        w = HALF * t
        t = HALF / t
        v = [(m[2][1] - m[1][2]) * t, (m[0][2] - m[2][0]) * t, (m[1][0] - m[0][1]) * t]
        cls, margin = "tr>0", tr
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = mp.sqrt(m[i][i] - m[j][j] - m[k][k] + 1)
        v[i] = HALF * t
        t = HALF / t
        w = (m[k][j] - m[j][k]) * t
        v[j] = (m[j][i] + m[i][j]) * t
        v[k] = (m[k][i] + m[i][k]) * t
        cls = "i%d%s" % (i, "+" if w >= 0 else "-")
        margin = min(-tr, m[i][i] - m[j][j], m[i][i] - m[k][k], abs(w))
    s = 1 / mp.sqrt(w * w + v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if w < 0:
        s = -s
    return [w * s, v[0] * s, v[1] * s, v[2] * s], cls, margin, abs(w)


def inc(d):
    """(pose, 1 - |d_rot|^2): translation d[:3], rotation of (sqrt(1 - |d_rot|^2), d_rot), the identity when that is < 0"""
    x, y, z = d[3], d[4], d[5]
    w2 = 1 - (x * x + y * y + z * z)
    if w2 < 0:
        Rm = [[ONE, ZERO, ZERO], [ZERO, ONE, ZERO], [ZERO, ZERO, ONE]]
    else:
        w = mp.sqrt(w2)
        Rm = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
              [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
              [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return (Rm, [d[0], d[1], d[2]]), w2


def robust(chi2, delta):
    if delta > 0:
        dsqr = F(float(delta)) * F(float(delta))
        aux = chi2 / dsqr + 1
        return dsqr * mp.log(aux), 1 / aux
    return chi2, ONE


def error(Xf, Xt, Z, O):
    """(Delta, q, e, chi2, class, margin, |raw w|) of one edge; the poses are (R, t) of mpf, O a 6x6 of mpf"""
    D = compose(inverse(Z), compose(inverse(Xf), Xt))
    q, cls, margin, w_raw = quaternion(D[0])
    e = list(D[1]) + q[1:]
    return D, q, e, mp.fdot(e, _mv(O, e)), cls, margin, w_raw


def edge(Xf, Xt, Z, O):
    """One edge without its kernel weight: dict(e, chi2, cls, margin, w_raw, Jf, Jt, and the products with Omega alone
    Pff = Jf^T O Jf, Ptt, Pft, hf = -Jf^T O e, ht; Aff = rho1 Pff and so on)"""
    Xf, Xt, Z, O = pose(Xf), pose(Xt), pose(Z), _mat(O)
    D, q, e, chi2, cls, margin, w_raw = error(Xf, Xt, Z, O)
    w, v = q[0], q[1:]
    Rm, t = D
    RzT, tz = _T(Z[0]), Z[1]
    wI = [[w if r == c else ZERO for c in range(3)] for r in range(3)]
    z3 = [[ZERO] * 3 for _ in range(3)]
    br = _add(wI, _skew(v))                                                   # w I + [v]x
    Jt = [Rm[r] + z3[r] for r in range(3)] + [z3[r] + br[r] for r in range(3)]
    tr_ = _scale(_add(_mm(_skew(t), RzT), _mm(RzT, _skew(tz))), TWO)           # 2 ([t]x Rz^T + Rz^T [tz]x)
    bf = _scale(_mm(_add(wI, _scale(_skew(v), -ONE)), RzT), -ONE)              # -(w I - [v]x) Rz^T
    Jf = [[-x for x in RzT[r]] + tr_[r] for r in range(3)] + [z3[r] + bf[r] for r in range(3)]
    OJf, OJt, Oe = _mm(O, Jf), _mm(O, Jt), _mv(O, e)
    JfT, JtT = _T(Jf), _T(Jt)
    return dict(e=e, chi2=chi2, cls=cls, margin=margin, w_raw=w_raw, Jf=Jf, Jt=Jt, Pff=_mm(JfT, OJf), Ptt=_mm(JtT, OJt),
                Pft=_mm(JfT, OJt), hf=[-x for x in _mv(JfT, Oe)], ht=[-x for x in _mv(JtT, Oe)])


def step(case, delta, moved, lam=LAMBDA):
    """One Levenberg trial (dvo_amd.h) of the two-vertex graph of `case` with the other vertex fixed: moved = "to" or "from".
    dict(F0, x, w2 = 1 - |x_rot|^2, rho the gain ratio, accepted, gain = sum x_i (lambda x_i + b_i), pose the moved vertex
    after the step (float64), Fp, chi2 / rho1 at that pose)"""
    ref = case["ref"]
    rho0, rho1 = robust(ref["chi2"], delta)
    P, h = (ref["Ptt"], ref["ht"]) if moved == "to" else (ref["Pff"], ref["hf"])
    lam = F(float(lam))
    b = [rho1 * x for x in h]
    A = [[rho1 * P[r][c] + (lam if r == c else ZERO) for c in range(6)] for r in range(6)]
    x = solve(A, b)
    D, w2 = inc(x)
    Xf, Xt, Z, O = pose(case["Xf"]), pose(case["Xt"]), pose(case["Z"]), _mat(case["O"])
    if moved == "to":
        Xt = compose(Xt, D)
    else:
        Xf = compose(Xf, D)
    chi2p = error(Xf, Xt, Z, O)[3]
    Fp, r1p = robust(chi2p, delta)
    rho = (rho0 - Fp) / (F("1e-3") + sum(xi * (lam * xi + bi) for xi, bi in zip(x, b)))
    gain = sum(xi * (lam * xi + bi) for xi, bi in zip(x, b))
    return dict(F0=float(rho0), x=_np(x), w2=float(w2), rho=float(rho), accepted=bool(rho > 0), gain=float(gain),
                pose=pose_np(Xt if moved == "to" else Xf), Fp=float(Fp), chi2=float(chi2p), rho1=float(r1p))


def blocks(case, delta):
    """float64 (Aff, Att, Aft, g_from, g_to, rho0, rho1) of the case under the Cauchy kernel of `delta`, each the reference's
    value rounded once"""
    ref = case["ref"]
    rho0, rho1 = robust(ref["chi2"], delta)
    out = [_np(_scale(ref[k], rho1)) for k in ("Pff", "Ptt", "Pft")] + [_np([rho1 * x for x in ref[k]]) for k in ("hf", "ht")]
    return tuple(out) + (float(rho0), float(rho1))


# ---- the same in float64: the restatement ---------------------------------------------------------------------------------------
def restatement_blocks(case, delta):
    Xf, Xt, Z, O = case["Xf"], case["Xt"], case["Z"], case["O"]
    e = R.edge_error(Xf, Xt, Z)
    Jf, Jt = R.jacobians(Xf, Xt, Z)
    chi2 = float(e @ (O @ e))
    rho0, rho1 = R.robust(chi2, delta)
    W = float(rho1) * O
    return Jf.T @ W @ Jf, Jt.T @ W @ Jt, Jf.T @ W @ Jt, -Jf.T @ (W @ e), -Jt.T @ (W @ e), float(rho0), float(rho1)


def rel(a, b):
    """max|a - b| / max|b| of one block (0 / 0 = 0, a difference on a zero block = inf): tests/test_pose_graph.py::_block_rel"""
    d, s = float(np.max(np.abs(a - b))), float(np.max(np.abs(b)))
    return 0.0 if d == 0 else (d / s if s > 0 else np.inf)


def block_rel(A, B, bs=6):
    """_block_rel of tests/test_pose_graph.py, vectorised: the worst block-relative deviation of A from B"""
    if A.ndim == 1:
        a, b = A.reshape(-1, bs), B.reshape(-1, bs)
        d, s = np.max(np.abs(a - b), axis=1), np.max(np.abs(b), axis=1)
    else:
        n, m = A.shape[0] // bs, A.shape[1] // bs
        d = np.max(np.abs(A - B).reshape(n, bs, m, bs), axis=(1, 3))
        s = np.max(np.abs(B).reshape(n, bs, m, bs), axis=(1, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, np.where(s > 0, d / s, np.inf))
    return float(np.max(r)) if r.size else 0.0


# ---- the case family ------------------------------------------------------------------------------------------------------------
def _exp(xi):
    from dvo_slam_amd import synth

    return synth.se3_exp(xi)


def _omega(rng, kind):
    if kind == 0:
        return R.information(rng)
    if kind == 1:
        return np.diag(np.r_[rng.uniform(100.0, 1000.0, size=3), rng.uniform(1000.0, 5000.0, size=3)])
    # strong translation-rotation cross terms: [[400 I, 900 Q], [900 Q^T, 2500 I]] with Q a rotation has the eigenvalues
    # (2900 +- sqrt(2100^2 + 4 * 900^2)) / 2 = 2833 and 67: positive definite, condition number 42
    Q = _exp(np.r_[0.0, 0.0, 0.0, rng.normal(size=3)])[:3, :3]
    O = np.zeros((6, 6))
    O[:3, :3], O[3:, 3:], O[:3, 3:], O[3:, :3] = 400.0 * np.eye(3), 2500.0 * np.eye(3), 900.0 * Q, 900.0 * Q.T
    return 0.5 * (O + O.T)


_QUARTER_TURNS = [np.array(m, dtype=np.float64) for m in (
    [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[0, 0, 1], [1, 0, 0], [0, 1, 0]], [[-1, 0, 0], [0, 0, 1], [0, 1, 0]],
    [[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, 0, 1], [0, -1, 0], [1, 0, 0]], [[0, 1, 0], [0, 0, 1], [1, 0, 0]])]


def _exact_pose(rng, k):
    """a pose far from the identity whose products round nowhere: a signed permutation as rotation, a translation of
    multiples of 2^-8 below 4"""
    T = np.eye(4)
    T[:3, :3] = _QUARTER_TURNS[k % len(_QUARTER_TURNS)]
    T[:3, 3] = rng.integers(-1000, 1000, size=3) / 256.0
    return T


def _axes(rng):
    out = [np.array(a, dtype=np.float64) for a in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                out.append(np.array([sx, sy, sz]) / np.sqrt(3.0))
    for _ in range(2):
        a = rng.normal(size=3)
        out.append(a / np.linalg.norm(a))
    return out


GRID_ANGLES = (0.0, 1e-8, 1e-3, np.pi / 2 - 1e-6, np.pi / 2 + 1e-6, 2 * np.pi / 3 - 1e-6, 2 * np.pi / 3 + 1e-6, np.pi - 1e-3)


def generate(seed=20):
    """The raw cases, before the reference looks at them: dicts of Xf, Xt, Z (4x4 row-major), O (6x6), angle, origin"""
    rng = np.random.default_rng(seed)
    raw = []

    def add(angle, axis, origin, short=False):
        k = len(raw)
        if angle == 0.0:  # exactly consistent: Delta is the identity in exact arithmetic too, e = 0 and chi2 = 0
            Xf, Z = _exact_pose(rng, k), _exact_pose(rng, k + 1)
            Xt = Xf @ Z
        else:
            Xf = _exp(np.r_[rng.uniform(-3.0, 3.0, size=3), rng.normal(size=3)])
            # short: a measurement with a short lever arm, so that a step of the from-vertex whose rotation inc() drops
            # (the identity rule) still lowers F through its translation and is kept
            Z = _exp(np.r_[(0.02 if short else 0.5) * rng.normal(size=3), 0.5 * rng.normal(size=3)])
            Xt = Xf @ Z @ _exp(np.r_[0.3 * rng.normal(size=3), axis * angle])
        raw.append(dict(Xf=Xf, Xt=Xt, Z=Z, O=_omega(rng, k % 3), angle=float(angle), origin=origin))

    def random_axis():
        a = rng.normal(size=3)
        return a / np.linalg.norm(a)

    for _ in range(90):      # any rotation error
        add(rng.uniform(0.05, np.pi - 1e-3), random_axis(), "random")
    for k in range(110):     # beyond 120 degrees, where the trace is negative
        add(rng.uniform(2.1, np.pi - 1e-3), random_axis(), "random, trace < 0", short=k % 2 == 1)
    for axis in _axes(rng):
        for angle in GRID_ANGLES:
            add(angle, axis, "grid")
    return raw


@functools.lru_cache(maxsize=None)
def family():
    """dict(cases, dropped, generated).  Every kept case carries `ref` (edge()), `cls`, and `strict`: its class counts (the
    deciding quantities are MARGIN_CLASS from their thresholds); the others are the near-tie group, compared only on what is
    continuous across the tie.  Dropped: |raw w| < MARGIN_CLASS below the trace threshold (the sign of e_q is undetermined),
    and the cases whose honest float64 error exceeds the bar -- the float64 restatement of the same formula misses BAR on
    them -- with the reason."""
    cases, dropped = [], []
    raw = generate()
    for c in raw:
        ref = edge(c["Xf"], c["Xt"], c["Z"], c["O"])
        c.update(ref=ref, cls=ref["cls"])
        if ref["cls"] != "tr>0" and float(ref["w_raw"]) < MARGIN_CLASS:
            dropped.append((c, "w within the margin of 0"))
            continue
        worst = 0.0
        for delta in DELTAS:
            a, b = restatement_blocks(c, delta), blocks(c, delta)
            worst = max([worst] + [rel(x, y) for x, y in zip(a[:5], b[:5])])
        c["restatement_rel"] = worst
        if worst > BAR:
            dropped.append((c, "float64 error of the formula itself: %.2e block-relative" % worst))
            continue
        c["strict"] = bool(float(ref["margin"]) >= MARGIN_CLASS)
        cases.append(c)
    return dict(cases=cases, dropped=dropped, generated=len(raw))


def census(cases):
    return {k: sum(1 for c in cases if c["strict"] and c["cls"] == k) for k in CLASSES}


@functools.lru_cache(maxsize=None)
def steps(delta, moved):
    """step() of every case of the family, in order"""
    return [step(c, delta, moved) for c in family()["cases"]]


# ---- the rotated loop closures of the multi-iteration run ------------------------------------------------------------------------
def flipped_loop_graph(m, planted=True, seed=17):
    """R.ring_graph(m, n_chords=6, noise=1e-3) and, with planted, three more loop edges at the end whose measurement is the
    true relative pose composed with a rotation of pi - 0.05 about x, y and z and a 0.5 m offset.  Returns (Graph, truth)."""
    g, truth = R.ring_graph(m, n_chords=6, seed=seed, noise=1e-3)
    edges = list(g.edges)
    if planted:
        rng = np.random.default_rng(seed + 1)
        for a, (f, t) in enumerate(((2, m // 2), (m // 4, m - 3), (m // 3, m - 8))):
            axis = np.eye(3)[a] * (np.pi - 0.05)
            offset = np.roll([0.5, 0.0, 0.0], a)
            Z = R.inverse(truth[f]) @ truth[t] @ _exp(np.r_[offset, axis])
            edges.append((f, t, Z, R.information(rng)))
    return R.Graph(g.poses, g.fixed, edges), truth
