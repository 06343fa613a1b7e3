"""Float64 numpy restatement of the pose-graph semantics pinned in include/dvo_amd.h (dvo_amd_optimize_graph): the increment,
the EdgeSE3 error and its analytic Jacobians, the Cauchy kernel, the normal equations, and the Levenberg-Marquardt and dogleg
drivers as g2o's OptimizationAlgorithmLevenberg / OptimizationAlgorithmDogleg run them.  Poses are row-major 4x4.

`optimize(..., follow=records)` adjudicates decisions: a gain ratio within `margin` of a threshold (0 for acceptance, 0.25 /
0.75 for the dogleg trust region) is a coin toss between two fp64 implementations that sum in different orders, so there the
restatement takes the decision the given records (the library's) made and logs the trial in `result["adjudicated"]`.
"""
from __future__ import annotations

import numpy as np


# ---- SE3 helpers ----------------------------------------------------------------------------------------------------------
def skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def inverse(T):
    R, t = T[:3, :3], T[:3, 3]
    o = np.eye(4)
    o[:3, :3] = R.T
    o[:3, 3] = -R.T @ t
    return o


def quaternion(m):
    """Eigen's Quaternion(Matrix3), normalised, sign with w >= 0: (w, x, y, z)"""
    tr = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
    if tr > 0.0:
        t = np.sqrt(tr + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1:] = [(m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t]
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[k, j] - m[j, k]) * t
        q[1 + j] = (m[j, i] + m[i, j]) * t
        q[1 + k] = (m[k, i] + m[i, k]) * t
    q = q / np.sqrt(np.sum(q * q))
    return -q if q[0] < 0 else q


def rotation_of(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def inc(d):
    """fromVectorMQT: translation d[:3], rotation of (sqrt(1 - |d[3:]|^2), d[3:]); identity when 1 - |q|^2 < 0"""
    d = np.asarray(d, dtype=np.float64)
    T = np.eye(4)
    w2 = 1.0 - float(d[3:] @ d[3:])
    if w2 >= 0.0:
        T[:3, :3] = rotation_of([np.sqrt(w2), d[3], d[4], d[5]])
    T[:3, 3] = d[:3]
    return T


def to_vector_mqt(T):
    q = quaternion(T[:3, :3])
    return np.r_[T[:3, 3], q[1:]]


# ---- edges ----------------------------------------------------------------------------------------------------------------
def edge_delta(Xf, Xt, Z):
    return inverse(Z) @ (inverse(Xf) @ Xt)


def edge_error(Xf, Xt, Z):
    return to_vector_mqt(edge_delta(Xf, Xt, Z))


def jacobians(Xf, Xt, Z):
    """(J_from, J_to), the closed forms of dvo_amd.h"""
    D = edge_delta(Xf, Xt, Z)
    R, t = D[:3, :3], D[:3, 3]
    q = quaternion(R)
    w, v = q[0], q[1:]
    RzT, tz = Z[:3, :3].T, Z[:3, 3]
    Jt = np.zeros((6, 6))
    Jt[:3, :3] = R
    Jt[3:, 3:] = w * np.eye(3) + skew(v)
    Jf = np.zeros((6, 6))
    Jf[:3, :3] = -RzT
    Jf[:3, 3:] = 2.0 * (skew(t) @ RzT + RzT @ skew(tz))
    Jf[3:, 3:] = -(w * np.eye(3) - skew(v)) @ RzT
    return Jf, Jt


def numeric_jacobians(Xf, Xt, Z, h=1e-6):
    Jf, Jt = np.zeros((6, 6)), np.zeros((6, 6))
    for c in range(6):
        d = np.zeros(6)
        d[c] = h
        Jf[:, c] = (edge_error(Xf @ inc(d), Xt, Z) - edge_error(Xf @ inc(-d), Xt, Z)) / (2 * h)
        Jt[:, c] = (edge_error(Xf, Xt @ inc(d), Z) - edge_error(Xf, Xt @ inc(-d), Z)) / (2 * h)
    return Jf, Jt


def robust(chi2, delta):
    chi2 = np.asarray(chi2, dtype=np.float64)
    if delta > 0:
        dsqr = delta * delta
        aux = (1.0 / dsqr) * chi2 + 1.0
        return dsqr * np.log(aux), 1.0 / aux
    return chi2.copy(), np.ones_like(chi2)


# ---- the graph --------------------------------------------------------------------------------------------------------------
class Graph:
    """poses: list of 4x4; fixed: list of bool; edges: list of (from, to, Z, Omega)"""

    def __init__(self, poses, fixed, edges):
        self.poses = [np.array(P, dtype=np.float64) for P in poses]
        self.fixed = list(fixed)
        self.edges = edges
        active = set()
        for f, t, _, _ in edges:
            active.update((f, t))
        self.free = [v for v in range(len(poses)) if v in active and not self.fixed[v]]
        self.slot = {v: s for s, v in enumerate(self.free)}

    def copy_poses(self):
        return [P.copy() for P in self.poses]


def edge_terms(poses, edges, delta):
    chi2 = np.empty(len(edges))
    for k, (f, t, Z, O) in enumerate(edges):
        e = edge_error(poses[f], poses[t], Z)
        chi2[k] = e @ (O @ e)
    rho0, rho1 = robust(chi2, delta)
    return chi2, rho0, rho1


def objective(poses, edges, delta):
    return float(np.sum(edge_terms(poses, edges, delta)[1]))


def linearise(g: Graph, delta, poses=None):
    """(H full n x n, b, F, chi2, rho1)"""
    poses = g.poses if poses is None else poses
    n = 6 * len(g.free)
    H, b = np.zeros((n, n)), np.zeros(n)
    chi2, rho0, rho1 = edge_terms(poses, g.edges, delta)
    for k, (f, t, Z, O) in enumerate(g.edges):
        e = edge_error(poses[f], poses[t], Z)
        Jf, Jt = jacobians(poses[f], poses[t], Z)
        W = rho1[k] * O
        blocks = [(g.slot.get(f), Jf), (g.slot.get(t), Jt)]
        for si, Ji in blocks:
            if si is None:
                continue
            b[6 * si:6 * si + 6] -= Ji.T @ (W @ e)
            for sj, Jj in blocks:
                if sj is None:
                    continue
                H[6 * si:6 * si + 6, 6 * sj:6 * sj + 6] += Ji.T @ W @ Jj
    return H, b, float(np.sum(rho0)), chi2, rho1


def apply(g: Graph, poses, x):
    out = [P.copy() for P in poses]
    for s, v in enumerate(g.free):
        out[v] = poses[v] @ inc(x[6 * s:6 * s + 6])
    return out


def cholesky_solve(A, b):
    """(x, ok): a pivot <= 0 (LAPACK potrf's failure) is a failed solve"""
    try:
        Lc = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None, False
    y = np.linalg.solve(Lc, b)
    return np.linalg.solve(Lc.T, y), True


class _Follow:
    """the library's decisions per (iteration, trial), from its records: trials - 1 rejections, then `accepted`"""

    def __init__(self, records, margin):
        self.r, self.margin = records, margin

    def decide(self, it, trial, rho, thresholds):
        near = min(abs(rho - th) for th in thresholds)
        if self.r is None or not (near < self.margin) or it >= len(self.r["trials"]):
            return None
        last = trial == int(self.r["trials"][it]) - 1
        return bool(last and self.r["accepted"][it])


def optimize(g: Graph, algorithm="dogleg", iterations=None, delta=5.0, max_trials=None, initial_lambda=None,
             initial_delta=1e4, follow=None, margin=1e-6):
    """Runs the driver on a copy of g's poses.  Returns dict(poses, records, iterations, termination, F0, F, chi2, rho1,
    cholesky_failures, lambdas (every lambda a dogleg solve used), trials (every trial: it, rho, F, F', decided)),
    adjudicated (trials decided by `follow`))."""
    lev = algorithm == "levenberg"
    iterations = (50 if lev else 100) if iterations is None else iterations
    max_trials = (10 if lev else 100) if max_trials is None else max_trials
    if initial_lambda is None:
        initial_lambda = 0.0 if lev else 1e-7
    fol = _Follow(follow, margin)
    poses = g.copy_poses()
    F = objective(poses, g.edges, delta)
    out = dict(F0=F, records=dict(objective=[], step_norm=[], **{"lambda": []}, delta=[], trials=[], accepted=[]),
               termination="iterations exhausted", iterations=0, cholesky_failures=0, trials=[], adjudicated=[], lambdas=[])
    rec = out["records"]

    def push_record(Fv, step, lam, Dl, trials, acc):
        rec["objective"].append(Fv)
        rec["step_norm"].append(step)
        rec["lambda"].append(lam)
        rec["delta"].append(Dl)
        rec["trials"].append(trials)
        rec["accepted"].append(acc)

    n = 6 * len(g.free)
    if n == 0:
        iterations = 0
    lam, nu, Dl, was_pd = 0.0, 2.0, initial_delta, True
    if not lev:
        lam = initial_lambda
    for it in range(iterations):
        H, b, _, _, _ = linearise(g, delta, poses)
        out["iterations"] = it + 1
        if lev:
            if it == 0:
                lam = initial_lambda if initial_lambda > 0 else 1e-5 * float(np.max(np.abs(np.diag(H))))
                nu = 2.0
            trials, rho, acc, step = 0, 0.0, 0, 0.0
            while True:
                x, ok = cholesky_solve(H + lam * np.eye(n), b)
                if ok:
                    trial = apply(g, poses, x)
                    Fp = objective(trial, g.edges, delta)
                    rho = (F - Fp) / (float(np.sum(x * (lam * x + b))) + 1e-3)
                else:
                    out["cholesky_failures"] += 1
                    Fp, rho = np.inf, -np.inf
                d = fol.decide(it, trials, rho, [0.0]) if np.isfinite(rho) else None
                out["trials"].append(dict(it=it, rho=rho, F=F, Fp=Fp, decided=d))
                if d is not None:
                    out["adjudicated"].append(out["trials"][-1])
                    last = trials == int(follow["trials"][it]) - 1
                    if d:
                        rho = 1e-300
                    else:  # a last rejection before max_trials means the library saw rho == 0
                        rho = 0.0 if (last and trials + 1 < max_trials) else -1e-300
                if rho > 0 and np.isfinite(Fp):
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    nu = 2.0
                    F, poses, acc, step = Fp, trial, 1, float(np.sqrt(x @ x))
                else:
                    lam *= nu
                    nu *= 2.0
                    if not np.isfinite(lam):
                        break
                trials += 1
                if not (rho < 0 and trials < max_trials):
                    break
            push_record(F, step, lam, 0.0, trials, acc)
            if trials == max_trials or rho == 0 or not np.isfinite(lam):
                out["termination"] = "terminate"
                break
        else:
            Hb = H @ b
            alpha = float(b @ b) / float(Hb @ b)
            hsd = alpha * b
            hsd_norm = float(np.sqrt(hsd @ hsd))
            hgn, hgn_norm, solved, good, trials, step = None, -1.0, False, False, 0, 0.0
            while True:
                trials += 1
                if not solved:
                    solved = True
                    ok = False
                    while not ok:
                        A = H if was_pd else H + lam * np.eye(n)
                        if not was_pd:
                            out["lambdas"].append(lam)
                        hgn, ok = cholesky_solve(A, b)
                        if not ok:
                            out["cholesky_failures"] += 1
                        was_pd = was_pd and ok
                        if not was_pd:
                            if ok:
                                lam = max(1e-12, lam / (0.5 * 10.0))
                            else:
                                lam *= 10.0
                                if lam > 1e3:
                                    lam = 1e3
                                    push_record(F, 0.0, lam, Dl, trials, 0)
                                    out["termination"] = "fail"
                                    return _finish(out, g, poses, delta, F)
                    hgn_norm = float(np.sqrt(hgn @ hgn))
                if hgn_norm < Dl:
                    hdl = hgn.copy()
                elif hsd_norm > Dl:
                    hdl = (Dl / hsd_norm) * hsd
                else:
                    aux = hgn - hsd
                    c = float(hsd @ aux)
                    bma = float(aux @ aux)
                    hsq = float(hsd @ hsd)
                    if c <= 0:
                        beta = (-c + np.sqrt(c * c + bma * (Dl * Dl - hsq))) / bma
                    else:
                        beta = (Dl * Dl - hsq) / (c + np.sqrt(c * c + bma * (Dl * Dl - hsq)))
                    hdl = hsd + beta * (hgn - hsd)
                gain = -1.0 * float((H @ hdl) @ hdl) + 2.0 * float(b @ hdl)
                trial = apply(g, poses, hdl)
                Fp = objective(trial, g.edges, delta)
                if abs(gain) < 1e-12:
                    gain = 1e-12
                rho = (F - Fp) / gain
                hdl_norm = float(np.sqrt(hdl @ hdl))
                d = fol.decide(it, trials - 1, rho, [0.0, 0.25, 0.75])
                out["trials"].append(dict(it=it, rho=rho, F=F, Fp=Fp, decided=d))
                if d is not None:
                    out["adjudicated"].append(out["trials"][-1])
                    if abs(rho) < margin:  # near 0: the follower's decision; either way rho < 0.25 halves Delta
                        rho = 1e-300 if d else -1e-300
                    elif follow is not None and trials == int(follow["trials"][it]):
                        # near 0.25 / 0.75 on the last trial: the trust region the library kept
                        if rho > 0:
                            good, F, poses, step = True, Fp, trial, hdl_norm
                        Dl = float(follow["delta"][it])
                        if good or trials >= max_trials:
                            break
                        continue
                if rho > 0:
                    good, F, poses, step = True, Fp, trial, hdl_norm
                if rho > 0.75:
                    Dl = max(Dl, 3.0 * hdl_norm)
                elif rho < 0.25:
                    Dl *= 0.5
                if good or trials >= max_trials:
                    break
            push_record(F, step, lam, Dl, trials, int(good))
            if trials == max_trials or not good:
                out["termination"] = "terminate"
                break
    out["lambda"], out["delta"] = lam, Dl
    return _finish(out, g, poses, delta, F)


def _finish(out, g, poses, delta, F):
    chi2, rho0, rho1 = edge_terms(poses, g.edges, delta) if g.edges else (np.zeros(0),) * 3
    out.update(poses=poses, F=F, F_final=float(np.sum(rho0)), chi2=chi2, rho1=rho1)
    out["records"] = {k: np.asarray(v) for k, v in out["records"].items()}
    return out


def gradient_norm(g: Graph, poses, delta):
    """|J^T W e| at the estimate: b of the normal equations"""
    return float(np.linalg.norm(linearise(g, delta, poses)[1]))


# ---- synthetic graphs ---------------------------------------------------------------------------------------------------------
def _exp(xi):
    from dvo_slam_amd import synth

    return synth.se3_exp(xi)


def ring_truth(m, radius=3.0, seed=0):
    """m poses on a ring of the given radius, facing along it, with a little hashed wobble"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(m):
        a = 2 * np.pi * i / m
        T = np.eye(4)
        c, s = np.cos(a), np.sin(a)
        T[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        T[:3, 3] = [radius * c, radius * s, 0.0]
        out.append(T @ _exp(np.r_[rng.normal(scale=0.02, size=3), rng.normal(scale=0.02, size=3)]))
    return out


def information(rng, scale=1.0):
    A = rng.normal(size=(6, 6)) * 0.1
    O = np.diag([400.0, 400.0, 400.0, 2500.0, 2500.0, 2500.0]) * scale + A @ A.T
    return 0.5 * (O + O.T)


def ring_graph(m, n_chords=20, star=0, seed=0, drift=0.02, noise=0.0, fixed_first=True, radius=3.0):
    """Truth on a ring; odometry edges i -> i+1 (and m-1 -> 0), `star` keyframe edges from every `star`-th vertex to the
    next keyframe, n_chords random chords; measurements = the true relative poses (times exp(noise)), initial estimate = the
    odometry chained with a drift of `drift` (twist per step, hashed).  Returns (Graph, truth)."""
    rng = np.random.default_rng(seed)
    truth = ring_truth(m, radius, seed)
    pairs = [(i, (i + 1) % m) for i in range(m)]
    if star:
        keys = list(range(0, m, star))
        for a in keys:
            for v in range(a + 2, min(a + star + 1, m)):
                pairs.append((a, v))
    chords = 0
    while chords < n_chords:
        a, c = sorted(int(v) for v in rng.choice(m, size=2, replace=False))
        if c - a > 2 and (a, c) not in pairs:
            pairs.append((a, c))
            chords += 1
    edges = []
    for f, t in pairs:
        Z = inverse(truth[f]) @ truth[t]
        if noise > 0:
            Z = Z @ _exp(rng.normal(scale=noise, size=6))
        edges.append((f, t, Z, information(rng)))
    poses = [truth[0].copy()]
    for i in range(1, m):
        step = inverse(truth[i - 1]) @ truth[i]
        poses.append(poses[-1] @ step @ _exp(rng.normal(scale=drift, size=6)))
    fixed = [fixed_first] + [False] * (m - 1)
    return Graph(poses, fixed, edges), truth


def rms_position(poses, truth):
    return float(np.sqrt(np.mean([np.sum((P[:3, 3] - T[:3, 3]) ** 2) for P, T in zip(poses, truth)])))
