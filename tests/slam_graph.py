"""A pose graph shaped like the reference's dense final graph (FinalOptimizationUseDenseGraph: one vertex per frame), from a
seeded synthetic trajectory: frames 0..F-1 with a keyframe every k frames; per frame an odometry edge from the previous frame
and an edge from its local map's keyframe (the last frame of a local map is the next keyframe); keyframe-keyframe constraints
between keyframes within a radius, and a few long loop closures.  Measurements are the true relative poses times seeded
noise, the initial estimate chains the odometry with drift, and the first keyframe is fixed."""
from __future__ import annotations

import numpy as np

import pose_graph_restatement as R


def truth_trajectory(n_frames, seed=0, lap=400, radius=2.5):
    """laps around a wobbling loop, so that later keyframes come back near earlier ones"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_frames):
        a = 2 * np.pi * i / lap
        r = radius * (1.0 + 0.1 * np.sin(3 * a)) + 0.05 * (i // lap)
        T = np.eye(4)
        c, s = np.cos(a), np.sin(a)
        T[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        T[:3, 3] = [r * c, r * s, 0.2 * np.sin(a * 2.0)]
        out.append(T @ R._exp(np.r_[rng.normal(scale=0.01, size=3), rng.normal(scale=0.01, size=3)]))
    return out


def slam_graph(n_frames, k=15, kf_radius=0.6, max_kf_links=3, n_loops=4, seed=0, noise=0.0, drift=0.01, lap=400):
    """Returns (Graph, truth, keyframes)."""
    rng = np.random.default_rng(seed)
    truth = truth_trajectory(n_frames, seed, lap)
    keys = list(range(0, n_frames, k))
    pairs = []
    for i in range(1, n_frames):
        pairs.append((i - 1, i))                      # odometry
        kf = ((i - 1) // k) * k                       # the local map's keyframe; frame kf + k is the next keyframe
        if kf != i - 1:
            pairs.append((kf, i))
    pos = np.array([truth[a][:3, 3] for a in keys])
    for ai, a in enumerate(keys):                     # keyframe-keyframe constraints within the radius
        d = np.linalg.norm(pos - pos[ai], axis=1)
        near = [bi for bi in np.argsort(d, kind="stable") if bi > ai + 1 and d[bi] < kf_radius][:max_kf_links]
        pairs.extend((a, keys[bi]) for bi in near)
    have = set(pairs)
    loops = 0
    while loops < n_loops and len(keys) > 8:          # a few long loop closures
        a, b = sorted(int(v) for v in rng.choice(len(keys), size=2, replace=False))
        if b - a > len(keys) // 3 and (keys[a], keys[b]) not in have:
            pairs.append((keys[a], keys[b]))
            have.add((keys[a], keys[b]))
            loops += 1
    edges = []
    for f, t in pairs:
        Z = R.inverse(truth[f]) @ truth[t]
        if noise > 0:
            Z = Z @ R._exp(rng.normal(scale=noise, size=6))
        edges.append((f, t, Z, R.information(rng)))
    poses = [truth[0].copy()]
    for i in range(1, n_frames):
        step = R.inverse(truth[i - 1]) @ truth[i]
        poses.append(poses[-1] @ step @ R._exp(rng.normal(scale=drift, size=6)))
    fixed = [True] + [False] * (n_frames - 1)
    return R.Graph(poses, fixed, edges), truth, keys
