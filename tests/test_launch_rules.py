"""The host-only launch rules (dvo_slam_amd/csrc/dvo_launch_rules.h) as a stand-alone program under ASan and UBSan: the rows of a
two-dimensional grid against the formula restated here, and the three transform helpers against numpy float64 in the same index
order with one cast at the end, compared on bit patterns.  No device, nothing loaded into Python."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _poses():
    """column-major 4x4 doubles: the identity, a 90 degree turn with a translation, a general rigid pose with entries of 1e-3 and 1e3"""
    identity = np.eye(4)
    turn = np.eye(4)
    turn[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    turn[:3, 3] = [0.25, -1.5, 2.0]
    a, b, c = 1.0e-3, 0.7, -0.3  # rotations about x, y, z: the first leaves entries of about 1e-3
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    general = np.eye(4)
    general[:3, :3] = rx @ ry @ rz
    general[:3, 3] = [1.0e3, -1.0e-3, 2.5]
    return [np.asarray(p, np.float64).flatten(order="F") for p in (identity, turn, general)]


def _rows(T):
    M = np.zeros(12, F)
    for r in range(3):
        for c in range(4):
            M[r * 4 + c] = F(T[c * 4 + r]) if T is not None else F(1.0 if r == c else 0.0)
    return M


def _inverse(T):
    if T is None:
        return _rows(None)
    M = np.zeros(12, F)
    t0, t1, t2 = T[12], T[13], T[14]
    for r in range(3):
        for c in range(3):
            M[r * 4 + c] = F(T[r * 4 + c])
        M[r * 4 + 3] = F(-((T[r * 4 + 0] * t0 + T[r * 4 + 1] * t1) + T[r * 4 + 2] * t2))
    return M


def _relative(A, B):
    M = np.zeros(12, F)
    for r in range(3):
        i0, i1, i2 = B[r * 4 + 0], B[r * 4 + 1], B[r * 4 + 2]
        ti = -((i0 * B[12] + i1 * B[13]) + i2 * B[14])
        for c in range(3):
            M[r * 4 + c] = F((i0 * A[c * 4 + 0] + i1 * A[c * 4 + 1]) + i2 * A[c * 4 + 2])
        M[r * 4 + 3] = F(((i0 * A[12] + i1 * A[13]) + i2 * A[14]) + ti)
    return M


def _bits(M):
    return " ".join("%08x" % b for b in np.asarray(M, F).view(np.uint32))


def _hex(T):
    return " ".join(float(v).hex() for v in T)


def test_the_launch_rules_are_clean_under_sanitizers_and_equal_python(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++11", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off"]
    if subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no ASan / UBSan runtime")
    exe = tmp_path / "launch_rules"
    res = subprocess.run([cxx] + flags + ["-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "dvo_slam_amd", "csrc"),
                                          os.path.join(ROOT, "tests", "launch_rules_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr

    lines, want, grids = [], [], []
    for block in (64, 256, 1024):
        for n, gx in itertools.product((0, 1, 65535, 65536, 2**31 - 1), (1, 2**23 // block, 2**31 // block, 2**31 // block + 1)):
            lines.append("grid %d %d %d" % (n, gx, block))
            want.append(str(max(1, min(min(n, 65535), 2**31 // (gx * block)))))  # the formula, restated
            grids.append((n, gx, block))
    poses = _poses()
    assert any(0.0 < abs(v) < 2.0e-3 for v in poses[2]) and any(abs(v) >= 1.0e3 for v in poses[2])
    for T in [None] + poses:
        text = "null" if T is None else _hex(T)
        lines += ["rows " + text, "inverse " + text]
        want += [_bits(_rows(T)), _bits(_inverse(T))]
    for A, B in itertools.product(poses, poses):
        lines.append("relative " + _hex(A) + " " + _hex(B))
        want.append(_bits(_relative(A, B)))

    res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0 and "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr, res.stderr
    got = res.stdout.strip().splitlines()
    assert got == want
    for (n, gx, block), gy in zip(grids, (int(g) for g in got)):
        assert 1 <= gy <= max(1, min(n, 65535))
        if gx * block <= 2**31:
            assert gx * gy * block <= 2**31
    # the helpers against each other: a null pose (either way), the identity and relative(identity, identity) are the same rows
    # (the identity's inverse is not: its translation is -0)
    assert got[len(grids)] == got[len(grids) + 1] == got[len(grids) + 2] == got[len(grids) + 8]
