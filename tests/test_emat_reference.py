"""The fp64 arithmetic of the calibrated verification (csrc/msfm_emat.h, through the host entry points of libmsfm_host.so)
against the independent reference tests/emat_ref.py: undistortion, sampling, the 5-point solution set, the Sampson error,
the stopping rule with sample size 5 and the whole RANSAC of the host twin.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emat_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
FP, DP, IP, UP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
CAM0 = (520.0, 515.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0)
DISTORTIONS = [(0.0, 0.0, 0.0, 0.0), (-0.2, 0.05, 0.0, 0.0), (0.12, -0.03, 1e-3, -2e-3), (-0.05, 0.0, -2e-3, 1e-3)]


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-C", HOST, "-s", "libmsfm_host.so"])
    L = C.CDLL(os.path.join(HOST, "libmsfm_host.so"))
    L.host_emat_undistort.argtypes = [DP, DP, C.c_int, DP]
    L.host_emat_sample5.argtypes = [C.c_ulonglong, C.c_int, C.c_int, IP]
    L.host_emat_five_point.argtypes = [DP, DP, DP, DP]
    L.host_emat_sampson.argtypes = [DP, C.c_double, C.c_double, C.c_double, C.c_double]
    L.host_emat_sampson.restype = C.c_double
    L.host_emat_replay.argtypes = [IP, C.c_int, C.c_int, C.c_int, C.c_double, IP, IP]
    L.host_essential_ransac.argtypes = [FP, FP, C.c_int, DP, C.c_double, C.c_double, C.c_int, C.c_ulonglong, UP]
    return L


def d(a):
    return np.ascontiguousarray(a, np.float64)


def lib_five_point(L, q1, q2):
    E = np.zeros(90)
    roots = np.zeros(10)
    ns = L.host_emat_five_point(d(q1).ctypes.data_as(DP), d(q2).ctypes.data_as(DP), E.ctypes.data_as(DP), roots.ctypes.data_as(DP))
    return [E[9 * s:9 * s + 9].reshape(3, 3) for s in range(ns)], roots[:ns]


def rot(rng, scale):
    w = rng.normal(size=3) * scale
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene(rng, n, planar=False):
    """n points seen by two calibrated cameras: normalised coordinates q1, q2 and the true E (unit norm)."""
    R_ = rot(rng, 0.15)
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    if planar:
        X = np.c_[rng.uniform(-2, 2, (n, 2)), np.zeros(n)]
        X[:, 2] = 6.0 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    else:
        X = np.c_[rng.uniform(-2, 2, (n, 2)), rng.uniform(4, 9, n)]
    Y = X @ R_.T + t
    q1 = X[:, :2] / X[:, 2:]
    q2 = Y[:, :2] / Y[:, 2:]
    E = R.essential_from_pose(R_, t)
    return q1, q2, E / np.linalg.norm(E)


def same_up_to_sign(A, B):
    return min(np.abs(A - B).max(), np.abs(A + B).max())


@pytest.mark.parametrize("dist", DISTORTIONS)
def test_undistort_matches_newton(L, dist):
    cam = CAM0[:4] + dist
    u, v = np.meshgrid(np.linspace(0, 640, 17), np.linspace(0, 480, 13))
    uv = d(np.c_[u.ravel(), v.ravel()])
    out = np.zeros_like(uv)
    L.host_emat_undistort(d(cam).ctypes.data_as(DP), uv.ctypes.data_as(DP), len(uv), out.ctypes.data_as(DP))
    ref = np.array([R.undistort(cam, a, b) for a, b in uv])
    scale = np.maximum(np.abs(ref), 1e-3)   # (relative, with the centre's zero crossing measured against 1e-3)
    assert np.max(np.abs(out - ref) / scale) <= 1e-12
    if dist == (0.0, 0.0, 0.0, 0.0):   # no loop: exact
        assert np.array_equal(out[:, 0], (uv[:, 0] - cam[2]) / cam[0]) and np.array_equal(out[:, 1], (uv[:, 1] - cam[3]) / cam[1])


def test_sample5_stream(L):
    idx = (C.c_int * 5)()
    for seed in (0x5EED5EED, 1, (1 << 64) - 1):
        for n in (5, 6, 7, 50, 1000):
            for it in (0, 1, 17, 999):
                L.host_emat_sample5(seed, it, n, idx)
                got = list(idx)
                assert got == R.sample5(seed, it, n)
                assert len(set(got)) == 5 and all(0 <= g < n for g in got)


def test_five_point_solution_set(L):
    rng = np.random.default_rng(5)
    compared = 0
    for trial in range(1400):
        q1, q2, _ = scene(rng, 5)
        ref, w = R.five_point(q1, q2)
        # well conditioned: eigenvalues clearly real or clearly complex, and separated
        im = np.abs(w.imag) / (1 + np.abs(w))
        if np.any((im > 1e-9) & (im < 1e-4)):
            continue
        gaps = np.abs(w[:, None] - w[None, :]) / (1 + np.abs(w[:, None]))
        if np.min(gaps + np.eye(10)) < 1e-3:
            continue
        # ... and the reference itself accurate (eig on the action matrix can lose digits): essential to 1e-10
        sv = [np.linalg.svd(E, compute_uv=False) for E in ref]
        if any((v[0] - v[1]) / v[0] > 1e-10 or v[2] / v[0] > 1e-10 for v in sv):
            continue
        got, _ = lib_five_point(L, q1, q2)
        assert len(got) == len(ref), trial
        for E in ref:
            assert min(same_up_to_sign(E, G) for G in got) <= 1e-8, trial
        for G in got:
            assert abs(np.linalg.norm(G) - 1) < 1e-12
        compared += 1
    assert compared >= 1000


@pytest.mark.parametrize("planar", [False, True])
def test_true_essential_among_solutions(L, planar):
    rng = np.random.default_rng(11 + planar)
    for _ in range(200):
        q1, q2, E = scene(rng, 5, planar)
        got, _ = lib_five_point(L, q1, q2)
        assert got and min(same_up_to_sign(E, G) for G in got) <= 1e-7


def test_sampson(L):
    rng = np.random.default_rng(3)
    for _ in range(500):
        E = rng.normal(size=(3, 3))
        x1, y1, x2, y2 = rng.normal(size=4) * 0.5
        got = L.host_emat_sampson(d(E.ravel()).ctypes.data_as(DP), x1, y1, x2, y2)
        assert abs(got - R.sampson(E, x1, y1, x2, y2)) <= 1e-13 * max(1.0, abs(got))


def test_replay_sample5_is_the_literal_loop(L):
    rng = np.random.default_rng(8)
    for trial in range(3000):
        n = int(rng.integers(5, 400))
        max_iters = int(rng.integers(1, 1200))
        conf = float(rng.choice([0.5, 0.9, 0.99, 0.999]))
        counts = np.sort(rng.integers(0, n + 1, max_iters)) if trial % 3 == 0 else rng.integers(0, n + 1, max_iters)
        counts = np.ascontiguousarray(counts, np.int32)
        want_it, want_best, ran = R.replay(counts.tolist(), n, max_iters, conf)
        bc, dec = C.c_int(), C.c_int()
        got = L.host_emat_replay(counts.ctypes.data_as(IP), max_iters, n, max_iters, conf, C.byref(bc), C.byref(dec))
        assert (got, bc.value, dec.value) == (want_it, want_best, 1)
        # staged: with only the first `avail` counts the replay is decided exactly when the loop never read beyond them
        for avail in (32, 64, ran, ran - 1):
            if avail < 1 or avail > max_iters:
                continue
            got2 = L.host_emat_replay(counts.ctypes.data_as(IP), avail, n, max_iters, conf, C.byref(bc), C.byref(dec))
            assert dec.value == (1 if ran <= avail else 0)
            if dec.value:
                assert (got2, bc.value) == (want_it, want_best)


def pixel_scene(rng, cam, n_in, n_out, planar=False, noise=0.3):
    """Pixel coordinates (float32) of a scene seen through `cam`, with planted outliers at random places."""
    q1, q2, _ = scene(rng, n_in, planar)

    def pix(q):
        xd, yd = R.distort(cam, q[:, 0], q[:, 1])
        return np.c_[cam[0] * xd + cam[2], cam[1] * yd + cam[3]] + rng.normal(size=q.shape) * noise

    p1, p2 = pix(q1), pix(q2)
    o1 = rng.uniform([0, 0], [640, 480], (n_out, 2))
    o2 = rng.uniform([0, 0], [640, 480], (n_out, 2))
    perm = rng.permutation(n_in + n_out)
    P1 = np.r_[p1, o1][perm].astype(np.float32)
    P2 = np.r_[p2, o2][perm].astype(np.float32)
    inlier = (perm < n_in)
    return P1, P2, inlier


def lib_ransac(L, cam, p1, p2, thr=3.0, conf=0.99, iters=1000, seed=0x5EED5EED):
    mask = np.zeros(max(1, len(p1)), np.uint8)
    m = L.host_essential_ransac(np.ascontiguousarray(p1, np.float32).ctypes.data_as(FP), np.ascontiguousarray(p2, np.float32).ctypes.data_as(FP),
                                len(p1), d(cam).ctypes.data_as(DP), thr, conf, iters, seed, mask.ctypes.data_as(UP))
    return mask[:m] if m else None


@pytest.mark.parametrize("dist,planar", [(DISTORTIONS[0], False), (DISTORTIONS[2], False), (DISTORTIONS[1], True)])
def test_twin_ransac_is_the_literal_loop(L, dist, planar):
    rng = np.random.default_rng(21 + planar)
    cam = CAM0[:4] + dist
    for n_in, n_out in ((60, 20), (40, 40), (120, 10)):
        p1, p2, inl = pixel_scene(rng, cam, n_in, n_out, planar)
        got = lib_ransac(L, cam, p1, p2)
        want = R.ransac(cam, p1, p2)
        assert got is not None and want is not None
        assert np.array_equal(got, want)
        assert got[inl].mean() >= 0.95 and got[~inl].mean() <= 0.35   # (random outliers near an epipolar line pass any check)


def test_small_inputs(L):
    rng = np.random.default_rng(2)
    for n in range(0, 5):
        p = rng.uniform(0, 640, (n, 2)).astype(np.float32)
        assert lib_ransac(L, CAM0, p, p) is None
    p1, p2, _ = pixel_scene(rng, CAM0, 6, 0)
    m = lib_ransac(L, CAM0, p1, p2)
    assert m is not None and m.sum() >= 5
