"""The fp64 arithmetic of the geometric verification (csrc/msfm_fmat.h, through the host entry points of libmsfm_host.so)
against the independent float64 reference oracle/fmat_ref.py: sampling, logarithm, stopping rule, per-hypothesis F,
the inlier decision, the consensus refit and the whole RANSAC.  The device kernels share the header with the host twin,
so device == twin (tests/test_gpu_verify.py) cannot see a wrong formula; these tests can.  CPU only."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import fmat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
F32 = np.float32
EPS = np.finfo(np.float64).eps
FP, DP, IP, UP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def L():
    subprocess.check_call(["make", "-C", HOST, "-s", "libmsfm_host.so"])
    L = C.CDLL(os.path.join(HOST, "libmsfm_host.so"))
    L.host_fmat_sample8.argtypes = [C.c_ulonglong, C.c_int, C.c_int, IP]
    L.host_fmat_hypothesis.argtypes = [FP, FP, FP, FP, C.c_int, C.c_ulonglong, C.c_int, DP]
    L.host_fmat_refit.argtypes = [FP, FP, FP, FP, C.c_int, UP, DP]
    L.host_fmat_epipolar_error.argtypes = [DP, C.c_float, C.c_float, C.c_float, C.c_float]
    L.host_fmat_epipolar_error.restype = C.c_double
    L.host_fmat_det_log.argtypes = [C.c_double]
    L.host_fmat_det_log.restype = C.c_double
    L.host_fmat_replay.argtypes = [IP, C.c_int, C.c_int, C.c_int, C.c_double, IP]
    L.host_fmat_counts.argtypes = [FP, FP, FP, FP, C.c_int, C.c_ulonglong, C.c_int, C.c_double, IP]
    L.host_fundamental_ransac_ex.argtypes = [FP, FP, C.c_int, C.c_double, C.c_double, C.c_int, C.c_ulonglong, UP]
    return L


def cols(p1, p2):
    return [np.ascontiguousarray(c, F32) for c in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1])]


def lib_hypothesis(L, p1, p2, seed, it):
    F = np.zeros(9)
    c = cols(p1, p2)
    ok = L.host_fmat_hypothesis(*[a.ctypes.data_as(FP) for a in c], len(p1), seed, it, F.ctypes.data_as(DP))
    return bool(ok), F


def lib_refit(L, p1, p2, mask):
    F = np.zeros(9)
    c = cols(p1, p2)
    m = np.ascontiguousarray(mask, np.uint8)
    ok = L.host_fmat_refit(*[a.ctypes.data_as(FP) for a in c], len(p1), m.ctypes.data_as(UP), F.ctypes.data_as(DP))
    return bool(ok), F


def lib_counts(L, p1, p2, seed, max_iters, thr2):
    out = np.zeros(max_iters, np.int32)
    c = cols(p1, p2)
    L.host_fmat_counts(*[a.ctypes.data_as(FP) for a in c], len(p1), seed, max_iters, thr2, out.ctypes.data_as(IP))
    return out


def lib_ransac(L, p1, p2, thr, conf, max_iters, seed):
    p1 = np.ascontiguousarray(p1, F32)
    p2 = np.ascontiguousarray(p2, F32)
    mask = np.zeros(max(len(p1), 1), np.uint8)
    n = L.host_fundamental_ransac_ex(p1.ctypes.data_as(FP), p2.ctypes.data_as(FP), len(p1), thr, conf, max_iters, seed,
                                     mask.ctypes.data_as(UP))
    return mask[:n].astype(bool) if n else None


def lib_replay(L, counts, n, max_iters, conf):
    c = np.ascontiguousarray(counts, np.int32)
    best = C.c_int()
    it = L.host_fmat_replay(c.ctypes.data_as(IP), len(c), n, max_iters, conf, C.byref(best))
    return it, best.value


# ---- scenes ---------------------------------------------------------------------------------------------------------
K = np.array([[2559.68, 0, 1536], [0, 2559.68, 1152], [0, 0, 1]])


def scene(kind, n, rng, noise=0.5, outliers=0.0):
    """n matches (float32 pixel coordinates) of one of the families; the first round((1 - outliers) n) obey the geometry."""
    n_in = int(round(n * (1.0 - outliers)))
    if kind == "planar":   # a 2 cm relief on a plane 6 m away
        X = np.c_[rng.uniform(-2, 2, n_in), rng.uniform(-1.5, 1.5, n_in), 6 + rng.normal(0, 0.01, n_in)]
    else:
        X = np.c_[rng.uniform(-2, 2, n_in), rng.uniform(-1.5, 1.5, n_in), rng.uniform(4, 9, n_in)]
    a = 0.1 + 0.1 * rng.random()
    Rm = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.8, 0.05, 0.1])
    if kind == "small_baseline":
        Rm, t = np.eye(3), t * 0.02
    x1 = (K @ X.T).T
    x1 = x1[:, :2] / x1[:, 2:]
    x2 = (K @ (Rm @ X.T + t[:, None])).T
    x2 = x2[:, :2] / x2[:, 2:]
    x1 = x1 + rng.normal(0, noise, x1.shape)
    x2 = x2 + rng.normal(0, noise, x2.shape)
    rnd = lambda m: np.c_[rng.uniform(0, 3072, m), rng.uniform(0, 2304, m)]
    x1 = np.r_[x1, rnd(n - n_in)]
    x2 = np.r_[x2, rnd(n - n_in)]
    if kind == "offset":
        x1, x2 = x1 + 1e5, x2 - 1e5
    if kind == "negative":
        x1, x2 = x1 - 3000.0, x2 - 2500.0
    return x1.astype(F32), x2.astype(F32)


FAMILIES = ["general", "planar", "small_baseline", "offset", "negative"]


def f64(p1, p2):
    return [np.asarray(c, np.float64) for c in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1])]


# ---- sampling -------------------------------------------------------------------------------------------------------
def _probes(seed, it, n):
    """True when some slot of the sample exhausts its 32 hashed draws and falls back to the linear probe."""
    idx = []
    for k in range(8):
        for attempt in range(32):
            c = R.mix64(seed ^ R.mix64(((it << 20) ^ (k << 8) ^ attempt) & R.MASK64)) % n
            if c not in idx:
                break
        else:
            return True
        idx.append(c)
    return False


@pytest.mark.parametrize("n", [8, 9, 1 << 20])
@pytest.mark.parametrize("seed", [0, 0x5EED5EED, U64_MAX])
def test_sample8_equals_the_splitmix_port(L, n, seed):
    its = list(range(0, 300)) + [1023, 1024, 4095, 4096, 32767, 65534, 65535]
    idx = np.zeros(8, np.int32)
    probed = 0
    for it in its:
        L.host_fmat_sample8(seed, it, n, idx.ctypes.data_as(IP))
        ref = R.sample8(seed, it, n)
        assert idx.tolist() == ref, (seed, it, n)
        assert len(set(ref)) == 8 and min(ref) >= 0 and max(ref) < n
        probed += _probes(seed, it, n)
    if n == 8:
        assert probed > 0    # the linear probe after 32 attempts is exercised


# ---- logarithm ------------------------------------------------------------------------------------------------------
CONFS = [0.5, 0.99, 0.999999, 1e-6, 1.0 - 1e-12]


def test_det_log_within_4_ulp_of_math_log(L):
    xs = []
    for e in range(-1022, 1024):
        x = math.ldexp(1.0, e)
        xs += [x, np.nextafter(x, np.inf), np.nextafter(x, 0.0) if e > -1022 else x]
    r2 = 1.4142135623730951
    xs += [r2, np.nextafter(r2, 0.0), np.nextafter(r2, np.inf), 1.0 - 2.0 ** -53, 1e-300, sys.float_info.min,
           0.5 * r2, np.nextafter(0.5 * r2, 0.0), np.nextafter(0.5 * r2, np.inf), sys.float_info.max]
    xs += [1.0 - c for c in CONFS]
    xs += [1.0 - w ** 8 for w in np.linspace(0.05, 0.999, 200)]
    worst = 0.0
    for x in xs:
        got, ref = L.host_fmat_det_log(float(x)), math.log(float(x))
        ulps = abs(got - ref) / math.ulp(ref) if ref != 0.0 else abs(got) / math.ulp(0.0)
        worst = max(worst, ulps)
        assert ulps <= 4.0, (x, got, ref)
    assert L.host_fmat_det_log(1.0) == 0.0


# ---- stopping rule --------------------------------------------------------------------------------------------------
def _replay_cases():
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(150):   # random sequences, counts mostly rising slowly
        n = int(rng.choice([8, 9, 50, 600, 3000]))
        m = int(rng.choice([1, 7, 255, 256, 257, 1000, 4096]))
        counts = np.minimum(n, rng.geometric(rng.uniform(0.02, 0.6), m) - 1 + int(rng.integers(0, n)) * (rng.random(m) < 0.05))
        cases.append((counts, n, m, float(rng.choice(CONFS))))
    cases.append((np.arange(1000) % 8, 600, 1000, 0.99))                  # counts below 8: nothing wins
    cases.append((np.r_[9, 50, 50, 50], 50, 4, 0.99))                      # w = 1: q clamped to 1e-300
    cases.append((np.full(1000, 0) + np.r_[np.arange(8, 108), np.zeros(900, int)], 1 << 20, 1000, 0.99))  # w^8 < 2^-53
    cases.append((np.r_[500], 600, 1, 0.99))                               # max_iters = 1
    for conf in (1e-6, 1.0 - 1e-12):
        cases.append((np.r_[10, 400, 100, 420, np.full(60, 430)], 600, 1000, conf))
    # the bound shrinks after it 1, and a larger count arrives before it ends
    cases.append((np.r_[20, 540, 3, 3, 545, 550, np.full(2000, 560)], 600, 4096, 0.99))
    # a need that sits on an integer: w = 1/2 and 1 - confidence = (255/256)^k
    on_integer = 0
    for k in range(2, 400):
        conf = 1.0 - (255.0 / 256.0) ** k
        if math.log(1.0 - conf) / math.log(1.0 - 0.5 ** 8) == float(k) and on_integer < 8:
            on_integer += 1
            cases.append((np.r_[300, np.full(k - 1, 100), 600], 600, 4096, conf))    # 600 at it k: just past the bound
            cases.append((np.r_[300, np.full(k - 2, 100), 600], 600, 4096, conf))    # 600 at it k - 1: the last one run
    assert on_integer == 8
    return cases


def test_replay_equals_the_literal_sequential_loop(L):
    on_integer = 0
    for counts, n, m, conf in _replay_cases():
        counts = np.asarray(counts, np.int64)
        counts = np.r_[counts, np.zeros(max(0, m - len(counts)), np.int64)][:m]
        ref = R.replay(counts, n, m, conf)[:2]
        got = lib_replay(L, counts, n, m, conf)
        # det_log is within 4 ulp of log, not equal to it: where need is an integer to the last bit, the bound may
        # come out one iteration longer; elsewhere the two are the same
        lo, hi = R.replay(counts, n, m, conf, 1.0 - 16 * EPS)[:2], R.replay(counts, n, m, conf, 1.0 + 16 * EPS)[:2]
        if lo == hi:
            assert got == ref, (counts[:20], n, m, conf)
        else:
            assert got in (lo, hi), (counts[:20], n, m, conf)
            on_integer += 1
    assert on_integer >= 1


# ---- per-hypothesis F -----------------------------------------------------------------------------------------------
COND_FLOOR = 3e-4   # sigma8 / sigma1 of the sample's normalised system


@pytest.mark.parametrize("kind", FAMILIES)
def test_hypothesis_F_equals_the_svd_reference(L, kind):
    rng = np.random.default_rng(FAMILIES.index(kind) + 20)
    compared = 0
    for trial in range(4):
        p1, p2 = scene(kind, 60, rng)
        x1, y1, x2, y2 = f64(p1, p2)
        for it in range(40):
            ok, F = lib_hypothesis(L, p1, p2, 0x5EED5EED + trial, it)
            (Fr, fn, T1, T2, sv), idx = R.hypothesis(x1, y1, x2, y2, 0x5EED5EED + trial, it)
            assert ok
            s = np.linalg.svd(F.reshape(3, 3), compute_uv=False)
            assert abs(np.linalg.norm(F) - 1.0) < 1e-14 and s[2] <= 1e-12 * s[0]      # unit norm, rank 2
            cond = sv[7] / sv[0]
            if cond < COND_FLOOR:
                continue
            compared += 1
            # the library solves the moment matrix A^T A, whose conditioning is the square of A's
            tol = 64 * EPS / cond ** 2
            sign = 1.0 if F @ Fr.reshape(9) >= 0 else -1.0
            assert np.max(np.abs(sign * F - Fr.reshape(9))) <= tol, (kind, it, cond)
            A = R.design(x1[idx], y1[idx], x2[idx], y2[idx], R.hartley(x1[idx], y1[idx]), R.hartley(x2[idx], y2[idx]))
            G = R.normalised(F, T1, T2)
            assert math.sqrt(R.residual(A, G)) <= math.sqrt(R.residual(A, fn)) + tol * sv[0]
    assert compared >= 25


@pytest.mark.parametrize("case", ["collinear", "duplicated", "identical"])
def test_degenerate_samples_give_a_finite_rank2_F(L, case):
    """Degenerate 8-point samples (collinear points, three matches repeated, all points identical) have a null space of
    more than one direction.  The solve does not report failure on them: the eps shift keeps the Cholesky factor
    alive, inverse iteration lands somewhere in the null space, and the rank-2 truncation of that vector comes back as
    a finite, unit-norm, rank-2 F.  The truncation need not satisfy the sample's constraints (it does not, here), so
    such a hypothesis simply scores low; what matters is that nothing is NaN or infinite."""
    rng = np.random.default_rng(["collinear", "duplicated", "identical"].index(case))
    for trial in range(20):
        if case == "collinear":
            s = rng.uniform(0, 3000, 8)
            p1 = np.c_[s, 0.5 * s + 100]
            p2 = np.c_[s * 0.9 + 30, 0.4 * s + 200]
        elif case == "duplicated":
            q1, q2 = scene("general", 3, rng)
            p1, p2 = q1[[0, 1, 2, 0, 1, 2, 0, 1]], q2[[0, 1, 2, 0, 1, 2, 0, 1]]
        else:
            p1 = np.tile(rng.uniform(0, 3000, 2), (8, 1))
            p2 = np.tile(rng.uniform(0, 3000, 2), (8, 1))
        p1, p2 = np.asarray(p1, F32), np.asarray(p2, F32)
        ok, F = lib_hypothesis(L, p1, p2, 1, 0)
        assert ok, (case, trial)
        s = np.linalg.svd(F.reshape(3, 3), compute_uv=False)
        assert np.all(np.isfinite(F)) and abs(np.linalg.norm(F) - 1.0) < 1e-14 and s[2] <= 1e-12 * s[0]


# ---- inlier decision ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.05, 1.0, 3.0, 30.0])
def test_epipolar_decisions_equal_the_exact_decisions(L, thr):
    """Points whose second image coordinate is the float32 on either side of the threshold crossing (by bisection on
    y2), and points spread around it: every decision of the library's float64 error equals the exact rational one."""
    rng = np.random.default_rng(int(thr * 100))
    thr2 = thr * thr
    p1, p2 = scene("general", 60, rng)
    Fr = R.fit(*f64(p1, p2))[0].reshape(9)
    Fp = np.ascontiguousarray(Fr)
    err = lambda a, b, c, d: L.host_fmat_epipolar_error(Fp.ctypes.data_as(DP), a, b, c, d)
    checked = 0
    for i in range(60):
        a, b, c = (float(v) for v in (p1[i, 0], p1[i, 1], p2[i, 0]))
        for side in (-1.0, 1.0):
            lo, hi = np.float32(p2[i, 1]), np.float32(p2[i, 1] + side * 4 * thr)
            if not (err(a, b, c, float(lo)) <= thr2 < err(a, b, c, float(hi))):
                continue
            while np.nextafter(lo, hi) != hi:     # adjacent float32 values bracketing thr^2
                mid = np.float32(0.5 * (float(lo) + float(hi)))
                if mid in (lo, hi):
                    break
                if err(a, b, c, float(mid)) <= thr2:
                    lo = mid
                else:
                    hi = mid
            for d in (lo, hi, np.nextafter(lo, -hi), np.nextafter(hi, 2 * hi - lo)):
                assert (err(a, b, c, float(d)) <= thr2) == R.exact_inlier(Fr, a, b, c, d, thr2), (i, d)
                checked += 1
        for d in np.float32(p2[i, 1] + rng.uniform(-3 * thr, 3 * thr, 8)):
            got = err(a, b, c, float(d)) <= thr2
            assert got == R.exact_inlier(Fr, a, b, c, d, thr2)
            assert got == R.decisions(Fr, np.r_[a], np.r_[b], np.r_[c], np.r_[float(d)], thr2)[0]
            checked += 1
    assert checked >= 300


# ---- refit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", FAMILIES)
def test_refit_reaches_the_least_squares_optimum(L, kind):
    """The consensus refit's F (rank 2, normalised frame) has an algebraic residual within (1 + 1e-9) of the SVD
    optimum followed by the SVD rank-2 truncation, including where sigma9 / sigma8 is close to 1."""
    rng = np.random.default_rng(FAMILIES.index(kind) + 40)
    worst = 0.0
    for trial in range(40):
        n = int(rng.integers(8, 601))
        p1, p2 = scene(kind, n, rng)
        mask = rng.random(n) < 0.9
        mask[:8] = True
        q1, q2 = p1[mask], p2[mask]
        x1, y1, x2, y2 = f64(q1, q2)
        _, fn, T1, T2, sv = R.fit(x1, y1, x2, y2)
        A = R.design(x1, y1, x2, y2, R.hartley(x1, y1), R.hartley(x2, y2))
        ok, F = lib_refit(L, p1, p2, mask)
        assert ok
        ratio = R.residual(A, R.normalised(F, T1, T2)) / R.residual(A, fn)
        worst = max(worst, ratio)
        assert ratio <= 1.0 + 1e-9, (kind, trial, n, sv[8] / sv[7], ratio)


# ---- whole RANSAC ---------------------------------------------------------------------------------------------------
RANSAC_GRID = [  # (n, outlier fraction, thr, confidence, max_iters, seed)
    (8, 0.0, 3.0, 0.99, 1000, 0x5EED5EED),
    (9, 0.0, 1.0, 0.99, 1000, 0),
    (9, 0.2, 3.0, 0.999999, 257, U64_MAX),
    (50, 0.0, 3.0, 0.99, 1000, 7),
    (50, 0.5, 1.0, 0.5, 255, 0x5EED5EED),
    (50, 0.9, 3.0, 0.99, 256, 0),
    (600, 0.3, 3.0, 0.99, 1000, 0x5EED5EED),
    (600, 0.6, 0.05, 0.999999, 1, 7),
    (600, 0.5, 30.0, 0.99, 7, U64_MAX),
    (600, 0.9, 3.0, 0.999999, 4096, 7),
    (3000, 0.4, 3.0, 0.99, 1000, 0),
    (3000, 0.0, 1.0, 0.999999, 257, U64_MAX),
]


@pytest.mark.parametrize("n,out,thr,conf,iters,seed", RANSAC_GRID)
def test_ransac_equals_the_reference(L, n, out, thr, conf, iters, seed):
    rng = np.random.default_rng(n * 7 + int(out * 10) + iters)
    p1, p2 = scene("general", n, rng, outliers=out)
    ref = R.ransac(p1, p2, thr, conf, iters, seed)
    got = lib_ransac(L, p1, p2, thr, conf, iters, seed)
    top = len(ref["sure"])
    counts = lib_counts(L, p1, p2, seed, max(top, 1), thr * thr)[:top]
    assert np.all(counts >= np.asarray(ref["sure"], int)) and np.all(counts <= np.asarray(ref["possible"], int))
    assert ref["decided"], "the margins leave the winner open: pick another scene"
    x1, y1, x2, y2 = f64(p1, p2)
    it, best = lib_replay(L, counts, n, iters, conf)
    assert (it, best) == (ref["best_it"], ref["best_count"])
    diff = got != ref["mask"]
    assert not np.any(diff & ~ref["unsure"])
    assert ref["unsure"].sum() <= max(2, n // 500)
    if ref["best_it"] >= 0 and out < 0.5 and thr >= 3.0:
        assert got[: int(round(n * (1 - out)))].mean() >= 0.9


@pytest.mark.parametrize("n", [0, 3, 6, 7])
def test_small_counts_follow_the_contract(L, n):
    rng = np.random.default_rng(n)
    p1, p2 = scene("general", max(n, 1), rng)
    p1, p2 = p1[:n], p2[:n]
    got = lib_ransac(L, p1, p2, 3.0, 0.99, 1000, 0x5EED5EED)
    ref = R.ransac(p1, p2, 3.0)
    if n < 7:
        assert got is None and ref["mask"] is None
    else:
        assert got.all() and ref["mask"].all()


def test_fewer_than_8_inliers_keep_nothing(L):
    rng = np.random.default_rng(5)
    p1 = rng.uniform(0, 3000, (40, 2)).astype(F32)
    p2 = rng.uniform(0, 3000, (40, 2)).astype(F32)
    ref = R.ransac(p1, p2, 0.05, 0.99, 300, 1)
    got = lib_ransac(L, p1, p2, 0.05, 0.99, 300, 1)
    assert ref["best_it"] == -1 and not ref["mask"].any() and not got.any()
