"""Independent float64 reference of the geometric verification (FeatureUtils::FilterMatches) -- TEST INFRASTRUCTURE ONLY.

It never calls the library and does not restate its algorithm: the library solves the 8-point system by Cholesky and
inverse iteration on the moment matrix and enforces rank 2 with a 3 x 3 Jacobi; here the null vector comes from
`np.linalg.svd` of the normalised design matrix and rank 2 from an SVD truncation, the error is evaluated directly
(and exactly with `fractions.Fraction` where it matters), and the adaptive stopping rule is the literal sequential
loop with `math.log`.

The contract encoded here (csrc/msfm_fmat.h, csrc/msfm_verify.hip.h, host/GeometricVerification.cpp):
  * n < 7 matches: no model, nothing kept; n == 7: all kept; otherwise RANSAC, and fewer than 8 inliers: nothing kept.
  * Hypothesis `it` is the normalised (Hartley: centroid, mean distance sqrt 2) 8-point F of the 8 distinct matches
    that the counter-based SplitMix sampling `sample8(seed, it, n)` picks, rank 2, unit Frobenius norm.
  * A match is an inlier of F when max(d(x2, F x1)^2, d(x1, F^T x2)^2) <= thr^2, compared in double.
  * The winner is the hypothesis the sequential loop ends with: `best` rises on a strictly larger count, and each rise
    bounds the loop at max(it + 1, ceil(log(1 - confidence) / log(1 - w^8))), w = best / n, where the bound shrinks.
  * The winner's consensus set is refitted (least squares, same normalisation, rank 2), and the refit is kept when it
    loses no inliers.
Deliberate differences from OpenCV's FM_RANSAC (SURVEY ruling, out of scope here): an 8-point solver instead of the
7-point one, w^8 and ceil in the stopping rule instead of w^7 and cvRound, and a double comparison against the
threshold instead of a float one; OpenCV's RNG stream is not reproduced.
"""
import math
from fractions import Fraction

import numpy as np

MASK64 = (1 << 64) - 1


# ---- sampling -------------------------------------------------------------------------------------------------------
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def sample8(seed, it, n):
    """The 8 distinct indices of hypothesis `it`: 32 hashed draws per slot, then a linear probe (n >= 8)."""
    idx = []
    for k in range(8):
        c = 0
        attempt = 0
        while True:
            if attempt < 32:
                c = mix64((seed & MASK64) ^ mix64(((it << 20) ^ (k << 8) ^ attempt) & MASK64)) % n
            else:
                c = (c + 1) % n
            if c not in idx:
                break
            attempt += 1
        idx.append(c)
    return idx


# ---- solver ---------------------------------------------------------------------------------------------------------
def hartley(x, y):
    """(cx, cy, s): centroid and the scale that brings the mean distance to sqrt 2."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    cx, cy = x.mean(), y.mean()
    d = np.mean(np.hypot(x - cx, y - cy))
    return cx, cy, (math.sqrt(2.0) / d if d > 1e-12 else 1.0)


def _tmat(t):
    cx, cy, s = t
    return np.array([[s, 0.0, -s * cx], [0.0, s, -s * cy], [0.0, 0.0, 1.0]])


def design(x1, y1, x2, y2, t1, t2):
    """Rows of the normalised system a . vec(F) = 0 (x2^T F x1 = 0, F row-major)."""
    a1 = (np.asarray(x1, np.float64) - t1[0]) * t1[2], (np.asarray(y1, np.float64) - t1[1]) * t1[2]
    a2 = (np.asarray(x2, np.float64) - t2[0]) * t2[2], (np.asarray(y2, np.float64) - t2[1]) * t2[2]
    u, v = a1
    p, q = a2
    one = np.ones_like(u)
    return np.stack([p * u, p * v, p, q * u, q * v, q, u, v, one], axis=-1)


def fit(x1, y1, x2, y2):
    """Normalised least-squares F of the given matches: (F pixel-space unit norm, Fn normalised rank 2 unit norm,
    T1, T2, singular values of the design matrix).  For 8 matches this is the 8-point F."""
    t1, t2 = hartley(x1, y1), hartley(x2, y2)
    A = design(x1, y1, x2, y2, t1, t2)
    _, sv, vt = np.linalg.svd(A, full_matrices=True)
    f = vt[-1].reshape(3, 3)
    u, s, wt = np.linalg.svd(f)
    fn = u @ np.diag([s[0], s[1], 0.0]) @ wt
    fn /= np.linalg.norm(fn)
    T1, T2 = _tmat(t1), _tmat(t2)
    F = T2.T @ fn @ T1
    F /= np.linalg.norm(F)
    sv = np.r_[sv, np.zeros(9 - len(sv))]
    return F, fn, T1, T2, sv


def normalised(F, T1, T2):
    """F brought back into the normalised frame of (T1, T2), unit Frobenius norm."""
    G = np.linalg.inv(T2).T @ np.asarray(F, np.float64).reshape(3, 3) @ np.linalg.inv(T1)
    return G / np.linalg.norm(G)


def residual(A, G):
    """Algebraic residual |A vec(G)|^2 of a unit-norm normalised F."""
    r = A @ np.asarray(G, np.float64).reshape(9)
    return float(r @ r)


def hypothesis(x1, y1, x2, y2, seed, it):
    idx = sample8(seed, it, len(x1))
    return fit(x1[idx], y1[idx], x2[idx], y2[idx]), idx


# ---- error and decisions --------------------------------------------------------------------------------------------
def epipolar_error(F, x1, y1, x2, y2):
    """max of the squared distances of x2 to F x1 and of x1 to F^T x2, float64 (OpenCV's form)."""
    F = np.asarray(F, np.float64).reshape(3, 3)
    p1 = np.stack([np.asarray(x1, np.float64), np.asarray(y1, np.float64), np.ones(np.shape(x1))])
    p2 = np.stack([np.asarray(x2, np.float64), np.asarray(y2, np.float64), np.ones(np.shape(x2))])
    l2 = F @ p1
    l1 = F.T @ p2
    d = np.sum(p2 * l2, axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e2 = d * d / (l2[0] ** 2 + l2[1] ** 2)
        e1 = d * d / (l1[0] ** 2 + l1[1] ** 2)
    return np.maximum(e1, e2)


def exact_inlier(F, x1, y1, x2, y2, thr2):
    """The decision max(e1, e2) <= thr2 in exact rational arithmetic on the float inputs and the double F."""
    f = [Fraction(float(v)) for v in np.asarray(F, np.float64).reshape(9)]
    a, b, c, d = (Fraction(float(v)) for v in (x1, y1, x2, y2))
    t = Fraction(float(thr2))
    l = (f[0] * a + f[1] * b + f[2], f[3] * a + f[4] * b + f[5], f[6] * a + f[7] * b + f[8])
    m = (f[0] * c + f[3] * d + f[6], f[1] * c + f[4] * d + f[7], f[2] * c + f[5] * d + f[8])
    r = c * l[0] + d * l[1] + l[2]
    n2, n1 = l[0] ** 2 + l[1] ** 2, m[0] ** 2 + m[1] ** 2
    if n1 == 0 or n2 == 0:
        return False
    return r * r <= t * n2 and r * r <= t * n1


def decisions(F, x1, y1, x2, y2, thr2, band=1e-12):
    """Inlier decisions of F: float64 where the error is clear of thr2 by a relative `band`, exact otherwise."""
    e = epipolar_error(F, x1, y1, x2, y2)
    inl = np.nan_to_num(e, nan=np.inf) <= thr2
    near = np.flatnonzero(np.abs(e - thr2) <= band * thr2)
    for i in near:
        inl[i] = exact_inlier(F, x1[i], y1[i], x2[i], y2[i], thr2)
    return inl


def intervals(e, thr2, margin):
    """(sure, possible) inlier masks of reference errors e when the F under test may move errors by margin * thr2."""
    e = np.nan_to_num(e, nan=np.inf)
    return e <= thr2 * (1.0 - margin), e <= thr2 * (1.0 + margin)


# ---- stopping rule --------------------------------------------------------------------------------------------------
def replay(counts, n, max_iters, confidence, need_scale=1.0):
    """The sequential loop, literally: (best_it or -1 below 8 inliers, best_count, iterations run).  need_scale != 1
    moves every bound by a relative amount (a logarithm a few ulp off moves a need that sits on an integer)."""
    best, best_it, iters, it = 0, -1, max_iters, 0
    while it < iters:
        c = int(counts[it])
        if c > best:
            best, best_it = c, it
            w = c / n
            w2 = w * w
            w4 = w2 * w2
            q = 1.0 - w4 * w4
            q = max(q, 1e-300)
            if q < 1.0:   # q == 1 (tiny consensus): log q = 0, no bound
                need = math.log(1.0 - confidence) / math.log(q) * need_scale
                if 0.0 < need < iters:
                    iters = max(math.ceil(need), it + 1)
        it += 1
    return (best_it if best >= 8 else -1), best, iters


# ---- whole RANSAC ---------------------------------------------------------------------------------------------------
def hyp_margin(sv):
    """Relative error margin (of thr2) for decisions of the F under test, from the conditioning sigma8 / sigma1 of the
    reference's 8-point system.  None: too ill-conditioned to predict that F at all."""
    cond = sv[7] / sv[0] if sv[0] > 0 else 0.0
    if cond < 1e-6:
        return None
    return min(1e-3, 1e-9 / cond)


def ransac(p1, p2, thr, confidence=0.99, max_iters=1000, seed=0x5EED5EED, refit_margin=1e-6):
    """Reference RANSAC.  Returns a dict:
    mask (None below 7 matches), best_it, best_count, decided (the count intervals fix the winner and the refit
    choice), unsure (bool per match: its final decision lies inside the margin), sure / possible per-hypothesis
    counts of every hypothesis evaluated."""
    p1 = np.asarray(p1, np.float32)
    p2 = np.asarray(p2, np.float32)
    n = len(p1)
    out = {"mask": None, "best_it": -1, "best_count": 0, "decided": True, "unsure": np.zeros(n, bool),
           "sure": [], "possible": []}
    if n < 7:
        return out
    if n == 7:
        out["mask"] = np.ones(7, bool)
        return out
    x1, y1, x2, y2 = (p1[:, 0].astype(np.float64), p1[:, 1].astype(np.float64), p2[:, 0].astype(np.float64),
                      p2[:, 1].astype(np.float64))
    thr2 = thr * thr
    sure, poss, errs = [], [], []

    def interval(it):
        while len(sure) <= it:
            (F, _, _, _, sv), _ = hypothesis(x1, y1, x2, y2, seed, len(sure))
            mg = hyp_margin(sv)
            if mg is None:
                sure.append(0)
                poss.append(n)
                errs.append(None)
                continue
            e = epipolar_error(F, x1, y1, x2, y2)
            s, p = intervals(e, thr2, mg)
            sure.append(int(s.sum()))
            poss.append(int(p.sum()))
            errs.append((e, mg))
        return sure[it], poss[it]

    class Lazy:
        def __init__(self, pick):
            self.pick = pick

        def __getitem__(self, it):
            return interval(it)[self.pick]

    lo = replay(Lazy(0), n, max_iters, confidence)
    hi = replay(Lazy(1), n, max_iters, confidence)
    top = max(lo[2], hi[2])
    for it in range(top):
        interval(it)
    decided = lo[:2] == hi[:2] and all(sure[i] == poss[i] for i in range(top))
    out.update(best_it=lo[0], best_count=lo[1], decided=decided, sure=sure[:top], possible=poss[:top])
    if lo[0] < 0:
        out["mask"] = np.zeros(n, bool)
        return out
    e, mg = errs[lo[0]]
    m1s, m1p = intervals(e, thr2, mg)
    unsure = m1s != m1p
    mask = m1s.copy()
    cons = np.flatnonzero(m1s)
    F2 = fit(x1[cons], y1[cons], x2[cons], y2[cons])[0]
    e2 = epipolar_error(F2, x1, y1, x2, y2)
    m2s, m2p = intervals(e2, thr2, refit_margin)
    if m2s.sum() >= m1p.sum():
        mask = m2s
        unsure = m2s != m2p
    elif m2p.sum() >= m1s.sum():   # the refit choice itself lies inside the margin
        out["decided"] = False
        unsure |= m2s != m2p
        unsure |= m1s != m2s
    out["mask"] = mask
    out["unsure"] = unsure
    return out
