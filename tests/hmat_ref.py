"""An independent numpy fp64 reference for the homography verification (csrc/msfm_hmat.h), written from the textbook / OpenCV
descriptions, not from the header: the DLT null vector by np.linalg.svd of the unnormalised 8 x 9 system, OpenCV's subset rule
(orientation signs of the four triples by np.linalg.det, collinearity as a small angle), findHomography's one-sided reprojection
error, the counter-based sample stream, and the sequential adaptive RANSAC loop."""
import numpy as np

MASK64 = (1 << 64) - 1
TRIPLES = ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3))


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def sample4(seed, it, n):
    """4 distinct indices: draw k, attempt a = mix64(seed ^ mix64(it << 20 ^ k << 8 ^ a)) % n for a < 32, then linear probing."""
    idx = []
    for k in range(4):
        c = 0
        attempt = 0
        while True:
            c = mix64(seed ^ mix64(((it << 20) ^ (k << 8) ^ attempt) & MASK64)) % n if attempt < 32 else (c + 1) % n
            if c not in idx:
                break
            attempt += 1
        idx.append(int(c))
    return idx


def hartley(p):
    """3 x 3 similarity taking the points' centroid to 0 and their mean distance from it to sqrt(2)."""
    p = np.asarray(p, np.float64)
    c = p.mean(0)
    s = np.sqrt(2.0) / np.linalg.norm(p - c, axis=1).mean()
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def dlt(p1, p2):
    """The homography of 4 (or more) correspondences: Hartley-normalised DLT, right singular vector of the smallest singular value,
    denormalised, unit norm, the entry of largest magnitude positive."""
    T1, T2 = hartley(p1), hartley(p2)
    q1 = np.c_[np.asarray(p1, np.float64), np.ones(len(p1))] @ T1.T
    q2 = np.c_[np.asarray(p2, np.float64), np.ones(len(p2))] @ T2.T
    A = []
    for (x, y, _), (u, v, _) in zip(q1, q2):
        A.append([x, y, 1, 0, 0, 0, -u * x, -u * y, -u])
        A.append([0, 0, 0, x, y, 1, -v * x, -v * y, -v])
    h = np.linalg.svd(np.asarray(A, np.float64))[2][-1]
    return canonical(np.linalg.inv(T2) @ h.reshape(3, 3) @ T1)


def canonical(h):
    h = np.asarray(h, np.float64).ravel()
    h = h / np.linalg.norm(h)
    return h if h[np.argmax(np.abs(h))] > 0 else -h


def collinear(a, b, c, tol=1e-6):
    u, v = np.subtract(b, a), np.subtract(c, a)
    nu, nv = np.linalg.norm(u), np.linalg.norm(v)
    return nu == 0 or nv == 0 or abs(u[0] * v[1] - u[1] * v[0]) <= tol * nu * nv


def subset_ok(p1, p2):
    """OpenCV's checkSubset for homographies: the orientation of each triple flips in all four or in none; no collinear triple."""
    negative = 0
    for t in TRIPLES:
        if collinear(*[p1[i] for i in t]) or collinear(*[p2[i] for i in t]):
            return False
        d1 = np.linalg.det(np.c_[np.asarray([p1[i] for i in t], np.float64), np.ones(3)])
        d2 = np.linalg.det(np.c_[np.asarray([p2[i] for i in t], np.float64), np.ones(3)])
        negative += d1 * d2 < 0
    return negative in (0, 4)


def reproj_error(H, x, y, u, v):
    H = np.asarray(H, np.float64).reshape(3, 3)
    w = H[2, 0] * x + H[2, 1] * y + H[2, 2]
    if w == 0 or not np.isfinite(w):
        return np.inf
    return ((H[0, 0] * x + H[0, 1] * y + H[0, 2]) / w - u) ** 2 + ((H[1, 0] * x + H[1, 1] * y + H[1, 2]) / w - v) ** 2


def sequential_replay(counts, n, max_iters, confidence, sample=4):
    """The literal sequential loop over precomputed counts -> (best index or -1, best count)."""
    best, best_it, iters, it = 0, -1, max_iters, 0
    while it < iters:
        c = counts[it]
        if c > best:
            best, best_it = c, it
            q = max(1.0 - (c / n) ** sample, 1e-300)
            need = np.log(1.0 - confidence) / np.log(q)
            if 0 < need < iters:
                iters = max(int(np.ceil(need)), it + 1)
        it += 1
    return (best_it if best >= sample else -1), best


def counter(p1, p2, threshold=3.0, seed=0x5EED5EED):
    """Hypothesis it of the RANSAC on pixel points p1, p2: count(it) -> (inliers, H), (0, None) for a rejected sample."""
    p1 = np.asarray(p1, np.float64)
    p2 = np.asarray(p2, np.float64)
    n = len(p1)
    thr2 = threshold * threshold

    def count(it):
        idx = sample4(seed, it, n)
        if not subset_ok(p1[idx], p2[idx]):
            return 0, None
        H = dlt(p1[idx], p2[idx])
        return sum(reproj_error(H, *p1[i], *p2[i]) <= thr2 for i in range(n)), H
    return count


def ransac_mask(p1, p2, threshold=3.0, confidence=0.99, max_iters=1000, seed=0x5EED5EED):
    """The whole RANSAC in numpy (no subset shortcut): a mask of n entries, or None when nothing is kept."""
    p1 = np.asarray(p1, np.float64)
    p2 = np.asarray(p2, np.float64)
    n = len(p1)
    if n < 4:
        return None
    thr2 = threshold * threshold
    count = counter(p1, p2, threshold, seed)

    counts = {}

    class Lazy:
        def __getitem__(self, it):
            counts[it] = count(it)
            return counts[it][0]
    bi, bc = sequential_replay(Lazy(), n, max_iters, confidence)
    if bi < 0:
        return None
    H = counts[bi][1]
    return np.array([reproj_error(H, *p1[i], *p2[i]) <= thr2 for i in range(n)])
