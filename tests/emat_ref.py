"""Independent float64 reference of the calibrated verification (csrc/msfm_emat.h): the device and the host twin share that
header, so only a second derivation can see a wrong formula in it.  Nothing here follows the header's route:

  undistortion   Newton's method on the forward Brown model, to 1e-15
  null space     numpy SVD
  constraints    generic polynomial arithmetic (coefficient tensors indexed by exponents, products by convolution)
  roots          Stewenius' action matrix of multiplication by x in the grevlex basis, numpy.linalg.eig
  stopping rule  the sequential loop with math.log
"""
import math

import numpy as np

M64 = (1 << 64) - 1


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample5(seed, it, n):
    idx = []
    for k in range(5):
        c = 0
        attempt = 0
        while True:
            c = mix64(seed ^ mix64(((it << 20) ^ (k << 8) ^ attempt) & M64)) % n if attempt < 32 else (c + 1) % n
            if c not in idx:
                break
            attempt += 1
        idx.append(c)
    return idx


def distort(cam, x, y):
    fx, fy, cx, cy, k1, k2, p1, p2 = cam
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 * r2
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return xd, yd


def undistort(cam, u, v):
    """Pixel -> normalised undistorted coordinates: Newton on distort(x, y) = ((u - cx) / fx, (v - cy) / fy)."""
    fx, fy, cx, cy, k1, k2, p1, p2 = cam
    xd, yd = (u - cx) / fx, (v - cy) / fy
    x, y = xd, yd
    for _ in range(100):
        fxv, fyv = distort(cam, x, y)
        rx, ry = fxv - xd, fyv - yd
        h = 1e-7
        a, c = [(q - p) / h for q, p in zip(distort(cam, x + h, y), (fxv, fyv))]
        b, d = [(q - p) / h for q, p in zip(distort(cam, x, y + h), (fxv, fyv))]
        det = a * d - b * c
        dx, dy = (d * rx - b * ry) / det, (-c * rx + a * ry) / det
        x, y = x - dx, y - dy
        if abs(dx) + abs(dy) < 1e-16 * (1 + abs(x) + abs(y)):
            break
    return x, y


def sampson(E, x1, y1, x2, y2):
    a = E @ np.array([x1, y1, 1.0])
    b = E.T @ np.array([x2, y2, 1.0])
    num = x2 * a[0] + y2 * a[1] + a[2]
    return num * num / (a[0] ** 2 + a[1] ** 2 + b[0] ** 2 + b[1] ** 2)


# ---- polynomials in x, y, z of degree <= 3: coefficient tensors P[a, b, c] of x^a y^b z^c
def pmul(P, Q):
    R = np.zeros((4, 4, 4))
    for a, b, c in zip(*np.nonzero(P)):
        for d, e, f in zip(*np.nonzero(Q)):
            if a + d < 4 and b + e < 4 and c + f < 4:
                R[a + d, b + e, c + f] += P[a, b, c] * Q[d, e, f]
    return R


GREVLEX = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
           (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def constraints(basis):
    """The 10 x 20 coefficient matrix (GREVLEX columns) of det E = 0 and 2 E E^T E - tr(E E^T) E = 0 for
    E = x X + y Y + z Z + W, basis = (X, Y, Z, W) as 3 x 3 arrays."""
    E = [[np.zeros((4, 4, 4)) for _ in range(3)] for _ in range(3)]
    for i in range(3):
        for j in range(3):
            E[i][j][1, 0, 0] = basis[0][i, j]
            E[i][j][0, 1, 0] = basis[1][i, j]
            E[i][j][0, 0, 1] = basis[2][i, j]
            E[i][j][0, 0, 0] = basis[3][i, j]
    det = (pmul(E[0][0], pmul(E[1][1], E[2][2]) - pmul(E[1][2], E[2][1]))
           - pmul(E[0][1], pmul(E[1][0], E[2][2]) - pmul(E[1][2], E[2][0]))
           + pmul(E[0][2], pmul(E[1][0], E[2][1]) - pmul(E[1][1], E[2][0])))
    EEt = [[sum(pmul(E[i][k], E[j][k]) for k in range(3)) for j in range(3)] for i in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    rows = [det]
    for i in range(3):
        for j in range(3):
            rows.append(2 * sum(pmul(EEt[i][k], E[k][j]) for k in range(3)) - pmul(tr, E[i][j]))
    return np.array([[r[m] for m in GREVLEX] for r in rows])


def five_point(q1, q2):
    """All real essential matrices (unit Frobenius norm) of 5 correspondences in normalised coordinates, with the z of each
    (E = x X + y Y + z Z + W over the SVD null basis -- not the header's basis: compare E, not z), and the complex
    eigenvalues for conditioning checks."""
    A = np.array([[b[0] * a[0], b[0] * a[1], b[0], b[1] * a[0], b[1] * a[1], b[1], a[0], a[1], 1.0] for a, b in zip(q1, q2)])
    _, _, Vt = np.linalg.svd(A)
    basis = [Vt[5 + k].reshape(3, 3) for k in range(4)]
    C = constraints(basis)
    B = np.linalg.solve(C[:, :10], C[:, 10:])
    # action matrix of multiplication by x on the basis x2 xy xz y2 yz z2 x y z 1
    M = np.zeros((10, 10))
    M[:6] = -B[:6]
    M[6, 0] = M[7, 1] = M[8, 2] = M[9, 6] = 1.0
    w, V = np.linalg.eig(M)
    sols = []
    for k in range(10):
        v = V[:, k]
        if abs(v[9]) == 0:
            continue
        x, y, z = v[6] / v[9], v[7] / v[9], v[8] / v[9]
        if abs(w[k].imag) > 1e-9 * (1 + abs(w[k])) or abs(z.imag) > 1e-9 * (1 + abs(z)):
            continue
        x, y, z = x.real, y.real, z.real
        E = x * basis[0] + y * basis[1] + z * basis[2] + basis[3]
        sols.append(E / np.linalg.norm(E))
    return sols, w


def essential_from_pose(R, t):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R


def replay(counts, n, max_iters, confidence, sample=5):
    """The sequential loop's adaptive stopping rule (math.log): (winner or -1, best count, iterations run)."""
    best, best_it, iters, it = 0, -1, max_iters, 0
    while it < iters:
        c = counts[it]
        if c > best:
            best, best_it = c, it
            w = c / n
            q = max(1.0 - w ** sample, 1e-300)
            if q < 1.0:
                need = math.log(1 - confidence) / math.log(q)
                if 0 < need < iters:
                    iters = max(math.ceil(need), it + 1)
        it += 1
    return (best_it if best >= sample else -1), best, iters


def scorer(cam, p1, p2, threshold=3.0, seed=0x5EED5EED):
    """Hypothesis it of the calibrated RANSAC on pixel points p1, p2: score(it) -> (count, mask) of its best solution (the first
    among equal counts; 0 and None when the sample has no solution)."""
    n = len(p1)
    q1 = np.array([undistort(cam, float(u), float(v)) for u, v in p1])
    q2 = np.array([undistort(cam, float(u), float(v)) for u, v in p2])
    thr2 = (threshold / ((cam[0] + cam[1]) / 2)) ** 2

    def score(it):
        idx = sample5(seed, it, n)
        sols, _ = five_point(q1[idx], q2[idx])
        best, bm = 0, None
        for E in sols:
            m = np.array([sampson(E, *q1[i], *q2[i]) <= thr2 for i in range(n)])
            if bm is None or m.sum() > best:
                best, bm = int(m.sum()), m
        return best, bm
    return score


def ransac(cam, p1, p2, threshold=3.0, confidence=0.99, max_iters=1000, seed=0x5EED5EED):
    """The whole calibrated RANSAC as a literal loop over this module's pieces: the mask (None: nothing kept)."""
    n = len(p1)
    if n < 5:
        return None
    score = scorer(cam, p1, p2, threshold, seed)

    best, best_it, best_mask, iters, it = 0, -1, None, max_iters, 0
    while it < iters:
        c, m = score(it)
        if c > best:
            best, best_it, best_mask = c, it, m
            q = max(1.0 - (c / n) ** 5, 1e-300)
            if q < 1.0:
                need = math.log(1 - confidence) / math.log(q)
                if 0 < need < iters:
                    iters = max(math.ceil(need), it + 1)
        it += 1
    if best < 5:
        return None
    return best_mask.astype(np.uint8)
