"""An independent fp64 reference of the two-view geometry (csrc/msfm_pose.h): what the reference's Initializer does after its model
choice (src/Reconstruction/Initializer.cpp:300-420) with numpy's own tools -- np.linalg.svd for the decomposition of E and for the
DLT, math.acos, a sort for the median, plain sums.  Every function takes `dtype`: np.float64 is the reference, np.longdouble the same
arithmetic in extended precision (the SVDs by a longdouble refinement of the fp64 ones), which measures the reference's own rounding
scatter for the tests' bounds.

Candidate order (msfm_pose.h): (Ra, +t), (Ra, -t), (Rb, +t), (Rb, -t); Ra the rotation with the larger trace, +t the sign whose
component of largest magnitude is positive."""
import math

import numpy as np

EPS = np.finfo(np.float64).eps
W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def _null_refine(A, x, dtype):
    """The right singular vector of the smallest singular value of A, refined in `dtype` from the fp64 one x by inverse iteration
    on A^T A (a no-op in fp64)."""
    if dtype is np.float64:
        return x
    A = A.astype(dtype)
    x = x.astype(dtype)
    M = A.T @ A
    for _ in range(4):
        s = x @ M @ x
        y = _solve(M - (s - dtype(1e-7) * (np.trace(M) + dtype(1e-300))) * np.eye(len(x), dtype=dtype), x)
        x = y / np.sqrt(y @ y)
    return x


def _solve(M, b):
    """Gaussian elimination with partial pivoting in the arrays' own dtype (np.linalg.solve has no longdouble)."""
    M = M.copy()
    b = b.copy()
    n = len(b)
    return _eliminate(M, b, n)


def _eliminate(M, b, n):
    with np.errstate(all="ignore"):   # (an exactly singular shifted matrix gives a non-finite step; the callers' measurements skip it)
        return _eliminate_checked(M, b, n)


def _eliminate_checked(M, b, n):
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if p != c:
            M[[c, p]] = M[[p, c]]
            b[[c, p]] = b[[p, c]]
        for r in range(c + 1, n):
            f = M[r, c] / M[c, c]
            M[r, c:] -= f * M[c, c:]
            b[r] -= f * b[c]
    x = np.zeros_like(b)
    for c in range(n - 1, -1, -1):
        x[c] = (b[c] - M[c, c + 1:] @ x[c + 1:]) / M[c, c]
    return x


def decompose(E, dtype=np.float64):
    """-> the four (R, t) candidates in the stated order, or None."""
    E = np.asarray(E, np.float64)
    if not np.all(np.isfinite(E)):
        return None
    U, s, Vt = np.linalg.svd(E)
    if not s[1] > 0:
        return None
    if dtype is not np.float64:
        # t: the left null vector of E, v3: the right one, refined; the in-plane vectors re-orthogonalised against them in longdouble
        t3 = _null_refine(E.T, U[:, 2], dtype)
        v3 = _null_refine(E, Vt[2], dtype)
        Ed = E.astype(dtype)
        v1 = Vt[0].astype(dtype)
        v1 = v1 - (v1 @ v3) * v3
        v1 /= np.sqrt(v1 @ v1)
        v2 = np.cross(v3, v1)
        # nearest essential matrix in longdouble: u_k = E v_k / |E v_k| made orthonormal, keeping U S V^T's polar structure
        a1, a2 = Ed @ v1, Ed @ v2
        # (E restricted to the plane is s1 u1 v1^T + s2 u2 v2^T with s1 ~ s2: its orthogonal polar factor)
        M = np.stack([a1, a2], 1)                     # 3 x 2
        G = M.T @ M
        # inverse square root of the 2 x 2 SPD G in closed form
        tr, det = G[0, 0] + G[1, 1], G[0, 0] * G[1, 1] - G[0, 1] * G[1, 0]
        sdet = np.sqrt(det)
        root = (G + sdet * np.eye(2, dtype=dtype)) / np.sqrt(tr + 2 * sdet)
        inv = np.array([[root[1, 1], -root[0, 1]], [-root[1, 0], root[0, 0]]], dtype=dtype) / (root[0, 0] * root[1, 1] - root[0, 1] * root[1, 0])
        Q = M @ inv                                   # orthonormal columns u1, u2 (for the basis v1, v2)
        u1, u2 = Q[:, 0], Q[:, 1]
        u3 = np.cross(u1, u2)
        if u3 @ t3 < 0:
            t3 = -t3
        U = np.stack([u1, u2, t3], 1)
        V = np.stack([v1, v2, np.cross(v1, v2)], 1)
        Wd = W.astype(dtype)
        R1, R2, t = U @ Wd @ V.T, U @ Wd.T @ V.T, t3
    else:
        if np.linalg.det(U) < 0:
            U = -U
        if np.linalg.det(Vt) < 0:
            Vt = -Vt
        R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    Ra, Rb = (R1, R2) if np.trace(R1) >= np.trace(R2) else (R2, R1)
    if t[int(np.argmax(np.abs(t)))] < 0:
        t = -t
    return [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]


def triangulate(R, t, x1, y1, x2, y2, dtype=np.float64):
    """The reference's DLT (Initializer.cpp:436-463) for P1 = [I | 0], P2 = [R | t]; None when not triangulated."""
    P1 = np.eye(3, 4)
    P2 = np.c_[np.asarray(R, np.float64), np.asarray(t, np.float64)]
    A = np.stack([x1 * P1[2] - P1[0], y1 * P1[2] - P1[1], x2 * P2[2] - P2[0], y2 * P2[2] - P2[1]])
    h = np.linalg.svd(A)[2][3]
    if dtype is not np.float64:
        Pd = np.c_[np.asarray(R, dtype), np.asarray(t, dtype)]
        I = np.eye(3, 4).astype(dtype)
        Ad = np.stack([dtype(x1) * I[2] - I[0], dtype(y1) * I[2] - I[1], dtype(x2) * Pd[2] - Pd[0], dtype(y2) * Pd[2] - Pd[1]])
        h = _null_refine_general(Ad, h.astype(dtype), dtype)
    if h[3] == 0:
        return None
    X = h[:3] / h[3]
    return X if np.all(np.isfinite(X.astype(np.float64))) else None


def _null_refine_general(A, x, dtype):
    M = A.T @ A
    for _ in range(4):
        s = x @ M @ x
        y = _solve(M - (s * (1 - dtype(1e-6))) * np.eye(4, dtype=dtype), x)
        if not np.all(np.isfinite(y)):
            # near-exact data (s ~ 0): the matrix shifted that closely is singular to working precision.  The step again with the
            # shift a safe distance below s (still 1e-12 of the other singular values: one step converges)
            y = _solve(M - (s - dtype(1e-12) * np.trace(M)) * np.eye(4, dtype=dtype), x)
        x = y / np.sqrt(y @ y)
    return x


def evaluate(R, t, f, x1, y1, x2, y2, dtype=np.float64):
    """-> (positive depth, error in pixels, angle in degrees, depths (z1, z2)) of one kept match under (R, t)."""
    X = triangulate(R, t, x1, y1, x2, y2, dtype)
    if X is None:
        return False, math.inf, 0.0, (0.0, 0.0)
    R = np.asarray(R, dtype)
    t = np.asarray(t, dtype)
    Y = R @ X + t
    depth = bool(X[2] > EPS and Y[2] > EPS)
    with np.errstate(all="ignore"):
        e1 = np.sqrt((X[0] / X[2] - dtype(x1)) ** 2 + (X[1] / X[2] - dtype(y1)) ** 2)
        e2 = np.sqrt((Y[0] / Y[2] - dtype(x2)) ** 2 + (Y[1] / Y[2] - dtype(y2)) ** 2)
        err = (e1 + e2) / 2 * dtype(f)
        O2 = -R.T @ t
        b = np.sqrt(O2 @ O2)
        r1 = np.sqrt(X @ X)
        r2 = np.sqrt((X - O2) @ (X - O2))
        c = (r1 * r1 + r2 * r2 - b * b) / (2 * r1 * r2)
    if dtype is np.float64:
        a = abs(math.acos(c)) if -1.0 <= c <= 1.0 else math.nan
        pi = math.pi
    else:
        a = abs(np.arccos(c))
        pi = np.arccos(dtype(-1))
    ang = 0.0 if a != a else min(a, pi - a) * 180 / pi
    return depth, err, ang, (X[2], Y[2])


def median(values):
    """The reference's median (Initializer.cpp:382-397): the middle entry, or the mean of the two middle ones."""
    v = sorted(values)
    n = len(v)
    return v[n // 2] if n % 2 == 1 else (v[(n - 1) // 2] + v[n // 2]) / 2


def record(E, q1, q2, f, min_num_inliers=100, tri_max_error=2.0, tri_min_angle=4.0, dtype=np.float64):
    """The whole record of one pair: E the winner, q1 / q2 (n x 2) the kept matches in normalised coordinates.  -> dict, with
    "per_match": [(depth, err, angle, (z1, z2))] under the winner and "counts": the four cheirality counts; valid = 0 and no more
    when there is no decomposition or no candidate with a match in front of both cameras."""
    cands = decompose(E, dtype) if len(q1) else None
    if cands is None:
        return {"valid": 0}
    per = [[evaluate(R, t, f, *a, *b, dtype=dtype) for a, b in zip(q1, q2)] for R, t in cands]
    counts = [sum(1 for m in p if m[0]) for p in per]
    w = int(np.argmax(counts))
    if counts[w] == 0:
        return {"valid": 0, "counts": counts}
    R, t = cands[w]
    tri = [m for m in per[w] if m[0] and m[1] < tri_max_error]
    n_tri = len(tri)
    zero = dtype(0)
    mean_res = sum((m[1] for m in tri), zero) / n_tri if n_tri else zero
    mean_ang = sum((m[2] for m in tri), zero) / n_tri if n_tri else zero
    med = median([m[2] for m in per[w]])
    return {"valid": 1, "winner": w, "R": R, "t": t, "n_kept": len(q1), "n_positive_depth": counts[w], "n_triangulated": n_tri,
            "median_tri_angle": med, "mean_tri_angle": mean_ang, "mean_residual": mean_res, "counts": counts, "per_match": per[w],
            "per_candidate": per,
            "is_initial_candidate": int(n_tri >= min_num_inliers and med >= tri_min_angle and mean_ang >= tri_min_angle and
                                        mean_res <= tri_max_error)}
