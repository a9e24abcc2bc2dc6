"""An independent reference of the map alignment in numpy (np.longdouble by default): Umeyama's similarity through np.linalg.svd with the
diag(1, 1, det) correction, its own error and inlier evaluation, its own pose and point transform.  It shares no code with
csrc/msfm_align.h and does not replay the sampler: the test scenes make the consensus set unique instead.  Test infrastructure only."""
import numpy as np

LD = np.longdouble


def umeyama(C, p, dtype=LD):
    """the similarity (s, Q, d) with p ~ s Q C + d in the least-squares sense (Umeyama 1991).  Means, covariance, s and d are formed in
    `dtype`; np.linalg.svd has no long-double form, so the 3 x 3 covariance is rounded to float64 for the decomposition alone (Q is
    then orthogonal to float64's precision and optimal to that of a 3 x 3 SVD, about 1e-16)."""
    C, p = np.asarray(C, dtype), np.asarray(p, dtype)
    mc, mp = C.mean(0), p.mean(0)
    dc, dp = C - mc, p - mp
    M = dp.T @ dc                               # sum (p - mp)(C - mc)^T
    va = (dc * dc).sum()
    U, S, Vt = np.linalg.svd(np.asarray(M, np.float64))
    D = np.diag([1.0, 1.0, float(np.sign(np.linalg.det(U) * np.linalg.det(Vt)))])
    Q = np.asarray(U @ D @ Vt, dtype)
    s = np.trace(Q.T @ M) / va
    d = mp - s * (Q @ mc)
    return s, Q, d


def errors(s, Q, d, C, p, dtype=LD):
    C, p = np.asarray(C, dtype), np.asarray(p, dtype)
    r = p - (s * (C @ np.asarray(Q, dtype).T) + np.asarray(d, dtype))
    return np.sqrt((r * r).sum(1))


def centre(R, t, dtype=LD):
    return -(np.asarray(R, dtype).reshape(3, 3).T @ np.asarray(t, dtype))


def transform_pose(s, Q, d, R, t, dtype=LD):
    """R' = R Q^T, t' = s t - R' d"""
    Rn = np.asarray(R, dtype).reshape(3, 3) @ np.asarray(Q, dtype).T
    return Rn, dtype(s) * np.asarray(t, dtype) - Rn @ np.asarray(d, dtype)


def transform_points(s, Q, d, X, dtype=LD):
    return dtype(s) * (np.asarray(X, dtype) @ np.asarray(Q, dtype).T) + np.asarray(d, dtype)


def inverse(s, Q, d, dtype=LD):
    """the similarity that undoes (s, Q, d)"""
    Q = np.asarray(Q, dtype)
    return 1 / dtype(s), Q.T, -(Q.T @ np.asarray(d, dtype)) / dtype(s)


def reprojection(R, t, X, f, uw, dtype=LD):
    """pixel error of the normalised observation uw under (R, t) at X"""
    Y = np.asarray(R, dtype).reshape(3, 3) @ np.asarray(X, dtype) + np.asarray(t, dtype)
    return np.sqrt(((Y[:2] / Y[2] - np.asarray(uw, dtype)) ** 2).sum()) * dtype(f)


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
