"""Independent numpy reference of the image registration (csrc/msfm_register.h is the code under test): another elimination of the P3P
equations (depth ratios against the THIRD point, the Sylvester resultant by numpy polynomial arithmetic, numpy.roots), an SVD (Kabsch)
alignment for the pose in long double, the sequential stopping rule with math.log, a Gauss-Newton refinement to convergence with a
Rodrigues update.  It takes the sample triples from the twin's sampler (host_register_sample3): it tests the arithmetic, not the
sampler.  Test infrastructure only."""
import math

import numpy as np

LD = np.longdouble
ATTEMPTED, POSE, SUCCEEDED, REFINED = 1, 2, 4, 8
DEPTH_EPS = 2.220446049250313e-16
ROUND = 64


def undistort(cam, x, y):
    """pixel -> normalised undistorted, by Newton on the Brown model"""
    cam = tuple(cam) + (0.0,) * (8 - len(cam))
    fx, fy, cx, cy, k1, k2, p1, p2 = cam
    x0, y0 = (np.asarray(x, np.float64) - cx) / fx, (np.asarray(y, np.float64) - cy) / fy
    if not any(cam[4:]):
        return x0, y0
    u, v = x0.copy(), y0.copy()
    for _ in range(60):
        r2 = u * u + v * v
        rad = 1 + (k2 * r2 + k1) * r2
        u, v = (x0 - (2 * p1 * u * v + p2 * (r2 + 2 * u * u))) / rad, (y0 - (p1 * (r2 + 2 * v * v) + 2 * p2 * u * v)) / rad
    return u, v


def kabsch(P, Q):
    """R, t with Q ~ R P + t (rows are points), det R = +1"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    pc, qc = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((Q - qc).T @ (P - pc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return R, qc - R @ pc


def p3p(u, v, X, with_condition=False):
    """-> list of (R, t), ascending in s3 / s1 (the twin's order of roots).  with_condition: also the smallest relative gap between
    the quartic's roots that were used or rejected as real (a measure of how well-conditioned the triple is)."""
    u, v, X = np.asarray(u, LD), np.asarray(v, LD), np.asarray(X, LD).reshape(3, 3)
    j = np.stack([u, v, np.ones(3, LD)], 1)
    j = j / np.sqrt((j * j).sum(1))[:, None]
    ca, cb, cg = float(j[1] @ j[2]), float(j[0] @ j[2]), float(j[0] @ j[1])
    a2, b2, c2 = (float(((X[i] - X[k]) ** 2).sum()) for i, k in ((1, 2), (0, 2), (0, 1)))
    P = np.polynomial.Polynomial
    x = P([0.0, 1.0])
    # s1 = x s3, s2 = y s3:  F1 = a2 (x^2 + 1 - 2 x cb) - b2 (y^2 + 1 - 2 y ca),  F2 = c2 (x^2 + 1 - 2 x cb) - b2 (x^2 + y^2 - 2 x y cg)
    f2, f1, f0 = P([-b2]), P([2 * b2 * ca]), a2 * (x * x + 1 - 2 * cb * x) - b2
    g2, g1, g0 = P([-b2]), 2 * b2 * cg * x, c2 * (x * x + 1 - 2 * cb * x) - b2 * x * x
    res = (f2 * g0 - f0 * g2) ** 2 - (f2 * g1 - f1 * g2) * (f1 * g0 - f0 * g1)
    coef = res.coef
    if len(coef) < 5 or not np.all(np.isfinite(coef)) or coef[4] == 0:
        return ([], 0.0) if with_condition else []
    roots = np.roots(coef[::-1])
    gap = min([abs(roots[i] - roots[k]) / max(abs(roots[i]), 1.0) for i in range(4) for k in range(i)] + [np.inf])
    out = []
    for r in roots:
        if abs(r.imag) > 1e-9 * max(1.0, abs(r)) or r.real <= 0:
            continue
        xr = float(r.real)
        lin, con = (f1 - g1)(xr), (f0 - g0)(xr)
        if lin == 0:
            continue
        yr = -con / lin
        d = xr * xr + 1 - 2 * xr * cb
        if not (yr > 0 and d > 0):
            continue
        s3 = math.sqrt(b2 / d)
        s = np.asarray([xr * s3, yr * s3, s3], LD)
        Y = np.asarray(j * s[:, None], np.float64)
        R, t = kabsch(np.asarray(X, np.float64), Y)
        fit = np.abs(np.asarray(X, np.float64) @ R.T + t - Y).max()
        if fit > 1e-6 * max(1.0, np.abs(Y).max()):   # a spurious root of the resultant
            continue
        out.append((1.0 / xr, R, t))
    out.sort(key=lambda e: e[0])
    sols = [(R, t) for _, R, t in out]
    return (sols, float(gap)) if with_condition else sols


def errors(R, t, cu, cv, X, f):
    """-> (pixel error, in front) per correspondence"""
    Y = X @ R.T + t
    with np.errstate(all="ignore"):
        e = np.hypot(Y[:, 0] / Y[:, 2] - cu, Y[:, 1] / Y[:, 2] - cv) * f
    return e, Y[:, 2] > DEPTH_EPS


def inliers(R, t, cu, cv, X, f, max_error):
    e, front = errors(R, t, cu, cv, X, f)
    with np.errstate(invalid="ignore"):
        return front & (e <= max_error)


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def refine(R, t, cu, cv, X, iters=50, tol=1e-15):
    """Gauss-Newton on the reprojection error (normalised units) to convergence: R <- exp([w]x) R, t <- exp([w]x) t + dt"""
    R, t = np.array(R, np.float64), np.array(t, np.float64)
    for _ in range(iters):
        Y = X @ R.T + t
        iz = 1.0 / Y[:, 2]
        px, py = Y[:, 0] * iz, Y[:, 1] * iz
        r = np.concatenate([px - cu, py - cv])
        n = len(cu)
        J = np.zeros((2 * n, 6))
        z = np.zeros(n)
        dpx = np.stack([iz, z, -px * iz], 1)
        dpy = np.stack([z, iz, -py * iz], 1)
        # dY = w x Y + dt  ->  d(pi)/dw = (Y x row)
        J[:n, :3], J[n:, :3] = np.cross(Y, dpx), np.cross(Y, dpy)
        J[:n, 3:], J[n:, 3:] = dpx, dpy
        step = np.linalg.lstsq(J, -r, rcond=None)[0]
        if not np.all(np.isfinite(step)):
            break
        E = rodrigues(step[:3])
        R, t = E @ R, E @ t + step[3:]
        if np.abs(step).max() < tol:
            break
    return R, t


def replay(count_at, n, max_iters, confidence, avail=None):
    """the sequential adaptive rule -> (best iteration or -1, best count, decided)"""
    best, best_it, iters, it = 0, -1, max_iters, 0
    while it < iters:
        if avail is not None and it >= avail:
            return best_it if best >= 3 else -1, best, False
        c = count_at(it)
        if c > best:
            best, best_it = c, it
            q = max(1.0 - (c / n) ** 3, 1e-300)
            if q < 1.0:
                need = math.log(1.0 - confidence) / math.log(q)
                if 0.0 < need < iters:
                    iters = max(int(math.ceil(need)), it + 1)
        it += 1
    return best_it if best >= 3 else -1, best, True


def register(image_id, cu, cv, X, f, sample, max_error=4.0, confidence=0.9999, max_iters=1024, min_inliers=15, refine_iters=10):
    """One image.  sample(it) -> the three indices.  -> dict: status, n_inliers, hypotheses, R, t, flags, residuals, and for the margin
    assertions: margin (the smallest | error - max_error | over the scored correspondences of the winning and the final pose),
    margin_all (the same over every pose of every hypothesis the rule read),
    tie (the winning count is reached by another iteration with another pose), R0 / t0 (the unrefined winner)."""
    n = len(cu)
    out = dict(status=0, n_inliers=0, hypotheses=0, R=np.zeros((3, 3)), t=np.zeros(3), flags=np.zeros(n, bool), residuals=np.full(n, -1.0),
               margin=np.inf, margin_all=np.inf, tie=False, R0=None, t0=None)
    if n < 3 or n < min_inliers:
        return out
    out["status"] = ATTEMPTED
    cache = {}

    def hyp(it):
        if it not in cache:
            idx = sample(it)
            sols = p3p(cu[idx], cv[idx], X[idx])
            cnt = [int(inliers(R, t, cu, cv, X, f, max_error).sum()) for R, t in sols]
            for R, t in sols:
                out["margin_all"] = min(out["margin_all"], float(np.nanmin(np.abs(errors(R, t, cu, cv, X, f)[0] - max_error))))
            b = int(np.argmax(cnt)) if cnt else -1
            cache[it] = (cnt[b] if cnt else 0, sols[b] if cnt else None)
        return cache[it]

    r = 1
    while True:
        best_it, best, decided = replay(lambda it: hyp(it)[0], n, max_iters, confidence, min(r * ROUND, max_iters))
        if decided:
            break
        r += 1
    out["hypotheses"] = min(r * ROUND, max_iters)
    if best_it < 0:
        return out
    out["tie"] = any(c == best and it != best_it and not np.allclose(s[0], cache[best_it][1][0], atol=1e-6) for it, (c, s) in cache.items() if s)
    R, t = cache[best_it][1]
    out["R0"], out["t0"] = R, t
    e0, _ = errors(R, t, cu, cv, X, f)
    margin = np.abs(e0 - max_error).min()
    win = inliers(R, t, cu, cv, X, f, max_error)
    status = ATTEMPTED | POSE
    if refine_iters > 0:
        Rr, tr = refine(R, t, cu[win], cv[win], X[win])
        er, _ = errors(Rr, tr, cu, cv, X, f)
        margin = min(margin, np.abs(er - max_error).min())
        if inliers(Rr, tr, cu, cv, X, f, max_error).sum() >= win.sum():
            R, t, status = Rr, tr, status | REFINED
    e, front = errors(R, t, cu, cv, X, f)
    flags = front & (e <= max_error)
    if flags.sum() >= min_inliers:
        status |= SUCCEEDED
    out.update(status=status, n_inliers=int(flags.sum()), R=R, t=t, flags=flags, residuals=e, margin=float(margin))
    return out


def correspondences(tracks, points, image_id, kp, cam):
    """-> (track ids, cu, cv, X) of an image: the succeeded tracks with an element of the image, by ascending track number"""
    offs, img, idx = tracks[0], tracks[1], tracks[2]
    ok = (points["status"] & 14) == 14
    tid_of_elem = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    sel = np.nonzero((img == image_id) & ok[tid_of_elem])[0]
    tids = tid_of_elem[sel]
    assert len(np.unique(tids)) == len(tids)
    px = np.asarray(kp, np.float32)[idx[sel], :2].astype(np.float64)
    cu, cv = undistort(cam, px[:, 0], px[:, 1])
    return tids.astype(np.int32), cu, cv, np.asarray(points["X"][tids], np.float64)
