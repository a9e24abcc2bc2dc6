"""An independent reference of the two-view pose refinement (csrc/msfm_pose_refine.h) in numpy: its own Sampson residual, its own
analytic Jacobian by the chain rule through dr/dE (checked against central differences here, in long double), its own
Levenberg-Marquardt with the stated rules, the statistics by tests/pose_ref.py.  Every function takes `dtype`: np.longdouble is the
reference, np.float64 the same arithmetic in double, which measures the reference's own rounding scatter for the tests' bounds.
Sums are plain sums: the stated order of the twin is a matter of bits, not of the definition."""
import numpy as np

import pose_ref

ELIGIBLE, STEP_ACCEPTED, REFINED = 1, 2, 4
STOP_NONE, STOP_STEP, STOP_MAX_ITERS, STOP_CEILING = 0, 1, 2, 3
LAMBDA0, LAMBDA_FLOOR, LAMBDA_CEILING = 1e-3, 1e-12, 1e4


def skew(v):
    return np.array([[0 * v[0], -v[2], v[1]], [v[2], 0 * v[0], -v[0]], [-v[1], v[0], 0 * v[0]]], dtype=v.dtype)


def homogeneous(q, dtype):
    q = np.asarray(q, dtype).reshape(-1, 2)
    return np.c_[q, np.ones(len(q), dtype)]


def residuals(R, t, f, q1, q2, dtype=np.longdouble):
    """r_i = f x2^T E x1 / sqrt((E x1)_0^2 + (E x1)_1^2 + (E^T x2)_0^2 + (E^T x2)_1^2), E = [t]x R"""
    E = skew(np.asarray(t, dtype)) @ np.asarray(R, dtype).reshape(3, 3)
    x1, x2 = homogeneous(q1, dtype), homogeneous(q2, dtype)
    a, b = x1 @ E.T, x2 @ E
    num = np.sum(x2 * a, 1)
    den = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
    with np.errstate(all="ignore"):
        return dtype(f) * num / np.sqrt(den)


def cayley(a):
    aa = a @ a
    return ((1 - aa) * np.eye(3, dtype=a.dtype) + 2 * np.outer(a, a) + 2 * skew(a)) / (1 + aa)


def basis(t):
    """-> B (3 x 2): e the axis of the smallest |t_k| (the first among equal ones), b1 = t x e normalised, b2 = t x b1"""
    e = np.zeros(3, t.dtype)
    e[int(np.argmin(np.abs(t)))] = 1
    b1 = np.cross(t, e)
    b1 = b1 / np.sqrt(b1 @ b1)
    return np.stack([b1, np.cross(t, b1)], 1)


def update(R, t, delta, dtype=np.longdouble):
    R, t, delta = np.asarray(R, dtype).reshape(3, 3), np.asarray(t, dtype), np.asarray(delta, dtype)
    u = t + basis(t) @ delta[3:]
    return cayley(delta[:3]) @ R, u / np.sqrt(u @ u)


def jacobian(R, t, f, q1, q2, dtype=np.longdouble):
    """-> J (n x 5) at (a, b) = 0: dr/dE (n x 3 x 3) contracted with dE/da_k = 2 [t]x [e_k]x R and dE/db_j = [b_j]x R"""
    R, t = np.asarray(R, dtype).reshape(3, 3), np.asarray(t, dtype)
    E = skew(t) @ R
    x1, x2 = homogeneous(q1, dtype), homogeneous(q2, dtype)
    a, b = x1 @ E.T, x2 @ E
    num = np.sum(x2 * a, 1)
    den = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
    dnum = x2[:, :, None] * x1[:, None, :]
    dden = np.zeros_like(dnum)
    dden[:, :2, :] += 2 * a[:, :2, None] * x1[:, None, :]
    dden[:, :, :2] += 2 * x2[:, :, None] * b[:, None, :2]
    dr = dtype(f) * (dnum / np.sqrt(den)[:, None, None] - (num / (2 * den ** dtype(1.5)))[:, None, None] * dden)
    eye = np.eye(3, dtype=dtype)
    B = basis(t)
    dE = [2 * skew(t) @ skew(eye[k]) @ R for k in range(3)] + [skew(B[:, j]) @ R for j in range(2)]
    return np.stack([np.sum(dr * D[None], (1, 2)) for D in dE], 1)


def jacobian_numeric(R, t, f, q1, q2, h=1e-7, dtype=np.longdouble):
    cols = []
    for k in range(5):
        d = np.zeros(5, dtype)
        d[k] = h
        cols.append((residuals(*update(R, t, d, dtype), f, q1, q2, dtype) - residuals(*update(R, t, -d, dtype), f, q1, q2, dtype)) / (2 * dtype(h)))
    return np.stack(cols, 1)


def _cholesky_solve(A, g):
    """A x = -g by Cholesky in the arrays' dtype; None when a pivot is not > 0 or x is not finite"""
    n = len(g)
    L = np.zeros_like(A)
    for k in range(n):
        d = A[k, k] - L[k, :k] @ L[k, :k]
        if not d > 0:
            return None
        L[k, k] = np.sqrt(d)
        for r in range(k + 1, n):
            L[r, k] = (A[r, k] - L[r, :k] @ L[k, :k]) / L[k, k]
    y = np.zeros_like(g)
    for k in range(n):
        y[k] = (-g[k] - L[k, :k] @ y[:k]) / L[k, k]
    x = np.zeros_like(g)
    for k in range(n - 1, -1, -1):
        x[k] = (y[k] - L[k + 1:, k] @ x[k + 1:]) / L[k, k]
    return x if np.all(np.isfinite(x.astype(np.float64))) else None


def lm(R, t, f, q1, q2, max_iters, step_tol, dtype=np.longdouble):
    """-> (R, t, trace): trace has steps, accepted, stop, cost_before, cost and the smallest margins of its decisions: cost_margin
    (|c_new - c| / c over the evaluated steps), step_margin (| |delta| - step_tol | over the accepted ones)"""
    R, t = np.asarray(R, dtype).reshape(3, 3), np.asarray(t, dtype)
    r = residuals(R, t, f, q1, q2, dtype)
    c = r @ r
    tr = dict(steps=0, accepted=0, stop=STOP_MAX_ITERS, cost_before=c, cost=c, cost_margin=np.inf, step_margin=np.inf, pivot_rejected=0)
    lam = dtype(LAMBDA0)
    fresh = False
    while tr["steps"] < max_iters:
        if not fresh:
            J = jacobian(R, t, f, q1, q2, dtype)
            r = residuals(R, t, f, q1, q2, dtype)
            H, g = J.T @ J, J.T @ r
            fresh = True
        tr["steps"] += 1
        delta = _cholesky_solve(H + lam * np.diag(np.diag(H)), g)
        accept = False
        if delta is None:
            tr["pivot_rejected"] += 1
        else:
            Rn, tn = update(R, t, delta, dtype)
            if np.all(np.isfinite(np.r_[Rn.ravel(), tn].astype(np.float64))):
                rn = residuals(Rn, tn, f, q1, q2, dtype)
                cn = rn @ rn
                if np.isfinite(np.float64(cn)):
                    tr["cost_margin"] = min(tr["cost_margin"], float(abs(cn - c) / c) if c > 0 else 0.0)
                accept = bool(np.isfinite(np.float64(cn)) and cn < c)
        if accept:
            R, t, c = Rn, tn, cn
            fresh = False
            tr["accepted"] += 1
            lam = max(lam / 10, dtype(LAMBDA_FLOOR))
            d2 = delta @ delta
            tr["step_margin"] = min(tr["step_margin"], float(abs(np.sqrt(d2) - dtype(step_tol))))
            if d2 <= dtype(step_tol) * dtype(step_tol):
                tr["stop"] = STOP_STEP
                break
        else:
            lam = lam * 10
            if lam > LAMBDA_CEILING:
                tr["stop"] = STOP_CEILING
                break
    tr["cost"] = c
    return R, t, tr


def statistics(R, t, f, q1, q2, tri_max_error, dtype=np.longdouble):
    """the record's statistics under (R, t) -> dict, with error_margin: the smallest |err - tri_max_error| of a match in front"""
    per = [pose_ref.evaluate(R, t, f, *a, *b, dtype=dtype) for a, b in zip(np.asarray(q1, np.float64), np.asarray(q2, np.float64))]
    tri = [m for m in per if m[0] and m[1] < tri_max_error]
    zero = dtype(0)
    n_tri = len(tri)
    margin = min([abs(float(m[1]) - tri_max_error) for m in per if m[0]] or [np.inf])
    depth_margin = min([min(abs(float(z)) for z in m[3]) for m in per] or [np.inf])
    return dict(n_positive_depth=sum(1 for m in per if m[0]), n_triangulated=n_tri,
                mean_residual=sum((m[1] for m in tri), zero) / n_tri if n_tri else zero,
                mean_tri_angle=sum((m[2] for m in tri), zero) / n_tri if n_tri else zero,
                median_tri_angle=pose_ref.median([m[2] for m in per]), error_margin=margin, depth_margin=depth_margin)


def refine(rec, q1, q2, f, params=(100, 2.0, 4.0), refine_params=(10, 15, 1e-6), dtype=np.longdouble):
    """rec: a two-view record (mapping with valid, R, t, n_kept, n_positive_depth, n_triangulated) -> (out, refinement): out is None
    when the record stays (not eligible, no accepted step, or a count drops), else a dict with the refined R, t and statistics;
    refinement: status, stop, steps, accepted, the two counts before, cost_before, cost_after, and the trace and margins."""
    max_iters, min_matches, step_tol = refine_params
    rf = dict(status=0, stop=STOP_NONE, steps=0, accepted=0, n_positive_depth_before=0, n_triangulated_before=0, cost_before=0.0,
              cost_after=0.0, trace=None, stats=None)
    if not rec["valid"] or rec["n_kept"] < min_matches:
        return None, rf
    R, t, tr = lm(rec["R"], rec["t"], f, q1, q2, max_iters, step_tol, dtype)
    rf.update(status=ELIGIBLE | (STEP_ACCEPTED if tr["accepted"] else 0), stop=tr["stop"], steps=tr["steps"], accepted=tr["accepted"],
              n_positive_depth_before=int(rec["n_positive_depth"]), n_triangulated_before=int(rec["n_triangulated"]),
              cost_before=tr["cost_before"], cost_after=tr["cost_before"], trace=tr)
    if not tr["accepted"]:
        return None, rf
    st = statistics(R, t, f, q1, q2, params[1], dtype)
    rf["stats"] = st
    if st["n_positive_depth"] < rec["n_positive_depth"] or st["n_triangulated"] < rec["n_triangulated"]:
        return None, rf
    rf["status"] |= REFINED
    rf["cost_after"] = tr["cost"]
    med, mean_ang, mean_res = st["median_tri_angle"], st["mean_tri_angle"], st["mean_residual"]
    out = dict(valid=1, R=R, t=t, n_kept=int(rec["n_kept"]), n_positive_depth=st["n_positive_depth"], n_triangulated=st["n_triangulated"],
               median_tri_angle=med, mean_tri_angle=mean_ang, mean_residual=mean_res,
               is_initial_candidate=int(st["n_triangulated"] >= params[0] and med >= params[2] and mean_ang >= params[2] and
                                        mean_res <= params[1]))
    return out, rf
