"""Independent reference of the point refinement (include/msfm_match.h "point refinement"), written from the
definitions in plain numpy on top of tests/triangulation_ref.py: the residuals and the Jacobian STACKED in long double (2m rows),
H = J^T J and g = J^T r as matrix products, the damped system by numpy.linalg.solve after numpy.linalg.cholesky has shown it positive
definite, errors in long double, angles by np.arccos; the same Levenberg-Marquardt and standing rules and the same trace fields as
the twin's msfm_ref::Trace.  Test infrastructure only."""
import numpy as np

import triangulation_ref as ref

REFINED, ROBUST = 64, 32
LD = np.longdouble
LAMBDA0, LAMBDA_FLOOR, LAMBDA_CEILING = 1e-3, 1e-12, 1e4
STOP_NONE, STOP_STEP, STOP_MAX_ITERS, STOP_CEILING = 0, 1, 2, 3
NOT_ELIGIBLE, NO_ACCEPTED_STEP = 1, 2
TRACE_KEYS = ("steps", "accepted", "stop", "verdict", "accepted_after_rejected", "depth_rejected")


def project(P, X):
    """P [m, 3, 4] long double, X [3] -> (x, y, depth), long double"""
    Xl = np.asarray(X, np.float64).astype(LD)
    Y = P[:, :, 0] * Xl[0] + P[:, :, 1] * Xl[1] + P[:, :, 2] * Xl[2] + P[:, :, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        return Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2], Y[:, 2]


def stacked(P, u, v, f, X):
    """-> (r [2m], J [2m, 3], depth [m]) in long double: rows (rx, ry) per observation"""
    x, y, z = project(P, X)
    r = np.empty(2 * len(u), LD)
    r[0::2], r[1::2] = (x - u) * f, (y - v) * f
    J = np.empty((2 * len(u), 3), LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        J[0::2] = (P[:, 0, :3] - x[:, None] * P[:, 2, :3]) * (f / z)[:, None]
        J[1::2] = (P[:, 1, :3] - y[:, None] * P[:, 2, :3]) * (f / z)[:, None]
    return r, J, z


def gradient_norm(obs, f, X):
    """|J^T r| at X over obs = [(u, v, P)], long double"""
    P = np.asarray([o[2] for o in obs], np.float64).astype(LD)
    u, v = np.asarray([o[0] for o in obs], LD), np.asarray([o[1] for o in obs], LD)
    r, J, _ = stacked(P, u, v, LD(f), X)
    return float(np.sqrt(((J.T @ r) ** 2).sum()))


def cost_at(obs, f, X):
    P = np.asarray([o[2] for o in obs], np.float64).astype(LD)
    u, v = np.asarray([o[0] for o in obs], LD), np.asarray([o[1] for o in obs], LD)
    r, _, _ = stacked(P, u, v, LD(f), X)
    return float((r * r).sum())


def observations(img, idx, kps, poses, cam):
    """the used observations of a track -> (element numbers, [(u, v, P)])"""
    used = [k for k in range(len(img)) if poses.get(int(img[k])) is not None]
    obs = []
    for k in used:
        R, t = poses[int(img[k])]
        P = np.c_[np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)]
        u, v = ref.observation(cam, kps[int(img[k])][int(idx[k]), :2])
        obs.append((u, v, P))
    return used, obs


def track(img, idx, kps, poses, cam, rec, mask=None, max_error=2.0, min_angle=1.5, max_iters=10, step_tol=1e-10):
    """One track.  rec: dict(status, n_views, X, mean_residual, tri_angle, residuals) as triangulation_ref.track /
    robust_triangulation_ref.track return it (not changed); mask: the robust call's bytes for the track's elements, or None.
    -> the same dict after the call, plus stands, trace (TRACE_KEYS + lambda, cost), fit (the fitting set as [(u, v, P)]), cost_before,
    and the margins of every decision taken: cost_margin (relative |c(Xn) - c| / c over the evaluated steps), step_margin (| |delta| -
    the stop radius |, absolute, over the accepted steps), depth_margin, error_margin (|err - max_error| over the fitting set at the
    verdict), angle_margin (the scanned pairs)."""
    n = len(img)
    out = dict(rec)
    out["residuals"] = np.array(rec["residuals"], np.float64)
    out["X"] = np.array(rec["X"], np.float64)
    tr = dict(steps=0, accepted=0, stop=STOP_NONE, verdict=NOT_ELIGIBLE, accepted_after_rejected=0, depth_rejected=0)
    tr["lambda"] = 0.0
    tr["cost"] = 0.0
    out.update(stands=False, trace=tr, fit=[], cost_before=0.0, cost_margin=np.inf, step_margin=np.inf, depth_margin=np.inf,
               error_margin=np.inf, angle_margin=np.inf)
    if (rec["status"] & 3) != 3:
        return out
    used, obs = observations(img, idx, kps, poses, cam)
    fit = [p for p, k in enumerate(used) if mask is None or mask[k]]
    f = (LD(cam[0]) + LD(cam[1])) / 2
    P = np.asarray([obs[p][2] for p in fit], np.float64).astype(LD)
    u, v = np.asarray([obs[p][0] for p in fit], LD), np.asarray([obs[p][1] for p in fit], LD)
    X = np.array(rec["X"], np.float64)
    r, J, z = stacked(P, u, v, f, X)
    c = float((r * r).sum())
    c0 = c
    lam, steps, accepted, stop, last_rejected = LAMBDA0, 0, 0, STOP_MAX_ITERS, False
    cm, sm, dm = [], [], []
    while steps < max_iters:
        H, g = (J.T @ J).astype(np.float64), (J.T @ r).astype(np.float64)
        steps += 1
        A = H + lam * np.diag(np.diag(H))
        delta = None
        try:
            with np.errstate(all="ignore"):
                np.linalg.cholesky(A)
                d = np.linalg.solve(A, -g)
            if np.all(np.isfinite(d)):
                delta = d
        except np.linalg.LinAlgError:
            pass
        accept = False
        if delta is not None:
            Xn = X + delta
            rn, Jn, zn = stacked(P, u, v, f, Xn)
            cn = float((rn * rn).sum())
            lower = np.isfinite(cn) and cn < c
            depth = bool(np.all(zn.astype(np.float64) > ref.EPS))
            if np.isfinite(cn) and c > 0:
                cm.append(abs(cn - c) / c)
            if lower:
                dm.append(float(np.min(np.abs(zn.astype(np.float64) - ref.EPS))))
            if lower and not depth:
                tr["depth_rejected"] += 1
            accept = bool(lower and depth)
        if accept:
            X, r, J, c = Xn, rn, Jn, cn
            accepted += 1
            tr["accepted_after_rejected"] += 1 if last_rejected else 0
            last_rejected = False
            lam = max(lam / 10.0, LAMBDA_FLOOR)
            d2, thr = float(delta @ delta), step_tol * step_tol * (float(X @ X) + step_tol)
            sm.append(abs(np.sqrt(d2) - np.sqrt(thr)))
            if d2 <= thr:
                stop = STOP_STEP
                break
        else:
            last_rejected = True
            lam = lam * 10.0
            if lam > LAMBDA_CEILING:
                stop = STOP_CEILING
                break
    tr.update(steps=steps, accepted=accepted, stop=stop, verdict=NO_ACCEPTED_STEP, cost=c)
    tr["lambda"] = lam
    out.update(fit=[obs[p] for p in fit], cost_before=c0, cost_margin=min(cm, default=np.inf), step_margin=min(sm, default=np.inf),
               depth_margin=min(dm, default=np.inf))
    if accepted == 0:
        return out
    # the verdict: every used observation's error, the tests over the fitting set
    Pa = np.asarray([o[2] for o in obs], np.float64).astype(LD)
    ua, va = np.asarray([o[0] for o in obs], LD), np.asarray([o[1] for o in obs], LD)
    x, y, za = project(Pa, X)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = (np.sqrt((x - ua) ** 2 + (y - va) ** 2) * f).astype(np.float64)
    ef, zf = e[fit], za[fit].astype(np.float64)
    bits = (ref.ERROR_OK if np.all(ef <= max_error) else 0) | (ref.DEPTH_OK if np.all(zf > ref.EPS) else 0)
    centres = [-(obs[p][2][:, :3].astype(LD).T @ obs[p][2][:, 3].astype(LD)) for p in fit]
    angle, hit, scanned = 0.0, False, []
    for a_ in range(len(fit)):
        for b_ in range(a_):
            g_ = ref.angle(X, centres[a_], centres[b_])
            scanned.append(g_)
            if g_ >= min_angle:
                angle, hit = g_, True
                break
            angle = max(angle, g_)
        if hit:
            break
    bits |= ref.ANGLE_OK if hit else 0
    cleared = rec["status"] & ~bits & (ref.ERROR_OK | ref.ANGLE_OK | ref.DEPTH_OK)
    tr["verdict"] = int(cleared)
    out.update(error_margin=float(np.min(np.abs(ef - max_error))),
               angle_margin=float(np.min(np.abs(np.asarray(scanned) - min_angle))) if scanned else np.inf)
    if cleared:
        return out
    res = out["residuals"]
    res[used] = e
    out.update(stands=True, status=3 | bits | (rec["status"] & ROBUST) | REFINED, X=X, residuals=res, tri_angle=angle,
               mean_residual=float(np.sum(np.asarray(ef, LD)) / len(fit)))
    return out


def run(tracks, kps, poses, cam, records, masks=None, max_error=2.0, min_angle=1.5, max_iters=10, step_tol=1e-10, select=None):
    """records: the list of dicts of triangulation_ref.run / robust_triangulation_ref.run (or of an earlier run()); masks: True to take
    each record's "mask" -> list of track() results"""
    offsets, img, idx = tracks[:3]
    todo = range(len(offsets) - 1) if select is None else select
    return [track(img[offsets[t]:offsets[t + 1]], idx[offsets[t]:offsets[t + 1]], kps, poses, cam, records[t],
                  records[t]["mask"] if masks else None, max_error, min_angle, max_iters, step_tol) for t in todo]
