"""Independent reference of the pose refinement (include/msfm_match.h "pose refinement"), written from the
definitions in plain numpy on top of tests/triangulation_ref.py: the residuals and the Jacobian of the parametrisation R <- C(a) R,
t <- C(a) t + dt STACKED in long double (2n rows, pixel units), H = J^T J and g = J^T r as matrix products, the damped system by
numpy.linalg.solve after numpy.linalg.cholesky has shown it positive definite, Cayley's rotation and the errors in long double, angles
by np.arccos; the same Levenberg-Marquardt, stop and standing rules and the same trace fields as the twin's msfm_ref::Trace.  No
partial sums, no butterfly, no 27 sums.  Test infrastructure only."""
import numpy as np

import triangulation_ref as ref

REPOSED, REFINED, ROBUST = 128, 64, 32
LD = np.longdouble
LAMBDA0, LAMBDA_FLOOR, LAMBDA_CEILING = 1e-3, 1e-12, 1e4
STOP_NONE, STOP_STEP, STOP_MAX_ITERS, STOP_CEILING = 0, 1, 2, 3
NOT_ELIGIBLE, NO_ACCEPTED_STEP, LOST_INLIERS = 1, 2, 3
POSE_ATTEMPTED, POSE_REFINED, POSE_FIXED = 1, 2, 4
TRACE_KEYS = ("steps", "accepted", "stop", "verdict", "accepted_after_rejected", "depth_rejected")
SUCCEEDED = ref.ATTEMPTED | ref.POINT | ref.ERROR_OK | ref.ANGLE_OK


def stacked(R, t, u, w, X, f):
    """R [3, 3], t [3] float64; u, w [n] long double; X [n, 3] float64 -> (r [2n], J [2n, 6], depth [n], err [n]) in long double"""
    Rl, tl, Xl = np.asarray(R, np.float64).astype(LD), np.asarray(t, np.float64).astype(LD), np.asarray(X, np.float64).astype(LD)
    Y = Xl @ Rl.T + tl
    with np.errstate(invalid="ignore", divide="ignore"):
        x, y, z = Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2], Y[:, 2]
        r = np.empty(2 * len(u), LD)
        r[0::2], r[1::2] = (x - u) * f, (y - w) * f
        J = np.zeros((2 * len(u), 6), LD)
        zero = np.zeros(len(u), LD)
        px = np.stack([1 / z, zero, -x / z], 1) * f          # d rx / dY
        py = np.stack([zero, 1 / z, -y / z], 1) * f          # d ry / dY
        # dY = 2 a x Y + dt:  row . (a x Y) = a . (Y x row)
        J[0::2, :3], J[1::2, :3] = 2 * np.cross(Y, px), 2 * np.cross(Y, py)
        J[0::2, 3:], J[1::2, 3:] = px, py
        err = np.sqrt((x - u) ** 2 + (y - w) ** 2) * f
    return r, J, z, err


def cayley(a):
    a = np.asarray(a, LD)
    aa = a @ a
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], LD)
    return ((1 - aa) * np.eye(3, dtype=LD) + 2 * np.outer(a, a) + 2 * K) / (1 + aa)


def inliers(err, z, max_error):
    return int(np.sum((z.astype(np.float64) > ref.EPS) & (err.astype(np.float64) <= max_error)))


def gradient_norm(R, t, u, w, X, f):
    r, J, _, _ = stacked(R, t, u, w, X, LD(f))
    return float(np.sqrt(((J.T @ r) ** 2).sum()))


def image(R, t, u, w, X, f, max_error, max_iters=10, step_tol=1e-6):
    """One eligible image from its fitting set -> dict(R, t (the pose that stands, else the old one), stands, trace (TRACE_KEYS +
    lambda, cost), cost_before, cost_after, inliers_before, inliers_after, and the margins of every decision taken: cost_margin
    (relative |c_new - c| / c over the evaluated steps), step_margin (| |delta| - the stop radius |, over the accepted steps),
    depth_margin, error_margin (|err - max_error| over both inlier counts))."""
    f = LD(f)
    R0, t0 = np.array(R, np.float64).reshape(3, 3), np.array(t, np.float64).reshape(3)
    Rc, tc = R0.copy(), t0.copy()
    r, J, z, err0 = stacked(Rc, tc, u, w, X, f)
    c = float((r * r).sum())
    c0 = c
    lam, steps, accepted, stop, last_rejected = LAMBDA0, 0, 0, STOP_MAX_ITERS, False
    tr = dict(steps=0, accepted=0, stop=STOP_NONE, verdict=NOT_ELIGIBLE, accepted_after_rejected=0, depth_rejected=0)
    cm, sm, dm = [], [], []
    while steps < max_iters:
        H, g = (J.T @ J).astype(np.float64), (J.T @ r).astype(np.float64)
        steps += 1
        A = H + lam * np.diag(np.diag(H))
        new = None
        try:
            with np.errstate(all="ignore"):
                np.linalg.cholesky(A)
                d = np.linalg.solve(A, -g)
            if np.all(np.isfinite(d)):
                C = cayley(d[:3])
                Rn = (C @ Rc.astype(LD)).astype(np.float64)
                tn = (C @ tc.astype(LD) + d[3:].astype(LD)).astype(np.float64)
                if np.all(np.isfinite(Rn)) and np.all(np.isfinite(tn)):
                    new = (d, Rn, tn)
        except np.linalg.LinAlgError:
            pass
        accept = False
        if new is not None:
            d, Rn, tn = new
            rn, Jn, zn, errn = stacked(Rn, tn, u, w, X, f)
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
            Rc, tc, r, J, c, errc, zc = Rn, tn, rn, Jn, cn, errn, zn
            accepted += 1
            tr["accepted_after_rejected"] += 1 if last_rejected else 0
            last_rejected = False
            lam = max(lam / 10.0, LAMBDA_FLOOR)
            d2, thr = float(d @ d), step_tol * step_tol * (1.0 + float(tc @ tc))
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
    before = inliers(err0, z, max_error)
    em = [float(np.min(np.abs(err0.astype(np.float64) - max_error)))]
    after = before
    if accepted:
        after = inliers(errc, zc, max_error)
        em.append(float(np.min(np.abs(errc.astype(np.float64) - max_error))))
    stands = accepted > 0 and after >= before
    tr.update(steps=steps, accepted=accepted, stop=stop, verdict=0 if stands else (LOST_INLIERS if accepted else NO_ACCEPTED_STEP), cost=c)
    tr["lambda"] = lam
    return dict(R=Rc if stands else R0, t=tc if stands else t0, stands=stands, trace=tr, cost_before=c0, cost_after=c if stands else c0,
                inliers_before=before, inliers_after=after, cost_margin=min(cm, default=np.inf), step_margin=min(sm, default=np.inf),
                depth_margin=min(dm, default=np.inf), error_margin=min(em), last=(Rc, tc))


def fitting_set(image_id, tracks, kps, cam, records, masks):
    """-> (u, w [n] long double, X [n, 3], track numbers) of the image: its FIT observations of succeeded tracks, by track number"""
    offsets, img, idx = tracks[:3]
    u, w, X, tid = [], [], [], []
    for t in range(len(offsets) - 1):
        if (records[t]["status"] & SUCCEEDED) != SUCCEEDED:
            continue
        for e in range(int(offsets[t]), int(offsets[t + 1])):
            if int(img[e]) == image_id and (masks is None or masks[e]):
                a, b = ref.observation(cam, kps[image_id][int(idx[e]), :2])
                u.append(a)
                w.append(b)
                X.append(records[t]["X"])
                tid.append(t)
    return np.asarray(u, LD), np.asarray(w, LD), np.asarray(X, np.float64).reshape(-1, 3), tid


def reverdict(img, idx, kps, poses, cam, rec, mask, max_error, min_angle):
    """One eligible track under (new) poses at its unchanged X -> the record's dict after the re-verdict, plus error_margin and
    angle_margin"""
    used = [k for k in range(len(img)) if poses.get(int(img[k])) is not None]
    fit = [p for p, k in enumerate(used) if mask is None or mask[k]]
    f = (LD(cam[0]) + LD(cam[1])) / 2
    X = np.asarray(rec["X"], np.float64)
    e, z, centres = [], [], []
    for k in used:
        R, t = poses[int(img[k])]
        u, w = ref.observation(cam, kps[int(img[k])][int(idx[k]), :2])
        _, _, zz, err = stacked(R, t, np.asarray([u], LD), np.asarray([w], LD), X[None], f)
        e.append(float(err[0]))
        z.append(float(zz[0]))
        Rl, tl = np.asarray(R, np.float64).astype(LD).reshape(3, 3), np.asarray(t, np.float64).astype(LD)
        centres.append(-(Rl.T @ tl))
    e, z = np.asarray(e), np.asarray(z)
    ef, zf = e[fit], z[fit]
    bits = (ref.ERROR_OK if np.all(ef <= max_error) else 0) | (ref.DEPTH_OK if np.all(zf > ref.EPS) else 0)
    angle, hit, scanned = 0.0, False, []
    for a_ in range(len(fit)):
        for b_ in range(a_):
            g_ = ref.angle(X, centres[fit[a_]], centres[fit[b_]])
            scanned.append(g_)
            if g_ >= min_angle:
                angle, hit = g_, True
                break
            angle = max(angle, g_)
        if hit:
            break
    bits |= ref.ANGLE_OK if hit else 0
    out = dict(rec)
    res = np.array(rec["residuals"], np.float64)
    res[used] = e
    out.update(status=3 | bits | (rec["status"] & (ROBUST | REFINED)) | REPOSED, residuals=res, tri_angle=angle,
               mean_residual=float(np.sum(np.asarray(ef, LD)) / len(fit)), error_margin=float(np.min(np.abs(ef - max_error))),
               angle_margin=float(np.min(np.abs(np.asarray(scanned) - min_angle))) if scanned else np.inf)
    return out


def run(tracks, kps, poses, cam, records, masks=None, max_error=2.0, min_angle=1.5, max_iters=10, step_tol=1e-6, min_observations=15,
        fixed=()):
    """poses: dict image id -> (R, t) or None (the pose list, by ascending id); records: list of dicts (status, n_views, X,
    mean_residual, tri_angle, residuals) per track; masks: None, or one byte per observation.
    -> (new poses dict, per listed image dict(image_id, status, n_observations, + image()'s fields where attempted), the records after
    the re-verdict (dicts; `reposed` True where re-evaluated))"""
    offsets, img, idx = tracks[:3]
    f = (float(cam[0]) + float(cam[1])) / 2
    new, images, changed = dict(poses), [], set()
    for i in sorted(poses):
        rec = dict(image_id=i, status=POSE_FIXED if i in fixed else 0, n_observations=0, stands=False, fit=None,
                   trace=dict(steps=0, accepted=0, stop=STOP_NONE, verdict=NOT_ELIGIBLE, accepted_after_rejected=0, depth_rejected=0, cost=0.0))
        rec["trace"]["lambda"] = 0.0
        if poses[i] is not None and i not in fixed:
            u, w, X, tid = fitting_set(i, tracks, kps, cam, records, masks)
            rec["n_observations"] = len(u)
            if len(u) >= min_observations:
                R, t = poses[i]
                rec.update(image(R, t, u, w, X, f, max_error, max_iters, step_tol))
                rec["status"] |= POSE_ATTEMPTED | (POSE_REFINED if rec["stands"] else 0)
                rec["fit"] = (u, w, X)
                if rec["stands"]:
                    new[i] = (rec["R"], rec["t"])
                    changed.add(i)
        images.append(rec)
    out = []
    for t in range(len(offsets) - 1):
        a, b = int(offsets[t]), int(offsets[t + 1])
        r = dict(records[t])
        r["reposed"] = False
        if (r["status"] & 3) == 3 and any(int(i) in changed for i in img[a:b]):
            r = reverdict(img[a:b], idx[a:b], kps, new, cam, records[t], None if masks is None else masks[a:b], max_error, min_angle)
            r["reposed"] = True
        out.append(r)
    return new, images, out
