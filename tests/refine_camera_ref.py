"""Independent numpy reference of the camera refinement: stacked residuals in pixel units in a chosen float type
(long double, or float64 for the reference's own scatter), the undistortion by a Newton solve to 1e-15, the Jacobian by implicit
differentiation of the Brown model with numpy.linalg.solve, H and g as matrix products, numpy.linalg.cholesky and numpy.linalg.solve
for the step, the LM, stop and standing rules of csrc/msfm_refine_camera.h, the trace fields of msfm_ref::Trace, and the re-verdict's
errors.  It shares no code with the twin and sums in numpy's order.  Test infrastructure only."""
import numpy as np

LD = np.longdouble
FX_FY, F, CX_CY, K1_K2 = 1, 2, 4, 8
STOP_NONE, STOP_STEP, STOP_MAX_ITERS, STOP_CEILING, STOP_FEW, STOP_NONFINITE = 0, 1, 2, 3, 4, 5
NOT_ELIGIBLE, NO_ACCEPTED_STEP, LOST_INLIERS = 1, 2, 3
STANDING = 1 | 2 | 4 | 8
RECALIBRATED = 2048
KEPT = 32 | 64 | 128 | 256 | 512 | 1024
DEPTH_EPS = 2.220446049250313e-16
TRACE_KEYS = ("steps", "accepted", "stop", "verdict", "accepted_after_rejected")


def columns(mask):
    """the unknowns a mask selects, as names in the system's order"""
    out = []
    if mask & FX_FY:
        out += ["fx", "fy"]
    if mask & F:
        out += ["s"]
    if mask & CX_CY:
        out += ["cx", "cy"]
    if mask & K1_K2:
        out += ["k1", "k2"]
    return out


def distort(cam, u, w):
    fx, fy, cx, cy, k1, k2, p1, p2 = cam
    r2 = u * u + w * w
    rad = 1 + k1 * r2 + k2 * r2 * r2
    return u * rad + 2 * p1 * u * w + p2 * (r2 + 2 * u * u), w * rad + p1 * (r2 + 2 * w * w) + 2 * p2 * u * w


def distort_jacobian(cam, u, w):
    """d distort / d(u, w) -> a, b, c, d of [[a, b], [c, d]] per observation"""
    fx, fy, cx, cy, k1, k2, p1, p2 = cam
    r2 = u * u + w * w
    rad = 1 + k1 * r2 + k2 * r2 * r2
    dr = k1 + 2 * k2 * r2
    return (rad + 2 * u * u * dr + 2 * p1 * w + 6 * p2 * u, 2 * u * w * dr + 2 * p1 * u + 2 * p2 * w,
            2 * u * w * dr + 2 * p1 * u + 2 * p2 * w, rad + 2 * w * w * dr + 6 * p1 * w + 2 * p2 * u)


def undistort(cam, px, py, T):
    """Newton on distort(u, w) = d to 1e-15 (relative to 1 + |d|)"""
    cam = tuple(T(v) for v in cam)
    dx, dy = (px - cam[2]) / cam[0], (py - cam[3]) / cam[1]
    u, w = dx.copy(), dy.copy()
    for _ in range(50):
        gx, gy = distort(cam, u, w)
        ex, ey = gx - dx, gy - dy
        a, b, c, d = distort_jacobian(cam, u, w)
        det = a * d - b * c
        su, sw = (d * ex - b * ey) / det, (a * ey - c * ex) / det
        u, w = u - su, w - sw
        with np.errstate(invalid="ignore"):
            if not np.any(np.hypot(su, sw) > 1e-15 * (1 + np.hypot(dx, dy))):   # (a NaN observation never converges and stops nothing)
                break
    return u, w


class Problem:
    """the contributing set of a map: raw pixels and reprojections, in the tracks' order"""

    def __init__(self, tracks, kps, poses, points, mask, T=LD):
        offs, img, idx = (np.asarray(a) for a in tracks[:3])
        px, py, qx, qy, self.slot = [], [], [], [], []
        self.behind = 0
        for t in range(len(offs) - 1):
            if (int(points[t]["status"]) & STANDING) != STANDING:
                continue
            X = np.asarray(points[t]["X"], T)
            for o in range(int(offs[t]), int(offs[t + 1])):
                pose = poses.get(int(img[o]))
                if pose is None or (mask is not None and not mask[o]):
                    continue
                Y = np.asarray(pose[0], T) @ X + np.asarray(pose[1], T)
                if not Y[2] > DEPTH_EPS:
                    self.behind += 1
                    continue
                k = kps[int(img[o])][int(idx[o])]
                px.append(T(np.float32(k[0])))
                py.append(T(np.float32(k[1])))
                qx.append(Y[0] / Y[2])
                qy.append(Y[1] / Y[2])
                self.slot.append(o)
        self.px, self.py, self.qx, self.qy = (np.asarray(a, T) for a in (px, py, qx, qy))
        self.n, self.T = len(px), T

    def residual(self, cam):
        """stacked (rx.., ry..) in pixels, and the per-observation error"""
        T = self.T
        u, w = undistort(cam, self.px, self.py, T)
        f = (T(cam[0]) + T(cam[1])) / 2
        ex, ey = self.qx - u, self.qy - w
        return np.concatenate([ex * f, ey * f]), np.sqrt(ex * ex + ey * ey) * f

    def cost(self, cam):
        r, err = self.residual(cam)
        return float(r @ r), err

    def jacobian(self, cam, mask):
        """d residual / d unknowns, [2 n, len(columns(mask))], by implicit differentiation: per observation numpy.linalg.solve of
        (d distort / d(u, w)) d(u, w) = d d - d distort"""
        T = self.T
        camT = tuple(T(v) for v in cam)
        fx, fy, cx, cy, k1, k2, p1, p2 = camT
        u, w = undistort(cam, self.px, self.py, T)
        f = (fx + fy) / 2
        dx, dy = (self.px - cx) / fx, (self.py - cy) / fy
        a, b, c, d = distort_jacobian(camT, u, w)
        A = np.stack([np.stack([a, b], -1), np.stack([c, d], -1)], -2).astype(np.float64)
        r2 = u * u + w * w
        zero = np.zeros_like(u)
        rhs = {"fx": (-dx / fx, zero), "fy": (zero, -dy / fy), "cx": (-1 / fx + zero, zero), "cy": (zero, -1 / fy + zero),
               "k1": (-r2 * u, -r2 * w), "k2": (-r2 * r2 * u, -r2 * r2 * w)}
        duw = {k: np.linalg.solve(A, np.stack(v, -1).astype(np.float64)[..., None])[..., 0].astype(T) for k, v in rhs.items()}
        ex, ey = self.qx - u, self.qy - w
        col = {}
        for k in rhs:
            df = T(0.5) if k in ("fx", "fy") else T(0)
            col[k] = np.concatenate([ex * df - f * duw[k][:, 0], ey * df - f * duw[k][:, 1]])
        col["s"] = fx * col["fx"] + fy * col["fy"]
        return np.stack([col[k] for k in columns(mask)], 1)


def apply(cam, mask, delta):
    """the camera moved by the step, and the step as (dfx, dfy, dcx, dcy, dk1, dk2)"""
    d = dict(zip(columns(mask), (float(v) for v in delta)))
    c = list(cam)
    if mask & F:
        dfx, dfy = c[0] * d["s"], c[1] * d["s"]
        c[0], c[1] = c[0] * (1.0 + d["s"]), c[1] * (1.0 + d["s"])
    else:
        dfx, dfy = d.get("fx", 0.0), d.get("fy", 0.0)
        c[0], c[1] = c[0] + dfx, c[1] + dfy
    for at, k in ((2, "cx"), (3, "cy"), (4, "k1"), (5, "k2")):
        c[at] = c[at] + d.get(k, 0.0)
    return tuple(c), (dfx, dfy, d.get("cx", 0.0), d.get("cy", 0.0), d.get("k1", 0.0), d.get("k2", 0.0))


def refine(pb, cam, mask, max_error, max_iters, step_tol, min_observations):
    """the LM of csrc/msfm_refine_camera.h over the Problem -> dict: camera, stands, trace, costs, inlier counts and the margins every
    decision kept from its threshold (cost: relative; step: of the stop test's left side from step_tol^2, relative; error: px)"""
    cam = tuple(float(v) for v in cam) + (0.0,) * (8 - len(cam))
    out = dict(camera=cam, stands=False, cost_before=0.0, cost_after=0.0, inliers_before=0, inliers_after=0, observations=pb.n,
               behind=pb.behind, cost_margin=np.inf, step_margin=np.inf, error_margin=np.inf, pivot_rejected=0,
               trace=dict(steps=0, accepted=0, stop=STOP_NONE, verdict=NOT_ELIGIBLE, accepted_after_rejected=0, cost=0.0, **{"lambda": 0.0}))
    tr = out["trace"]
    if pb.n < min_observations:
        tr["stop"] = STOP_FEW
        return out
    c, err0 = pb.cost(cam)
    if not np.isfinite(c):
        tr["stop"] = STOP_NONFINITE
        return out
    c0, lam, cur = c, 1e-3, cam
    steps = accepted = after_rejected = 0
    last_rejected, stop, J, r = False, STOP_MAX_ITERS, None, None
    while steps < max_iters:
        if J is None:
            J, r = pb.jacobian(cur, mask), pb.residual(cur)[0]
            H, g = np.asarray(J.T @ J, np.float64), np.asarray(J.T @ r, np.float64)
        steps += 1
        accept, new = False, None
        try:
            A = H + lam * np.diag(np.diag(H))
            np.linalg.cholesky(A)                      # (a pivot that is not > 0: LinAlgError)
            delta = np.linalg.solve(A, -g)
            new, d6 = apply(cur, mask, delta)
            ok = np.all(np.isfinite(delta)) and np.all(np.isfinite(new)) and new[0] > 0 and new[1] > 0
        except np.linalg.LinAlgError:
            ok = False
            out["pivot_rejected"] += 1
        if ok:
            cn, _ = pb.cost(new)
            accept = bool(np.isfinite(cn) and cn < c)
            if np.isfinite(cn):
                out["cost_margin"] = min(out["cost_margin"], abs(cn - c) / c)
        if accept:
            cur, c, J = new, cn, None
            accepted += 1
            after_rejected += 1 if last_rejected else 0
            last_rejected = False
            lam = max(lam / 10.0, 1e-12)
            fn = (cur[0] + cur[1]) / 2
            d2 = (d6[0] / cur[0]) ** 2 + (d6[1] / cur[1]) ** 2 + (d6[2] / fn) ** 2 + (d6[3] / fn) ** 2 + d6[4] ** 2 + d6[5] ** 2
            if step_tol > 0:
                out["step_margin"] = min(out["step_margin"], abs(d2 - step_tol ** 2) / step_tol ** 2)
            if d2 <= step_tol ** 2:
                stop = STOP_STEP
                break
        else:
            last_rejected = True
            lam = lam * 10.0
            if lam > 1e4:
                stop = STOP_CEILING
                break
    before = int((err0 <= max_error).sum())
    after = before
    margin = float(np.abs(np.asarray(err0, np.float64) - max_error).min())
    if accepted:
        err1 = pb.cost(cur)[1]
        after = int((err1 <= max_error).sum())
        margin = min(margin, float(np.abs(np.asarray(err1, np.float64) - max_error).min()))
    stands = accepted > 0 and after >= before
    out.update(camera=cur if stands else cam, refined_camera=cur, stands=stands, cost_before=c0, cost_after=c if stands else c0,
               inliers_before=before, inliers_after=after, error_margin=margin)
    tr.update(steps=steps, accepted=accepted, stop=stop, verdict=0 if stands else (LOST_INLIERS if accepted else NO_ACCEPTED_STEP),
              accepted_after_rejected=after_rejected, cost=c, **{"lambda": lam})
    return out


def reverdict(tracks, kps, poses, points, residuals, mask, cam, max_error, T=LD):
    """every ATTEMPTED | POINT track at its X under `cam` -> list of None (not eligible) or dict(status, residuals, mean_residual,
    error_margin); the record's ANGLE_OK and DEPTH_OK do not depend on the camera and are taken from the record"""
    offs, img, idx = (np.asarray(a) for a in tracks[:3])
    f = (T(cam[0]) + T(cam[1])) / 2
    n_obs = np.diff(offs)
    track_of = np.repeat(np.arange(len(offs) - 1), n_obs)
    status = np.asarray(points["status"]).astype(np.int64)
    err = np.full(len(img), T(-1.0), T)
    used = np.zeros(len(img), bool)
    X = np.asarray(points["X"], T)
    for i, pose in poses.items():
        if pose is None:
            continue
        at = np.nonzero((img == i) & ((status[track_of] & 3) == 3))[0]
        if not len(at):
            continue
        k = np.asarray(kps[int(i)], np.float32)[idx[at]]
        u, w = undistort(cam, k[:, 0].astype(T), k[:, 1].astype(T), T)
        Y = X[track_of[at]] @ np.asarray(pose[0], T).T + np.asarray(pose[1], T)
        err[at] = np.sqrt((Y[:, 0] / Y[:, 2] - u) ** 2 + (Y[:, 1] / Y[:, 2] - w) ** 2) * f
        used[at] = True
    out = []
    for t in range(len(offs) - 1):
        st = int(status[t])
        if (st & 3) != 3:
            out.append(None)
            continue
        a, b = int(offs[t]), int(offs[t + 1])
        res = np.asarray(residuals[a:b], np.float64).copy()
        res[used[a:b]] = err[a:b][used[a:b]].astype(np.float64)
        fit = used[a:b] if mask is None else used[a:b] & (np.asarray(mask[a:b]) != 0)
        e = err[a:b][fit]
        out.append(dict(status=1 | 2 | (4 if bool(np.all(e <= max_error)) else 0) | (st & (8 | 16)) | (st & KEPT) | RECALIBRATED, residuals=res,
                        mean_residual=float(e.sum() / len(e)), error_margin=float(np.abs(e.astype(np.float64) - max_error).min())))
    return out
