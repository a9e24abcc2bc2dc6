"""Independent reference of the track triangulation (include/msfm_match.h "track triangulation"), written from the definitions in plain
numpy: the DLT point from the STACKED 2n x 4 rows by numpy.linalg.svd (no normal equations, no Jacobi), the undistortion by a Newton
solve in long double (tests/emat_ref.py), errors in long double, angles by np.arccos.  Test infrastructure only.

    used observations   the elements of a consistent track whose image has a pose, in element order; fewer than max(2, min_views): status 0
    rows                u P[2] - P[0], v P[2] - P[1] with P = [R | t] and (u, v) the normalised undistorted observation
    point               the right singular vector of the smallest singular value, X = h[:3] / h[3]
    error               |proj(R X + t) - (u, v)| (fx + fy) / 2 per used observation; ERROR_OK: all <= max_error
    parallax            pairs for i: for j < i; the first angle >= min_angle ends the scan, else the largest one
"""
import numpy as np

import emat_ref

ATTEMPTED, POINT, ERROR_OK, ANGLE_OK, DEPTH_OK = 1, 2, 4, 8, 16
SUCCESS = POINT | ERROR_OK | ANGLE_OK
LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def observation(cam, xy):
    """fp32 pixel -> normalised undistorted (u, v), long double"""
    cam = tuple(LD(c) for c in (tuple(cam) + (0.0,) * (8 - len(cam))))
    x, y = LD(float(np.float32(xy[0]))), LD(float(np.float32(xy[1])))
    if not any(float(c) != 0.0 for c in cam[4:]):
        return (x - cam[2]) / cam[0], (y - cam[3]) / cam[1]
    return emat_ref.undistort(cam, x, y)


def angle(X, Oi, Oj):
    X, Oi, Oj = (np.asarray(a, LD) for a in (X, Oi, Oj))
    base, r1, r2 = np.sqrt(((Oi - Oj) ** 2).sum()), np.sqrt(((X - Oi) ** 2).sum()), np.sqrt(((X - Oj) ** 2).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        a = abs(np.arccos((r1 * r1 + r2 * r2 - base * base) / (2 * r1 * r2)))
    if np.isnan(a):
        return 0.0
    return float(min(a, LD(np.pi) - a) * 180 / LD(np.pi))


def mp_point(obs, dps=50):
    """The same algebraic problem as track()'s point -- the stacked rows u P[2] - P[0], v P[2] - P[1] (u, v rounded to fp64 as
    there), the right singular vector of the smallest singular value -- solved with mpmath at `dps` digits.  obs: [(u, v, P [3, 4])].
    -> X as three mpmath numbers, or None (h[3] == 0)"""
    import mpmath as mp
    with mp.workdps(dps):
        rows = []
        for u, v, P in obs:
            P = [[mp.mpf(float(x)) for x in row] for row in np.asarray(P, np.float64)]
            rows.append([mp.mpf(float(u)) * P[2][k] - P[0][k] for k in range(4)])
            rows.append([mp.mpf(float(v)) * P[2][k] - P[1][k] for k in range(4)])
        _, S, V = mp.svd_r(mp.matrix(rows))
        k = min(range(4), key=lambda i: S[i])
        if V[k, 3] == 0:
            return None
        return [V[k, j] / V[k, 3] for j in range(3)]


def mp_points(jobs):
    """mp_point over a list of observation lists, as float64 [n, 3] (NaN where there is no point): the unit of work of a process pool"""
    out = np.full((len(jobs), 3), np.nan)
    for n, obs in enumerate(jobs):
        X = mp_point(obs)
        if X is not None:
            out[n] = [float(x) for x in X]
    return out


def mp_angle(X, Oi, Oj, law_of_cosines, dps=50):
    """the parallax angle at X between the centres, degrees, with mpmath: by the definition's law of cosines, or (the true angle) by
    atan2 of the cross and dot products of the two rays"""
    import mpmath as mp
    with mp.workdps(dps):
        X, Oi, Oj = ([mp.mpf(x) for x in a] for a in (X, Oi, Oj))
        a, b = [x - o for x, o in zip(X, Oi)], [x - o for x, o in zip(X, Oj)]
        if law_of_cosines:
            base2 = sum((p - q) ** 2 for p, q in zip(Oi, Oj))
            r1, r2 = mp.sqrt(sum(x * x for x in a)), mp.sqrt(sum(x * x for x in b))
            ang = abs(mp.acos((r1 * r1 + r2 * r2 - base2) / (2 * r1 * r2)))
        else:
            cr = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            ang = mp.atan2(mp.sqrt(sum(x * x for x in cr)), sum(p * q for p, q in zip(a, b)))
        return min(ang, mp.pi - ang) * 180 / mp.pi


def track(img, idx, consistent, kps, poses, cam, max_error=2.0, min_angle=1.5, min_views=2):
    """One track (image ids, keypoint indices in element order) -> dict(status, n_views, X, mean_residual, tri_angle, residuals
    (element-aligned, -1 where none), error_margin = min |err - max_error|, angle_margin = min |a - min_angle| over the scanned pairs)."""
    n = len(img)
    out = dict(status=0, n_views=0, X=np.zeros(3), mean_residual=0.0, tri_angle=0.0, residuals=np.full(n, -1.0),
               error_margin=np.inf, angle_margin=np.inf)
    used = [k for k in range(n) if poses.get(int(img[k])) is not None]
    if not consistent or len(used) < max(2, int(min_views)):
        return out
    out["status"], out["n_views"] = ATTEMPTED, len(used)
    f = (LD(cam[0]) + LD(cam[1])) / 2
    rows, obs = [], []
    for k in used:
        R, t = poses[int(img[k])]
        P = np.c_[np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)]
        u, v = observation(cam, kps[int(img[k])][int(idx[k]), :2])
        obs.append((u, v, P))
        rows.append(float(u) * P[2] - P[0])
        rows.append(float(v) * P[2] - P[1])
    h = np.linalg.svd(np.asarray(rows, np.float64))[2][-1]
    if h[3] == 0.0 or not np.all(np.isfinite(h[:3] / h[3])):
        return out
    X = h[:3] / h[3]
    status = ATTEMPTED | POINT | ERROR_OK | DEPTH_OK
    errs = []
    for (u, v, P), k in zip(obs, used):
        Y = P[:, :3].astype(LD) @ X.astype(LD) + P[:, 3].astype(LD)
        if not float(Y[2]) > EPS:
            status &= ~DEPTH_OK
        with np.errstate(invalid="ignore", divide="ignore"):
            e = float(np.sqrt((Y[0] / Y[2] - u) ** 2 + (Y[1] / Y[2] - v) ** 2) * f)
        errs.append(e)
        out["residuals"][k] = e
        if not e <= max_error:
            status &= ~ERROR_OK
    centres = [-(P[:, :3].astype(LD).T @ P[:, 3].astype(LD)) for _, _, P in obs]
    best, hit, scanned = 0.0, False, []
    for i in range(len(used)):
        for j in range(i):
            a = angle(X, centres[i], centres[j])
            scanned.append(a)
            if a >= min_angle:
                best, hit = a, True
                break
            best = max(best, a)
        if hit:
            break
    if hit:
        status |= ANGLE_OK
    out.update(status=status, X=X, mean_residual=float(np.sum(np.asarray(errs, LD)) / len(errs)), tri_angle=best,
               error_margin=float(np.min(np.abs(np.asarray(errs) - max_error))),
               angle_margin=float(np.min(np.abs(np.asarray(scanned) - min_angle))) if scanned else np.inf)
    return out


def run(tracks, kps, poses, cam, max_error=2.0, min_angle=1.5, min_views=2):
    """tracks = (offsets, image_ids, point_idx, consistent) -> list of track() results"""
    offsets, img, idx, cons = tracks
    return [track(img[offsets[t]:offsets[t + 1]], idx[offsets[t]:offsets[t + 1]], bool(cons[t]), kps, poses, cam, max_error, min_angle,
                  min_views) for t in range(len(offsets) - 1)]


def proto_tracks(ids, protos, min_length=2):
    """The ground-truth tracks of a synthetic capture: every prototype seen by at least min_length images is one track, its elements
    by ascending (image id, row), the tracks by ascending first element -- the order of a track session's result."""
    seen = {}
    for k in np.argsort(np.asarray(ids)):
        for row, p in enumerate(np.asarray(protos[k])):
            if p >= 0:
                seen.setdefault(int(p), []).append((int(ids[k]), row))
    kept = sorted((el, p) for p, el in seen.items() if len(el) >= min_length)
    offsets = np.concatenate([[0], np.cumsum([len(el) for el, _ in kept])]).astype(np.int64)
    flat = [e for el, _ in kept for e in el]
    img = np.asarray([e[0] for e in flat], np.int32)
    idx = np.asarray([e[1] for e in flat], np.int32)
    return (offsets, img, idx, np.ones(len(kept), np.uint8)), [p for _, p in kept]
