"""Independent reference of the map filtering (include/msfm_match.h "map filtering"), written from the definitions and the reference's
Map::FilterPoints3DWithLargeReprojectionError / ...WithSmallTriangulationAngle in plain numpy: projection errors, depths, centres and
the parallax scans in long double (np.arccos for the angle).  Test infrastructure only.

    inlier bytes      given, or (a session without any) 1 on the posed elements of an attempted track
    fitting set F     the posed elements whose byte is 1, in element order
    eligible          consistent, ATTEMPTED | POINT, and (with a scope) an element of F in a listed image
    drop              per element of F: depth <= eps -> dropped by depth; otherwise not (err <= max_error) -> dropped by error
    removed           fewer than two survivors (by views); otherwise no pair of survivors reaches the call's min_angle (by angle)
    trimmed           something dropped, not removed: the verdict over the survivors at the same X with the SESSION's thresholds
"""
import numpy as np

import triangulation_ref as ref

LD = ref.LD
NOT_ELIGIBLE, UNTOUCHED, TRIMMED, REMOVED_BY_VIEWS, REMOVED_BY_ANGLE = 0, 1, 2, 3, 4
ROBUST, REFINED, REPOSED, EXTENDED, FILTERED = 32, 64, 128, 256, 512


def scan(X, centres, order, min_angle):
    """pairs for a: for b < a over `order`; -> (hit, the pair's angle or the largest seen, min |angle - min_angle| over the scanned pairs)"""
    best, margin = 0.0, np.inf
    for a in range(len(order)):
        for b in range(a):
            g = ref.angle(X, centres[order[a]], centres[order[b]])
            margin = min(margin, abs(g - min_angle))
            if g >= min_angle:
                return True, g, margin
            best = max(best, g)
    return False, best, margin


def track(img, idx, consistent, kps, poses, cam, rec, res, mask, session, call, scope=None):
    """One track.  rec: its POINT3D record, res: its residual slots, mask: its inlier bytes or None; poses: dict id -> (R, t) / None;
    session, call: (max_error, min_angle); scope: a set of image ids or None.
    -> dict(kind, dropped_by_depth, dropped_by_error, kept, regained, status, n_views, X, mean_residual, tri_angle, residuals, mask,
            error_margin = min |err - a threshold it was compared with|, angle_margin = the same for the scanned angles)"""
    n = len(img)
    status = int(rec["status"])
    posed = np.asarray([poses.get(int(i)) is not None for i in img], bool)
    if mask is None:
        mask = (posed & bool(status & ref.ATTEMPTED)).astype(np.uint8)
    else:
        mask = np.array(mask, np.uint8)
    out = dict(kind=NOT_ELIGIBLE, dropped_by_depth=0, dropped_by_error=0, kept=0, regained=False, status=status, n_views=int(rec["n_views"]),
               X=np.array(rec["X"], np.float64), mean_residual=float(rec["mean_residual"]), tri_angle=float(rec["tri_angle"]),
               residuals=np.array(res, np.float64), mask=mask, error_margin=np.inf, angle_margin=np.inf)
    fit = [k for k in range(n) if posed[k] and mask[k]]
    need = ref.ATTEMPTED | ref.POINT
    if not consistent or (status & need) != need:
        return out
    if scope is not None and not any(int(img[k]) in scope for k in fit):
        return out
    f = (LD(cam[0]) + LD(cam[1])) / 2
    X = out["X"].astype(LD)
    errs, depth, centres = {}, {}, {}
    for k in range(n):
        if not posed[k]:
            continue
        R, t = poses[int(img[k])]
        R, t = np.asarray(R, np.float64).reshape(3, 3).astype(LD), np.asarray(t, np.float64).reshape(3).astype(LD)
        u, v = ref.observation(cam, kps[int(img[k])][int(idx[k]), :2])
        Y = R @ X + t
        with np.errstate(invalid="ignore", divide="ignore"):
            errs[k] = np.sqrt((Y[0] / Y[2] - u) ** 2 + (Y[1] / Y[2] - v) ** 2) * f
        depth[k] = bool(float(Y[2]) > ref.EPS)
        centres[k] = -(R.T @ t)
    K = []
    for k in fit:
        if not depth[k]:
            out["dropped_by_depth"] += 1
            continue
        out["error_margin"] = min(out["error_margin"], abs(float(errs[k]) - call[0]))
        if not bool(errs[k] <= call[0]):
            out["dropped_by_error"] += 1
            continue
        K.append(k)
    out["kept"] = len(K)
    dropped = len(fit) - len(K)
    removed = None
    if len(K) < 2:
        removed = REMOVED_BY_VIEWS
    else:
        hit, _, margin = scan(X, centres, K, call[1])
        out["angle_margin"] = min(out["angle_margin"], margin)
        if not hit:
            removed = REMOVED_BY_ANGLE
    if removed is not None:
        out.update(kind=removed, status=ref.ATTEMPTED | FILTERED, n_views=0, X=np.zeros(3), mean_residual=0.0, tri_angle=0.0,
                   residuals=np.full(n, -1.0), mask=np.zeros(n, np.uint8))
        return out
    if dropped == 0:
        out["kind"] = UNTOUCHED
        return out
    out["kind"] = TRIMMED
    total, error_ok = LD(0), True
    for k in K:
        total = total + errs[k]
        out["error_margin"] = min(out["error_margin"], abs(float(errs[k]) - session[0]))
        error_ok = error_ok and bool(errs[k] <= session[0])
    hit, best, margin = scan(X, centres, K, session[1])
    out["angle_margin"] = min(out["angle_margin"], margin)
    bits = (ref.ERROR_OK if error_ok else 0) | (ref.ANGLE_OK if hit else 0) | ref.DEPTH_OK    # (every survivor has positive depth)
    for k in range(n):
        if posed[k]:
            out["residuals"][k] = float(errs[k])
    new_mask = np.zeros(n, np.uint8)
    new_mask[K] = 1
    new_status = ref.ATTEMPTED | ref.POINT | bits | (status & (ROBUST | REFINED | REPOSED | EXTENDED)) | FILTERED
    out.update(status=new_status, n_views=len(K), mean_residual=float(total / len(K)), tri_angle=best, mask=new_mask,
               regained=(status & ref.SUCCESS) != ref.SUCCESS and (new_status & ref.SUCCESS) == ref.SUCCESS)
    return out


def run(tracks, kps, poses, cam, points, residuals, mask, session, call=None, scope=None):
    """tracks = (offsets, image_ids, point_idx, consistent); kps: dict id -> keypoints; poses: dict id -> (R, t) / None; session =
    (max_error, min_angle) of the triangulation; call: the call's, None = the session's; scope: image ids, None or empty = every track
    -> list of track() results"""
    offsets, img, idx, cons = tracks[:4]
    call = tuple(session[:2]) if call is None else tuple(call)
    scope = set(int(i) for i in scope) if scope is not None and len(scope) else None
    out = []
    for t in range(len(offsets) - 1):
        b, e = int(offsets[t]), int(offsets[t + 1])
        out.append(track(img[b:e], idx[b:e], bool(cons[t]), kps, poses, cam, points[t], residuals[b:e],
                         None if mask is None else mask[b:e], tuple(session[:2]), call, scope))
    return out
