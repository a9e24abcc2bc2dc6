"""Independent reference of the map completion (include/msfm_match.h "map completion"), written from the definitions and the
reference's Map::CompletePoint3D (positive depth first, then the reprojection error against the threshold) in plain numpy: projection
errors, depths, centres and the parallax scan in long double (np.arccos for the angle).  Test infrastructure only.

    inlier bytes      given, or (a session without any) 1 on the posed elements of an attempted track
    candidates        the posed elements whose byte is 0, in element order, in a listed image where a list is given
    eligible          consistent, POINT | ERROR_OK | ANGLE_OK
    admission         per candidate: depth <= eps -> rejected by depth; otherwise not (err <= max_error) -> rejected by error
    completed         something admitted: the verdict over the old fitting set and the admitted ones at the same X with the SESSION's
                      thresholds
"""
import numpy as np

import filter_ref as fr
import triangulation_ref as ref

LD = ref.LD
NOT_ELIGIBLE, UNTOUCHED, COMPLETED = 0, 1, 2
HISTORY = fr.ROBUST | fr.REFINED | fr.REPOSED | fr.EXTENDED | fr.FILTERED
COMPLETED_BIT = 1024


def track(img, idx, consistent, kps, poses, cam, rec, res, mask, session, max_error, scope=None):
    """One track.  rec: its POINT3D record, res: its residual slots, mask: its inlier bytes or None; poses: dict id -> (R, t) / None;
    session: (max_error, min_angle); max_error: the call's; scope: a set of image ids or None.
    -> dict(kind, candidates, admitted, rejected_by_depth, rejected_by_error, status, n_views, X, mean_residual, tri_angle, residuals,
            mask, error_margin = min |err - a threshold it was compared with|, angle_margin = the same for the scanned angles)"""
    n = len(img)
    status = int(rec["status"])
    posed = np.asarray([poses.get(int(i)) is not None for i in img], bool)
    if mask is None:
        mask = (posed & bool(status & ref.ATTEMPTED)).astype(np.uint8)
    else:
        mask = np.array(mask, np.uint8)
    out = dict(kind=NOT_ELIGIBLE, candidates=0, admitted=0, rejected_by_depth=0, rejected_by_error=0, status=status,
               n_views=int(rec["n_views"]), X=np.array(rec["X"], np.float64), mean_residual=float(rec["mean_residual"]),
               tri_angle=float(rec["tri_angle"]), residuals=np.array(res, np.float64), mask=mask, error_margin=np.inf, angle_margin=np.inf)
    if not consistent or (status & ref.SUCCESS) != ref.SUCCESS:
        return out
    out["kind"] = UNTOUCHED
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
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            errs[k] = np.sqrt((Y[0] / Y[2] - u) ** 2 + (Y[1] / Y[2] - v) ** 2) * f
        depth[k] = bool(float(Y[2]) > ref.EPS)
        centres[k] = -(R.T @ t)
    admitted = []
    for k in range(n):
        if not posed[k] or mask[k] or (scope is not None and int(img[k]) not in scope):
            continue
        out["candidates"] += 1
        if not depth[k]:
            out["rejected_by_depth"] += 1
            continue
        out["error_margin"] = min(out["error_margin"], abs(float(errs[k]) - max_error))
        if not bool(errs[k] <= max_error):
            out["rejected_by_error"] += 1
            continue
        admitted.append(k)
    out["admitted"] = len(admitted)
    if not admitted:
        return out
    out["kind"] = COMPLETED
    new_mask = mask.copy()
    new_mask[admitted] = 1
    K = [k for k in range(n) if posed[k] and new_mask[k]]
    total, error_ok, depth_ok = LD(0), True, True
    for k in K:
        total = total + errs[k]
        out["error_margin"] = min(out["error_margin"], abs(float(errs[k]) - session[0]))
        error_ok = error_ok and bool(errs[k] <= session[0])
        depth_ok = depth_ok and depth[k]
    hit, best, margin = fr.scan(X, centres, K, session[1])
    out["angle_margin"] = min(out["angle_margin"], margin)
    bits = (ref.ERROR_OK if error_ok else 0) | (ref.ANGLE_OK if hit else 0) | (ref.DEPTH_OK if depth_ok else 0)
    for k in range(n):
        if posed[k]:
            out["residuals"][k] = float(errs[k])
    out.update(status=ref.ATTEMPTED | ref.POINT | bits | (status & HISTORY) | COMPLETED_BIT, n_views=len(K),
               mean_residual=float(total / len(K)), tri_angle=best, mask=new_mask)
    return out


def run(tracks, kps, poses, cam, points, residuals, mask, session, max_error=None, scope=None):
    """tracks = (offsets, image_ids, point_idx, consistent); kps: dict id -> keypoints; poses: dict id -> (R, t) / None; session =
    (max_error, min_angle) of the triangulation; max_error: the call's, None = the session's; scope: image ids, None or empty = every
    image -> list of track() results"""
    offsets, img, idx, cons = tracks[:4]
    max_error = float(session[0]) if max_error is None else float(max_error)
    scope = set(int(i) for i in scope) if scope is not None and len(scope) else None
    out = []
    for t in range(len(offsets) - 1):
        b, e = int(offsets[t]), int(offsets[t + 1])
        out.append(track(img[b:e], idx[b:e], bool(cons[t]), kps, poses, cam, points[t], residuals[b:e],
                         None if mask is None else mask[b:e], tuple(session[:2]), max_error, scope))
    return out
