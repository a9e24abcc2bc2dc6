"""Independent reference of the map extension (include/msfm_match.h "map extension"), written from the definitions in plain numpy:
projection errors, depths, centres and the parallax scan of a CONTINUED track in long double (np.arccos for the angle), CREATED tracks
through tests/triangulation_ref.py / tests/robust_triangulation_ref.py under the enlarged poses.  Test infrastructure only.

    new observation   an element of a consistent track in an image that gets its valid pose in this call
    inlier bytes      given, or (after the plain call) 1 on the elements of an attempted track whose image was posed before the call
    continue          the record has POINT | ERROR_OK | ANGLE_OK: per new observation err at the record's X, byte = depth > eps and
                      err <= max_error; at least one accepted: n_views, the mean of the byte-1 residual slots, the parallax scan
    create            every other touched track: the full triangulation of the track under the enlarged poses
"""
import numpy as np

import robust_triangulation_ref as rob
import triangulation_ref as ref

LD = ref.LD
UNTOUCHED, CONTINUE, CREATE = 0, 1, 2
EXTENDED = 256


def bytes_before(img, rec_status, poses_before):
    """the inlier bytes of one track of a session without any"""
    posed = np.asarray([poses_before.get(int(i)) is not None for i in img], bool)
    return (posed & bool(rec_status & ref.ATTEMPTED)).astype(np.uint8)


def track(img, idx, consistent, kps, poses_before, new, cam, rec, res, mask, track_no, max_error=2.0, min_angle=1.5, min_views=2,
          max_hypotheses=0):
    """One track.  rec: its POINT3D record, res: its residual slots, mask: its inlier bytes or None.
    -> dict(kind, new (element positions), accepted, rejected, status, n_views, X, mean_residual, tri_angle, residuals, mask,
            error_margin = min |err - max_error| over the new observations, angle_margin = min |a - min_angle| over the scanned pairs,
            depth_margin = min |depth| over the new observations)"""
    n = len(img)
    mask = bytes_before(img, int(rec["status"]), poses_before) if mask is None else np.array(mask, np.uint8)
    out = dict(kind=UNTOUCHED, new=[], accepted=0, rejected=0, status=int(rec["status"]), n_views=int(rec["n_views"]),
               X=np.array(rec["X"], np.float64), mean_residual=float(rec["mean_residual"]), tri_angle=float(rec["tri_angle"]),
               residuals=np.array(res, np.float64), mask=mask, error_margin=np.inf, angle_margin=np.inf, depth_margin=np.inf, retried=False)
    fresh = [k for k in range(n) if new.get(int(img[k])) is not None] if consistent else []
    out["new"] = fresh
    if not fresh:
        return out
    poses = dict(poses_before)
    poses.update({i: p for i, p in new.items() if p is not None})
    if (out["status"] & ref.SUCCESS) != ref.SUCCESS:
        out["kind"] = CREATE
        if max_hypotheses > 0:
            r = rob.track(img, idx, True, kps, poses, cam, track_no, max_error, min_angle, min_views, max_hypotheses)
        else:
            r = ref.track(img, idx, True, kps, poses, cam, max_error, min_angle, min_views)
            r["mask"] = bytes_before(img, r["status"], poses)
        out.update(status=r["status"] | EXTENDED, n_views=r["n_views"], X=r["X"], mean_residual=r["mean_residual"], tri_angle=r["tri_angle"],
                   residuals=r["residuals"], mask=r["mask"], error_margin=r["error_margin"], angle_margin=r["angle_margin"],
                   retried=bool(r.get("retried", False)))
        return out
    out["kind"] = CONTINUE
    f = (LD(cam[0]) + LD(cam[1])) / 2
    X = out["X"].astype(LD)
    errs = {}
    for k in fresh:
        R, t = poses[int(img[k])]
        R, t = np.asarray(R, np.float64).reshape(3, 3).astype(LD), np.asarray(t, np.float64).reshape(3).astype(LD)
        u, v = ref.observation(cam, kps[int(img[k])][int(idx[k]), :2])
        Y = R @ X + t
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.sqrt((Y[0] / Y[2] - u) ** 2 + (Y[1] / Y[2] - v) ** 2) * f
        ok = bool(float(Y[2]) > ref.EPS) and bool(e <= max_error)
        errs[k] = e
        out["residuals"][k] = float(e)
        out["mask"][k] = 1 if ok else 0
        out["accepted" if ok else "rejected"] += 1
        out["error_margin"] = min(out["error_margin"], abs(float(e) - max_error))
        out["depth_margin"] = min(out["depth_margin"], abs(float(Y[2])))
    if out["accepted"] == 0:
        return out
    fit = [k for k in range(n) if out["mask"][k]]
    total = LD(0)
    for k in fit:
        total = total + (errs[k] if k in errs else LD(res[k]))
    centres = {}
    for k in fit:
        R, t = poses[int(img[k])]
        centres[k] = -(np.asarray(R, np.float64).reshape(3, 3).astype(LD).T @ np.asarray(t, np.float64).reshape(3).astype(LD))
    best, hit = 0.0, False
    for a in range(len(fit)):
        for b in range(a):
            g = ref.angle(X, centres[fit[a]], centres[fit[b]])
            out["angle_margin"] = min(out["angle_margin"], abs(g - min_angle))
            if g >= min_angle:
                best, hit = g, True
                break
            best = max(best, g)
        if hit:
            break
    out.update(status=out["status"] | EXTENDED, n_views=len(fit), mean_residual=float(total / len(fit)), tri_angle=best, angle_hit=hit)
    return out


def run(tracks, kps, poses_before, new, cam, points, residuals, mask=None, max_error=2.0, min_angle=1.5, min_views=2, max_hypotheses=0):
    """tracks = (offsets, image_ids, point_idx, consistent); kps: dict id -> keypoints; poses_before, new: dicts id -> (R, t) / None
    -> list of track() results"""
    offsets, img, idx, cons = tracks[:4]
    out = []
    for t in range(len(offsets) - 1):
        b, e = int(offsets[t]), int(offsets[t + 1])
        out.append(track(img[b:e], idx[b:e], bool(cons[t]), kps, poses_before, new, cam, points[t], residuals[b:e],
                         None if mask is None else mask[b:e], t, max_error, min_angle, min_views, max_hypotheses))
    return out
