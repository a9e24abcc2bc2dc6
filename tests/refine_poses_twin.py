"""ctypes driver of the pose refinement's host twin (csrc/msfm_refine_poses.h, RefinePoses, through libmsfm_host.so): the poses,
per-image records, point records, residuals and counters the device must give after msfm_refine_poses.  One call, one thread: an
image's fitting set runs through every track.  Test infrastructure only."""
import ctypes as C

import numpy as np

import refine_points_twin as rtw
import triangulation_twin as tw
from monocularsfm_amd import _lib
from monocularsfm_amd._lib import pose_table

DP = tw.DP
DEFAULTS = (10, 1e-6, 15)   # max_iters, step_tol, min_observations
COUNT_KEYS = ("images", "eligible", "refined", "rejected_by_inliers", "iterations", "observations", "points_reposed", "points_lost",
              "points_gained")
COST_KEYS = ("cost_before", "cost_after")
STOP_NONE, STOP_STEP, STOP_MAX_ITERS, STOP_CEILING = 0, 1, 2, 3
NOT_ELIGIBLE, NO_ACCEPTED_STEP, LOST_INLIERS = 1, 2, 3          # verdict: 0 stands, else why not
# msfm_ref::Trace, as msfm_rp::refine_image fills it: the route an image took (csrc/msfm_refine.h)
TRACE = np.dtype([("steps", np.int32), ("accepted", np.int32), ("stop", np.int32), ("verdict", np.int32),
                  ("accepted_after_rejected", np.int32), ("depth_rejected", np.int32), ("lambda", np.float64), ("cost", np.float64)])
assert TRACE.itemsize == 40


def load_host():
    L = rtw.load_host()   # (the triangulation and point refinement twins' exports as well)
    vp = C.c_void_p
    L.host_refine_poses.argtypes = [vp, vp, vp, C.c_longlong, vp, C.c_int, vp, vp, vp, C.c_int, DP, C.c_double, C.c_double, C.c_double,
                                    C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    return L


def as_pose_list(poses):
    """a dict as triangulate_tracks takes it, or (ids, POSE_RT array) as Context.pose_list() returns it -> (ids, a copy of the table)"""
    if isinstance(poses, dict):
        return pose_table(poses)
    ids, tab = poses
    return np.ascontiguousarray(ids, np.int32), np.array(tab, _lib.POSE_RT)


def poses_dict(ids, tab):
    return {int(i): ((p["R"].reshape(3, 3).copy(), p["t"].copy()) if p["valid"] else None) for i, p in zip(ids, tab)}


def run(host, tracks, ids, kps, poses, cam, points, residuals, mask=None, thresholds=(2.0, 1.5), params=DEFAULTS, fixed=(), trace=False):
    """tracks, ids, kps, cam as triangulation_twin.run takes them; poses: see as_pose_list; points, residuals (and mask, after the
    robust call): the current records -- they are NOT changed; thresholds = (max_error, min_angle) of the triangulation; params =
    (max_iters, step_tol, min_observations).
    -> (POINT3D array [T], residuals float64 [O], (ids, POSE_RT array) of the new pose list, POSE_REFINEMENT array, dict of COUNT_KEYS and
    COST_KEYS); with trace=True a sixth value, the TRACE array per listed image."""
    offsets = np.ascontiguousarray(tracks[0], np.int64)
    img = np.ascontiguousarray(tracks[1], np.int32)
    idx = np.ascontiguousarray(tracks[2], np.int32)
    ids = np.ascontiguousarray(ids, np.int32)
    T = len(offsets) - 1
    keep = []   # (the float32 (x, y) arrays must outlive the call)
    ptrs = (C.c_void_p * max(len(ids), 1))()
    for k, i in enumerate(ids):
        a = kps[int(i)] if isinstance(kps, dict) else kps[k]
        if a is None:
            ptrs[k] = None
            continue
        a = np.ascontiguousarray(np.asarray(a, np.float32)[:, :2])
        keep.append(a)
        ptrs[k] = a.ctypes.data
    pid, tab = as_pose_list(poses)
    tab = np.concatenate([tab, np.zeros(1, _lib.POSE_RT)])
    camv = np.asarray(tuple(cam) + (0.0,) * (8 - len(cam)), np.float64)
    pts = np.zeros(max(T, 1), points.dtype)
    pts[:T] = points
    res = np.zeros(max(len(img), 1), np.float64)
    res[:len(img)] = residuals
    m = None if mask is None else np.ascontiguousarray(np.concatenate([mask, np.zeros(1, np.uint8)]), np.uint8)
    fx = np.ascontiguousarray(list(fixed) + [0], np.int32)
    rec = np.zeros(len(pid) + 1, _lib.POSE_REFINEMENT)
    tr = np.zeros(len(pid) + 1, TRACE)
    c9, c2 = np.zeros(9, np.int64), np.zeros(2, np.float64)
    rc = host.host_refine_poses(offsets.ctypes.data, img.ctypes.data, idx.ctypes.data, T, ids.ctypes.data, len(ids), C.cast(ptrs, C.c_void_p),
                                pid.ctypes.data, tab.ctypes.data, len(pid), camv.ctypes.data_as(DP), float(thresholds[0]),
                                float(thresholds[1]), float(params[1]), int(params[0]), int(params[2]), fx.ctypes.data, len(fx) - 1,
                                pts.ctypes.data, res.ctypes.data, None if m is None else m.ctypes.data, rec.ctypes.data, c9.ctypes.data,
                                c2.ctypes.data, tr.ctypes.data if trace else None)
    assert rc == 0, rc
    counts = dict(zip(COUNT_KEYS, (int(v) for v in c9)))
    counts.update(zip(COST_KEYS, (float(v) for v in c2)))
    out = (pts[:T], res[:len(img)], (pid, tab[:len(pid)]), rec[:len(pid)], counts)
    return out + (tr[:len(pid)],) if trace else out
