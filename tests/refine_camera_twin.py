"""ctypes driver of the camera refinement's host twin (csrc/msfm_refine_camera.h, RefineCamera, through libmsfm_host.so): the camera,
point records, residuals and counters the device must give after msfm_refine_camera.  One call, one thread: the one problem runs
through every track.  Test infrastructure only."""
import ctypes as C

import numpy as np

import refine_poses_twin as ptw
import triangulation_twin as tw
from monocularsfm_amd import _lib

DP = tw.DP
DEFAULTS = (10, 1e-6, 100)   # max_iters, step_tol, min_observations
FX_FY, F, CX_CY, K1_K2 = 1, 2, 4, 8
COUNT_KEYS = ("observations", "behind", "iterations", "accepted_steps", "stop", "refined", "rejected_by_inliers", "inliers_before",
              "inliers_after", "points_recalibrated", "points_lost", "points_gained")
COST_KEYS = ("cost_before", "cost_after")
STOP_NONE, STOP_STEP, STOP_MAX_ITERS, STOP_CEILING, STOP_FEW, STOP_NONFINITE = 0, 1, 2, 3, 4, 5
NOT_ELIGIBLE, NO_ACCEPTED_STEP, LOST_INLIERS = 1, 2, 3          # verdict: 0 stands, else why not
TRACE = ptw.TRACE


def load_host():
    L = ptw.load_host()   # (the triangulation, point and pose refinement twins' exports as well)
    vp = C.c_void_p
    L.host_refine_camera.argtypes = [vp, vp, vp, C.c_longlong, vp, C.c_int, vp, vp, vp, C.c_int, DP, C.c_double, C.c_double, C.c_double,
                                     C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.host_rc_reduce.argtypes = [DP, C.c_longlong]
    L.host_rc_reduce.restype = C.c_double
    return L


def camera8(cam):
    if isinstance(cam, dict):
        cam = tuple(cam[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"))
    return tuple(float(v) for v in cam) + (0.0,) * (8 - len(cam))


def reduce(host, v):
    """the summation order of csrc/msfm_refine_camera.h over the doubles v"""
    v = np.ascontiguousarray(v, np.float64)
    return float(host.host_rc_reduce(v.ctypes.data_as(DP), len(v)))


def run(host, tracks, ids, kps, poses, cam, points, residuals, mask=None, thresholds=(2.0, 1.5), params=DEFAULTS, cam_mask=FX_FY,
        trace=False):
    """tracks, ids, kps as triangulation_twin.run takes them; poses: see refine_poses_twin.as_pose_list; cam: the session's camera;
    points, residuals (and mask, after the robust call): the current records -- they are NOT changed; thresholds = (max_error,
    min_angle) of the triangulation; params = (max_iters, step_tol, min_observations); cam_mask: MSFM_CAM_* bits.
    -> (POINT3D array [T], residuals float64 [O], the camera as 8 floats, dict of COUNT_KEYS and COST_KEYS); with trace=True a fifth
    value, the one TRACE record."""
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
    pid, tab = ptw.as_pose_list(poses)
    tab = np.concatenate([tab, np.zeros(1, _lib.POSE_RT)])
    camv = np.asarray(camera8(cam), np.float64)
    pts = np.zeros(max(T, 1), points.dtype)
    pts[:T] = points
    res = np.zeros(max(len(img), 1), np.float64)
    res[:len(img)] = residuals
    m = None if mask is None else np.ascontiguousarray(np.concatenate([mask, np.zeros(1, np.uint8)]), np.uint8)
    tr = np.zeros(1, TRACE)
    c12, c2 = np.zeros(12, np.int64), np.zeros(2, np.float64)
    rc = host.host_refine_camera(offsets.ctypes.data, img.ctypes.data, idx.ctypes.data, T, ids.ctypes.data, len(ids), C.cast(ptrs, C.c_void_p),
                                 pid.ctypes.data, tab.ctypes.data, len(pid), camv.ctypes.data_as(DP), float(thresholds[0]),
                                 float(thresholds[1]), float(params[1]), int(cam_mask), int(params[0]), int(params[2]), pts.ctypes.data,
                                 res.ctypes.data, None if m is None else m.ctypes.data, c12.ctypes.data, c2.ctypes.data,
                                 tr.ctypes.data if trace else None)
    assert rc == 0, rc
    counts = dict(zip(COUNT_KEYS, (int(v) for v in c12)))
    counts.update(zip(COST_KEYS, (float(v) for v in c2)))
    out = (pts[:T], res[:len(img)], tuple(float(v) for v in camv), counts)
    return out + (tr[0],) if trace else out
