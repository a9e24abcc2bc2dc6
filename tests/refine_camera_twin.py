"""ctypes driver of the camera refinement's host twin (csrc/msfm_refine_camera.h, RefineCamera, through libmsfm_host.so): the camera,
point records, residuals and counters the device must give after msfm_refine_camera.  One call, one thread: the one problem runs
through every track.  Test infrastructure only."""
import numpy as np

import refine_poses_twin as ptw
import twin_host as th
from twin_host import camera8  # noqa: F401  (the tests take it from here)

DEFAULTS = (10, 1e-6, 100)   # max_iters, step_tol, min_observations
FX_FY, F, CX_CY, K1_K2 = 1, 2, 4, 8
COUNT_KEYS = ("observations", "behind", "iterations", "accepted_steps", "stop", "refined", "rejected_by_inliers", "inliers_before",
              "inliers_after", "points_recalibrated", "points_lost", "points_gained")
COST_KEYS = ("cost_before", "cost_after")
STOP_NONE, STOP_STEP, STOP_MAX_ITERS, STOP_CEILING, STOP_FEW, STOP_NONFINITE = 0, 1, 2, 3, 4, 5
NOT_ELIGIBLE, NO_ACCEPTED_STEP, LOST_INLIERS = 1, 2, 3          # verdict: 0 stands, else why not
TRACE = ptw.TRACE
load_host = th.load


def reduce(host, v):
    """the summation order of csrc/msfm_refine_camera.h over the doubles v"""
    v = np.ascontiguousarray(v, np.float64)
    return float(host.host_rc_reduce(v.ctypes.data_as(th.DP), len(v)))


def run(host, tracks, ids, kps, poses, cam, points, residuals, mask=None, thresholds=(2.0, 1.5), params=DEFAULTS, cam_mask=FX_FY,
        trace=False):
    """tracks, ids, kps as triangulation_twin.run takes them; poses: see refine_poses_twin.as_pose_list; cam: the session's camera;
    points, residuals (and mask, after the robust call): the current records -- they are NOT changed; thresholds = (max_error,
    min_angle) of the triangulation; params = (max_iters, step_tol, min_observations); cam_mask: MSFM_CAM_* bits.
    -> (POINT3D array [T], residuals float64 [O], the camera as 8 floats, dict of COUNT_KEYS and COST_KEYS); with trace=True a fifth
    value, the one TRACE record."""
    block, st = th.pack(tracks, ids, kps, poses, cam, thresholds, points, residuals, mask)
    tr = np.zeros(1, TRACE)
    c12, c2 = np.zeros(12, np.int64), np.zeros(2, np.float64)
    rc = host.twin_refine_camera(block, float(params[1]), int(cam_mask), int(params[0]), int(params[2]), c12.ctypes.data, c2.ctypes.data,
                                 tr.ctypes.data if trace else None)
    assert rc == 0, rc
    counts = dict(zip(COUNT_KEYS, (int(v) for v in c12)))
    counts.update(zip(COST_KEYS, (float(v) for v in c2)))
    out = (st.points[:st.T], st.residuals[:st.O], tuple(float(v) for v in block.cam), counts)
    return out + (tr[0],) if trace else out
