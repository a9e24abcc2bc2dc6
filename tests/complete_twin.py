"""ctypes driver of the map completion's host twin (csrc/msfm_complete.h, CompletePoints, through libmsfm_host.so): the records,
residuals, inlier bytes and counters the device must give after msfm_complete_points, computed in slices on a thread pool as
tests/filter_twin.py runs its twin.  Test infrastructure only."""
import numpy as np

import twin_host as th

COUNT_KEYS = ("eligible", "candidates", "admitted", "rejected_by_depth", "rejected_by_error", "completed")
ALL_KEYS = COUNT_KEYS + ("succeeded", "observations_used")
KIND_NOT_ELIGIBLE, KIND_UNTOUCHED, KIND_COMPLETED = 0, 1, 2
# msfm_cmp::Trace: the route a track took (csrc/msfm_complete.h)
TRACE = np.dtype([(k, np.int32) for k in ("kind", "candidates", "admitted", "rejected_by_depth")])
assert TRACE.itemsize == 16
load_host = th.load


def run(host, tracks, ids, kps, pose_list, cam, points, residuals, mask=None, thresholds=(2.0, 1.5), max_error=None, scope=(), select=None,
        workers=th.WORKERS, trace=False):
    """tracks (with `consistent`), ids, kps, cam as triangulation_twin.run takes them; pose_list: the session's current poses (a dict or
    an (ids, POSE_RT) pair); points, residuals (and mask, where the session has inlier bytes): the state before the call -- they are NOT
    changed; thresholds = (max_error, min_angle) of the triangulation that made the points; max_error: the call's, None = the
    session's; scope: the listed image ids (empty: every image).
    -> (POINT3D array [T], residuals [O], inlier bytes [O], dict of ALL_KEYS); with trace=True a fifth value, the TRACE array."""
    sid = np.asarray([int(i) for i in scope] + [0], np.int32)
    call = float(thresholds[0] if max_error is None else max_error)
    packed = th.pack(tracks, ids, kps, pose_list, cam, thresholds, points, residuals, mask, exact=True)
    return th.edit(host.twin_complete_points, (sid.ctypes.data, len(sid) - 1, call), COUNT_KEYS, TRACE, packed, select, workers, trace)
