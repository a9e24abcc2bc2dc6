"""ctypes driver of the map filtering's host twin (csrc/msfm_filter.h, FilterPoints, through libmsfm_host.so): the records, residuals,
inlier bytes and counters the device must give after msfm_filter_points, computed in slices on a thread pool as tests/extend_twin.py
runs its twin.  Test infrastructure only."""
import numpy as np

import twin_host as th

COUNT_KEYS = ("eligible", "dropped_by_depth", "dropped_by_error", "trimmed", "regained", "removed_by_views", "removed_by_angle")
ALL_KEYS = COUNT_KEYS + ("succeeded", "observations_used")
KIND_NOT_ELIGIBLE, KIND_UNTOUCHED, KIND_TRIMMED, KIND_REMOVED_BY_VIEWS, KIND_REMOVED_BY_ANGLE = 0, 1, 2, 3, 4
# msfm_flt::Trace: the route a track took (csrc/msfm_filter.h)
TRACE = np.dtype([(k, np.int32) for k in ("kind", "dropped_by_depth", "dropped_by_error", "kept")])
assert TRACE.itemsize == 16
load_host = th.load


def run(host, tracks, ids, kps, pose_list, cam, points, residuals, mask=None, thresholds=(2.0, 1.5), params=None, scope=(), select=None,
        workers=th.WORKERS, trace=False):
    """tracks (with `consistent`), ids, kps, cam as triangulation_twin.run takes them; pose_list: the session's current poses (a dict or
    an (ids, POSE_RT) pair); points, residuals (and mask, where the session has inlier bytes): the state before the call -- they are NOT
    changed; thresholds = (max_error, min_angle) of the triangulation that made the points; params = the call's (max_error, min_angle),
    None = the session's; scope: the listed image ids (empty: every track).
    -> (POINT3D array [T], residuals [O], inlier bytes [O], dict of ALL_KEYS); with trace=True a fifth value, the TRACE array."""
    sid = np.asarray([int(i) for i in scope] + [0], np.int32)
    flt = tuple(thresholds[:2]) if params is None else tuple(params)
    packed = th.pack(tracks, ids, kps, pose_list, cam, thresholds, points, residuals, mask, exact=True)
    return th.edit(host.twin_filter_points, (sid.ctypes.data, len(sid) - 1, float(flt[0]), float(flt[1])), COUNT_KEYS, TRACE, packed, select,
                   workers, trace)
