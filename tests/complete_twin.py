"""ctypes driver of the map completion's host twin (csrc/msfm_complete.h, CompletePoints, through libmsfm_host.so): the records,
residuals, inlier bytes and counters the device must give after msfm_complete_points, computed in slices on a thread pool as
tests/filter_twin.py runs its twin.  Test infrastructure only."""
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import filter_twin as ftw
import refine_poses_twin as ptw
import triangulation_twin as tw

DP = tw.DP
COUNT_KEYS = ("eligible", "candidates", "admitted", "rejected_by_depth", "rejected_by_error", "completed")
ALL_KEYS = COUNT_KEYS + ("succeeded", "observations_used")
KIND_NOT_ELIGIBLE, KIND_UNTOUCHED, KIND_COMPLETED = 0, 1, 2
# msfm_cmp::Trace: the route a track took (csrc/msfm_complete.h)
TRACE = np.dtype([(k, np.int32) for k in ("kind", "candidates", "admitted", "rejected_by_depth")])
assert TRACE.itemsize == 16


def load_host():
    L = ftw.load_host()   # (the other twins' exports as well: the completion starts from their outputs)
    vp = C.c_void_p
    L.host_complete_points.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, DP, C.c_double, C.c_double, C.c_double,
                                       C.c_longlong, C.c_longlong, vp, vp, vp, C.c_int, vp, vp]
    L.host_complete_points.restype = C.c_int
    return L


def run(host, tracks, ids, kps, pose_list, cam, points, residuals, mask=None, thresholds=(2.0, 1.5), max_error=None, scope=(), select=None,
        workers=tw.WORKERS, trace=False):
    """tracks (with `consistent`), ids, kps, cam as triangulation_twin.run takes them; pose_list: the session's current poses (a dict or
    an (ids, POSE_RT) pair); points, residuals (and mask, where the session has inlier bytes): the state before the call -- they are NOT
    changed; thresholds = (max_error, min_angle) of the triangulation that made the points; max_error: the call's, None = the
    session's; scope: the listed image ids (empty: every image).
    -> (POINT3D array [T], residuals [O], inlier bytes [O], dict of ALL_KEYS); with trace=True a fifth value, the TRACE array."""
    offsets = np.ascontiguousarray(tracks[0], np.int64)
    img = np.ascontiguousarray(tracks[1], np.int32)
    idx = np.ascontiguousarray(tracks[2], np.int32)
    cons = np.ascontiguousarray(tracks[3], np.uint8)
    ids = np.ascontiguousarray(ids, np.int32)
    T = len(offsets) - 1
    keep = []   # (the float32 (x, y) arrays must outlive the calls)
    ptrs = (C.c_void_p * max(len(ids), 1))()
    for k, i in enumerate(ids):
        a = kps[int(i)] if isinstance(kps, dict) else kps[k]
        if a is None:
            ptrs[k] = None
            continue
        a = np.ascontiguousarray(np.asarray(a, np.float32)[:, :2])
        keep.append(a)
        ptrs[k] = a.ctypes.data
    pid, tab = ptw.as_pose_list(pose_list)
    tab = np.concatenate([tab, np.zeros(1, tab.dtype)])
    sid = np.asarray([int(i) for i in scope] + [0], np.int32)
    camv = np.asarray(tuple(cam) + (0.0,) * (8 - len(cam)), np.float64)
    call = float(thresholds[0] if max_error is None else max_error)
    # sized exactly: an index past a track's own slots leaves the arrays
    pts = np.array(points[:T], copy=True)
    res = np.array(residuals[:len(img)], np.float64, copy=True)
    m = np.zeros(len(img), np.uint8) if mask is None else np.array(mask[:len(img)], np.uint8, copy=True)
    tr = np.zeros(max(T, 1), TRACE)
    total = np.zeros(6, np.int64)
    lock = threading.Lock()

    def part(first, count):
        c6 = np.zeros(6, np.int64)
        rc = host.host_complete_points(offsets.ctypes.data, img.ctypes.data, idx.ctypes.data, cons.ctypes.data, ids.ctypes.data, len(ids),
                                       C.cast(ptrs, C.c_void_p), pid.ctypes.data, tab.ctypes.data, len(pid), sid.ctypes.data, len(sid) - 1,
                                       camv.ctypes.data_as(DP), float(thresholds[0]), float(thresholds[1]), call, first, count,
                                       pts.ctypes.data, res.ctypes.data, m.ctypes.data, 0 if mask is None else 1, c6.ctypes.data,
                                       tr.ctypes.data if trace else None)
        assert rc == 0, rc
        with lock:
            total[:] += c6

    if select is None:
        step = max(1, (T + 4 * workers - 1) // (4 * workers))
        jobs = [(f, min(step, T - f)) for f in range(0, T, step)]
    else:
        jobs = [(int(t), 1) for t in select]
    if len(jobs) <= 1 or workers <= 1:
        for j in jobs:
            part(*j)
    else:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(lambda j: part(*j), jobs))
    counts = dict(zip(COUNT_KEYS, (int(v) for v in total)))
    counts["succeeded"] = int(((pts["status"] & 14) == 14).sum())
    counts["observations_used"] = int(pts["n_views"].sum())
    out = (pts, res, m, counts)
    return out + (tr[:T],) if trace else out
