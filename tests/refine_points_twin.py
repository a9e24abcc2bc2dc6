"""ctypes driver of the point refinement's host twin (csrc/msfm_refine.h, RefinePoints, through libmsfm_host.so): the records,
residuals and counters the device must give after msfm_refine_points, computed in slices on a thread pool as
tests/triangulation_twin.py runs the plain twin.  Test infrastructure only."""
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import robust_triangulation_twin as robtw
import triangulation_twin as tw
from monocularsfm_amd._lib import pose_table

DP = tw.DP
DEFAULTS = (10, 1e-10)   # max_iters, step_tol
COUNT_KEYS = ("eligible", "refined", "gained_error_ok", "rejected_by_verdict", "iterations")
COST_KEYS = ("cost_before", "cost_after")
STOP_NONE, STOP_STEP, STOP_MAX_ITERS, STOP_CEILING = 0, 1, 2, 3
NOT_ELIGIBLE, NO_ACCEPTED_STEP = 1, 2          # verdict: 0 stands, these two, else the status bits that would have been cleared
# msfm_ref::Trace: the route a track took (csrc/msfm_refine.h)
TRACE = np.dtype([("steps", np.int32), ("accepted", np.int32), ("stop", np.int32), ("verdict", np.int32),
                  ("accepted_after_rejected", np.int32), ("depth_rejected", np.int32), ("lambda", np.float64), ("cost", np.float64)])
assert TRACE.itemsize == 40


def load_host():
    L = robtw.load_host()   # (the plain and the robust twins' exports as well: the refinement starts from their outputs)
    vp = C.c_void_p
    L.host_refine_points.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, DP, C.c_double, C.c_double, C.c_double, C.c_int,
                                     C.c_longlong, C.c_longlong, vp, vp, vp, vp, vp, vp]
    return L


def run(host, tracks, ids, kps, poses, cam, points, residuals, mask=None, thresholds=(2.0, 1.5), params=DEFAULTS, select=None,
        workers=tw.WORKERS, trace=False):
    """tracks, ids, kps, poses, cam as triangulation_twin.run takes them; points, residuals (and mask, after the robust call): the
    outputs of the triangulation twin or of an earlier run() -- they are NOT changed; thresholds = (max_error, min_angle) of that
    triangulation; params = (max_iters, step_tol).
    -> (POINT3D array [T], residuals float64 [O], dict of COUNT_KEYS and COST_KEYS); with trace=True a fourth value, the TRACE array."""
    offsets = np.ascontiguousarray(tracks[0], np.int64)
    img = np.ascontiguousarray(tracks[1], np.int32)
    idx = np.ascontiguousarray(tracks[2], np.int32)
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
    pid, tab = pose_table(poses)
    camv = np.asarray(tuple(cam) + (0.0,) * (8 - len(cam)), np.float64)
    pts = np.zeros(max(T, 1), points.dtype)
    pts[:T] = points
    res = np.zeros(max(len(img), 1), np.float64)
    res[:len(img)] = residuals
    m = None if mask is None else np.ascontiguousarray(np.concatenate([mask, np.zeros(1, np.uint8)]), np.uint8)
    tr = np.zeros(max(T, 1), TRACE)
    parts = {}
    lock = threading.Lock()

    def part(first, count):
        c5, c2 = np.zeros(5, np.int64), np.zeros(2, np.float64)
        rc = host.host_refine_points(offsets.ctypes.data, img.ctypes.data, idx.ctypes.data, ids.ctypes.data, len(ids),
                                     C.cast(ptrs, C.c_void_p), pid.ctypes.data, tab.ctypes.data, len(pid), camv.ctypes.data_as(DP),
                                     float(thresholds[0]), float(thresholds[1]), float(params[1]), int(params[0]), first, count,
                                     pts.ctypes.data, res.ctypes.data, None if m is None else m.ctypes.data, c5.ctypes.data,
                                     c2.ctypes.data, tr.ctypes.data if trace else None)
        assert rc == 0, rc
        with lock:
            parts[first] = (c5, c2)

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
    c5, c2 = np.zeros(5, np.int64), np.zeros(2, np.float64)
    for first in sorted(parts):   # (the slices' costs in track order)
        c5 += parts[first][0]
        c2 += parts[first][1]
    counts = dict(zip(COUNT_KEYS, (int(v) for v in c5)))
    counts.update(zip(COST_KEYS, (float(v) for v in c2)))
    out = (pts[:T], res[:len(img)], counts)
    return out + (tr[:T],) if trace else out
