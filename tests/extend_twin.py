"""ctypes driver of the map extension's host twin (csrc/msfm_extend.h, ExtendPoints, through libmsfm_host.so): the records, residuals,
inlier bytes, pose list and counters the device must give after msfm_extend_points, computed in slices on a thread pool as
tests/refine_points_twin.py runs its twin.  Test infrastructure only."""
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import refine_poses_twin as ptw
import triangulation_twin as tw
from monocularsfm_amd._lib import POSE_RT, TRI_EXTENDED, pose_table

DP = tw.DP
COUNT_KEYS = ("tracks_touched", "continued", "observations_added", "observations_rejected", "created_attempted", "created", "retried")
KIND_UNTOUCHED, KIND_CONTINUE, KIND_CREATE = 0, 1, 2
ROUTE_NONE, ROUTE_PLAIN, ROUTE_ROBUST = 0, 1, 2
# msfm_ext::Trace: the route a track took (csrc/msfm_extend.h)
TRACE = np.dtype([(k, np.int32) for k in ("kind", "new_observations", "accepted", "route")])
assert TRACE.itemsize == 16


def load_host():
    L = ptw.load_host()   # (the triangulation and refinement twins' exports as well: the extension starts from their outputs)
    vp = C.c_void_p
    L.host_extend_points.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, DP, C.c_double, C.c_double, C.c_int,
                                     C.c_int, C.c_longlong, C.c_longlong, vp, vp, vp, C.c_int, vp, vp]
    return L


def enlarged(pose_list, new):
    """The session's pose list after msfm_extend_points: `pose_list` (a dict or an (ids, POSE_RT) pair, as triangulate_tracks was given
    it) with the valid entries of `new` appended in the call's order, or replacing a valid == 0 entry in place.
    -> ((ids, POSE_RT table), the ids that gained a valid pose)"""
    pid, tab = pose_table(pose_list)
    nid, ntab = pose_table(new)
    pid, tab = list(int(i) for i in pid), [tab[k].copy() for k in range(len(pid))]
    got = []
    for k, i in enumerate(nid):
        if not ntab[k]["valid"]:
            continue
        p = ntab[k].copy()
        p["valid"], p["reserved"] = 1, 0
        if int(i) in pid:
            assert not tab[pid.index(int(i))]["valid"], "the image already has a pose"
            tab[pid.index(int(i))] = p
        else:
            pid.append(int(i))
            tab.append(p)
        got.append(int(i))
    out = np.zeros(len(pid), POSE_RT)
    for k, p in enumerate(tab):
        out[k] = p
    return (np.asarray(pid, np.int32), out), got


def run(host, tracks, ids, kps, pose_list, new, cam, points, residuals, mask=None, thresholds=(2.0, 1.5, 2), max_hypotheses=0, select=None,
        workers=tw.WORKERS, trace=False):
    """tracks (with `consistent`), ids, kps, cam as triangulation_twin.run takes them; pose_list: the session's poses before the call;
    new: the poses the call is given; points, residuals (and mask, where the session has inlier bytes): the state before the call --
    they are NOT changed; thresholds = (max_error, min_angle, min_views) of the triangulation that made the points.
    -> (POINT3D array [T], residuals [O], inlier bytes [O], dict of COUNT_KEYS plus images_added / succeeded / observations_used,
        the enlarged (ids, POSE_RT) list); with trace=True a sixth value, the TRACE array."""
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
    (pid, tab), got = enlarged(pose_list, new)
    gid = np.asarray(got + [0], np.int32)
    camv = np.asarray(tuple(cam) + (0.0,) * (8 - len(cam)), np.float64)
    # sized exactly: an index past a track's own slots leaves the arrays
    pts = np.array(points[:T], copy=True)
    res = np.array(residuals[:len(img)], np.float64, copy=True)
    m = np.zeros(len(img), np.uint8) if mask is None else np.array(mask[:len(img)], np.uint8, copy=True)
    tr = np.zeros(max(T, 1), TRACE)
    total = np.zeros(7, np.int64)
    lock = threading.Lock()

    def part(first, count):
        c7 = np.zeros(7, np.int64)
        rc = host.host_extend_points(offsets.ctypes.data, img.ctypes.data, idx.ctypes.data, cons.ctypes.data, ids.ctypes.data, len(ids),
                                     C.cast(ptrs, C.c_void_p), pid.ctypes.data, tab.ctypes.data, len(pid), gid.ctypes.data, len(got),
                                     camv.ctypes.data_as(DP), float(thresholds[0]), float(thresholds[1]), int(thresholds[2]),
                                     int(max_hypotheses), first, count, pts.ctypes.data, res.ctypes.data, m.ctypes.data,
                                     0 if mask is None else 1, c7.ctypes.data, tr.ctypes.data if trace else None)
        assert rc == 0, rc
        with lock:
            total[:] += c7

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
    counts["images_added"] = len(got)
    counts["succeeded"] = int(((pts["status"] & 14) == 14).sum())
    counts["observations_used"] = int(pts["n_views"].sum())
    out = (pts, res, m, counts, (pid, tab))
    return out + (tr[:T],) if trace else out


def without_bit(points):
    """the records with MSFM_TRI_EXTENDED cleared: what a created track is compared with the full triangulation under"""
    p = np.array(points, copy=True)
    p["status"] &= ~TRI_EXTENDED
    return p
