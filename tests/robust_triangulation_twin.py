"""ctypes driver of the robust track triangulation's host twin (csrc/msfm_triangulate.h, TriangulateTracksRobust, through
libmsfm_host.so): the records, residuals, inlier bytes and counters the device must give, computed in slices on a thread pool as
tests/triangulation_twin.py runs the plain twin.  Test infrastructure only."""
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import triangulation_twin as tw
from monocularsfm_amd._lib import POINT3D, pose_table

DP = tw.DP
DEFAULTS = (2.0, 1.5, 2, 64)   # max_error (px), min_angle (degrees), min_views, max_hypotheses
ROBUST_KEYS = ("retried", "rescued", "observations_rejected", "hypotheses")
# msfm_tri::RobustTrace: the route a track took (csrc/msfm_triangulate.h)
TRACE = np.dtype([(k, np.int32) for k in ("retried", "m", "hypotheses", "winner", "best", "valid", "depth_rejected", "depth_rejected_best",
                                          "mask1", "mask2", "refit_stood", "flipped")])
assert TRACE.itemsize == 48


def load_host():
    L = tw.load_host()
    vp = C.c_void_p
    L.host_triangulate_tracks_robust.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, DP, C.c_double, C.c_double, C.c_int,
                                                 C.c_int, C.c_longlong, C.c_longlong, vp, vp, vp, vp]
    L.host_triangulate_tracks_robust_trace.argtypes = L.host_triangulate_tracks_robust.argtypes + [vp]
    L.host_tri_sample2.argtypes = [C.c_longlong, C.c_int, C.c_int, vp]
    return L


def run(host, tracks, ids, kps, poses, cam, params=DEFAULTS, select=None, workers=tw.WORKERS, trace=False):
    """As triangulation_twin.run, with params = (max_error, min_angle, min_views, max_hypotheses).
    -> (POINT3D array [T], residuals float64 [O], inlier bytes uint8 [O], dict of ROBUST_KEYS); with trace=True a fifth value, the TRACE
    array [T] (the same outputs otherwise: the trace changes nothing the twin computes)"""
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
    pid, tab = pose_table(poses)
    camv = np.asarray(tuple(cam) + (0.0,) * (8 - len(cam)), np.float64)
    pts = np.zeros(max(T, 1), POINT3D)
    res = np.zeros(max(len(img), 1), np.float64)
    mask = np.zeros(max(len(img), 1), np.uint8)
    tr = np.zeros(max(T, 1), TRACE)
    total = np.zeros(4, np.int64)
    lock = threading.Lock()

    def part(first, count):
        c4 = np.zeros(4, np.int64)
        rc = host.host_triangulate_tracks_robust_trace(offsets.ctypes.data, img.ctypes.data, idx.ctypes.data, cons.ctypes.data, ids.ctypes.data,
                                                       len(ids), C.cast(ptrs, C.c_void_p), pid.ctypes.data, tab.ctypes.data, len(pid),
                                                       camv.ctypes.data_as(DP), float(params[0]), float(params[1]), int(params[2]),
                                                       int(params[3]), first, count, pts.ctypes.data, res.ctypes.data, mask.ctypes.data,
                                                       c4.ctypes.data, tr.ctypes.data if trace else None)
        assert rc == 0, rc
        with lock:
            total[:] += c4

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
    out = (pts[:T], res[:len(img)], mask[:len(img)], dict(zip(ROBUST_KEYS, (int(v) for v in total))))
    return out + (tr[:T],) if trace else out


def sample2(host, track, h, m):
    out = np.zeros(2, np.int32)
    host.host_tri_sample2(int(track), int(h), int(m), out.ctypes.data)
    return [int(out[0]), int(out[1])]
