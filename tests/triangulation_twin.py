"""ctypes driver of the track triangulation's host twin (csrc/msfm_triangulate.h, TriangulateTracks, through libmsfm_host.so): the
records and residuals the device must give for a finished track result, computed in slices on a thread pool as tests/pose_twin.py runs
the two-view records.  Test infrastructure only."""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DP = C.POINTER(C.c_double)
WORKERS = 16

# msfm_pose_rt (104 bytes) and msfm_point3d (48 bytes) of include/msfm_match.h: the binding's dtypes and its pose-list builder, not copies
from monocularsfm_amd._lib import POINT3D, POSE_RT, pose_table  # noqa: E402

assert POSE_RT.itemsize == 104 and POINT3D.itemsize == 48
DEFAULTS = (2.0, 1.5, 2)   # max_error (px), min_angle (degrees), min_views: Triangulator::Parameters
COUNT_KEYS = ("attempted", "with_point", "error_ok", "angle_ok", "depth_ok", "succeeded", "observations_used")


def load_host():
    subprocess.check_call(["make", "-C", HOST, "-s", "libmsfm_host.so"])
    L = C.CDLL(os.path.join(HOST, "libmsfm_host.so"))
    vp = C.c_void_p
    L.host_triangulate_tracks.argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, DP, C.c_double, C.c_double, C.c_int,
                                          C.c_longlong, C.c_longlong, vp, vp]
    L.host_tri_centre.argtypes = [DP, DP, DP]
    L.host_tri_parallax.argtypes = [DP, DP, DP]
    L.host_tri_parallax.restype = C.c_double
    return L


def run(host, tracks, ids, kps, poses, cam, params=DEFAULTS, select=None, workers=WORKERS):
    """tracks = (offsets, image_ids, point_idx, consistent) of a finished session over the declared images `ids`; kps: dict or sequence
    (by position in ids) of n x (>= 2) keypoint arrays (None allowed for unposed images); poses: dict id -> (R, t) / None.
    select: None (every track) or an iterable of track numbers -- only those are computed, the others stay zero.
    -> (POINT3D array [T], residuals float64 [O])"""
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

    def part(first, count):
        rc = host.host_triangulate_tracks(offsets.ctypes.data, img.ctypes.data, idx.ctypes.data, cons.ctypes.data, ids.ctypes.data, len(ids),
                                          C.cast(ptrs, C.c_void_p), pid.ctypes.data, tab.ctypes.data, len(pid), camv.ctypes.data_as(DP),
                                          float(params[0]), float(params[1]), int(params[2]), first, count, pts.ctypes.data, res.ctypes.data)
        assert rc == 0, rc

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
    return pts[:T], res[:len(img)]


def counts(points):
    """The integer fields of msfm_triangulation_stats from a POINT3D array (COUNT_KEYS)."""
    s = points["status"]
    ok = (s & 14) == 14
    return dict(attempted=int(((s & 1) != 0).sum()), with_point=int(((s & 2) != 0).sum()), error_ok=int(((s & 4) != 0).sum()),
                angle_ok=int(((s & 8) != 0).sum()), depth_ok=int(((s & 16) != 0).sum()), succeeded=int(ok.sum()),
                observations_used=int(points["n_views"].sum()))


def centre(host, R, t):
    R = np.ascontiguousarray(R, np.float64).reshape(9)
    t = np.ascontiguousarray(t, np.float64).reshape(3)
    out = np.zeros(3)
    host.host_tri_centre(R.ctypes.data_as(DP), t.ctypes.data_as(DP), out.ctypes.data_as(DP))
    return out


def parallax(host, X, Oi, Oj):
    a = [np.ascontiguousarray(v, np.float64).reshape(3) for v in (X, Oi, Oj)]
    return float(host.host_tri_parallax(*[v.ctypes.data_as(DP) for v in a]))
