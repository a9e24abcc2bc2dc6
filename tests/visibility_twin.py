"""ctypes driver of the map visibility's host twin (csrc/msfm_visibility.h, MapVisibility, through libmsfm_host.so): the records, the
matrix and the counters the device must give for msfm_map_visibility, and the route function msfm_vis::vis_route.  Test infrastructure
only."""
import ctypes as C

import numpy as np

import complete_twin as ctw
import refine_poses_twin as ptw
from monocularsfm_amd import _lib

COUNT_KEYS = ("tracks_counted", "elements_counted", "pair_increments")
ROUTE_KEYS = ("route", "lds_bytes", "matrix_in_lds", "wgs_per_cu")
BASES = {"tracks": _lib.VIS_TRACKS, "map": _lib.VIS_MAP}


def load_host():
    L = ctw.load_host()   # (the other twins' exports as well: the visibility counts their outputs)
    vp = C.c_void_p
    L.host_map_visibility.argtypes = [vp, vp, vp, C.c_longlong, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    L.host_map_visibility.restype = C.c_int
    L.host_vis_route.argtypes = [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, C.c_longlong, vp]
    L.host_vis_route.restype = None
    return L


def route(host, want, n, n_query, T, O):
    """msfm_vis::vis_route -> dict of ROUTE_KEYS (route 0: ROUTE_LDS was asked for and does not fit)."""
    out = np.zeros(4, np.int32)
    host.host_vis_route(int(want), int(n), int(n_query), int(T), int(O), out.ctypes.data)
    return dict(zip(ROUTE_KEYS, (int(v) for v in out)))


def run(host, tracks, ids, pose_list=None, points=None, mask=None, query=(), basis="map", expect=0):
    """tracks (with `consistent`) as triangulation_twin.run takes them; ids: the declared images (any order: the twin ranks them by
    ascending id, as the session does); pose_list: the session's current poses (a dict or an (ids, POSE_RT) pair; None without one);
    points: the records (None under basis "tracks"); mask: the session's inlier bytes or None; query: the listed ids.
    -> (VISIBILITY array [n], matrix uint32 [len(query), n], dict of COUNT_KEYS); with expect != 0 the twin's return code is asserted
    and None returned."""
    offsets = np.ascontiguousarray(tracks[0], np.int64)
    img = np.ascontiguousarray(tracks[1], np.int32)
    cons = np.ascontiguousarray(tracks[3], np.uint8)
    ids = np.ascontiguousarray(sorted(int(i) for i in ids), np.int32)
    T, n = len(offsets) - 1, len(ids)
    if pose_list is None:
        pid, tab = np.zeros(1, np.int32), np.zeros(1, _lib.POSE_RT)
        n_poses = 0
    else:
        pid, tab = ptw.as_pose_list(pose_list)
        n_poses = len(pid)
        pid = np.concatenate([pid, np.zeros(1, np.int32)])
        tab = np.concatenate([tab, np.zeros(1, tab.dtype)])
    q = np.asarray([int(i) for i in query] + [0], np.int32)
    pts = None if points is None else np.ascontiguousarray(points[:T], _lib.POINT3D)
    m = None if mask is None else np.ascontiguousarray(mask[:len(img)], np.uint8)
    rec = np.zeros(max(n, 1), _lib.VISIBILITY)
    mat = np.zeros((len(q) - 1, n), np.uint32)
    c3 = np.zeros(3, np.int64)
    rc = host.host_map_visibility(offsets.ctypes.data, img.ctypes.data, cons.ctypes.data, T, ids.ctypes.data, n, pid.ctypes.data,
                                  tab.ctypes.data, n_poses, q.ctypes.data, len(q) - 1, BASES[basis],
                                  None if pts is None or len(pts) == 0 else pts.ctypes.data,
                                  None if m is None or len(m) == 0 else m.ctypes.data, rec.ctypes.data,
                                  mat.ctypes.data if mat.size else None, c3.ctypes.data)
    assert rc == expect, rc
    if expect:
        return None
    return rec[:n], mat, dict(zip(COUNT_KEYS, (int(v) for v in c3)))
