"""ctypes driver of the map visibility's host twin (csrc/msfm_visibility.h, MapVisibility, through libmsfm_host.so): the records, the
matrix and the counters the device must give for msfm_map_visibility, and the route function msfm_vis::vis_route.  Test infrastructure
only."""
import numpy as np

import twin_host as th
from monocularsfm_amd import _lib

COUNT_KEYS = ("tracks_counted", "elements_counted", "pair_increments")
ROUTE_KEYS = ("route", "lds_bytes", "matrix_in_lds", "wgs_per_cu")
BASES = {"tracks": _lib.VIS_TRACKS, "map": _lib.VIS_MAP}
load_host = th.load


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
    ids = sorted(int(i) for i in ids)
    n = len(ids)
    # (no pixel is read: no keypoints, any camera and thresholds)
    block, st = th.pack(tracks, ids, None, pose_list, (1.0, 1.0), (0.0, 0.0), points, None, None if mask is None else mask[:len(tracks[1])])
    if points is None or st.T == 0:
        block.points = None   # (NULL without records: the twin then reads status 0)
    if st.O == 0:
        block.mask = None
    q = np.asarray([int(i) for i in query] + [0], np.int32)
    rec = np.zeros(max(n, 1), _lib.VISIBILITY)
    mat = np.zeros((len(q) - 1, n), np.uint32)
    c3 = np.zeros(3, np.int64)
    rc = host.twin_map_visibility(block, q.ctypes.data, len(q) - 1, BASES[basis], rec.ctypes.data, mat.ctypes.data if mat.size else None,
                                  c3.ctypes.data)
    assert rc == expect, rc
    if expect:
        return None
    return rec[:n], mat, dict(zip(COUNT_KEYS, (int(v) for v in c3)))
