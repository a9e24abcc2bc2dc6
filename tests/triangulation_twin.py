"""ctypes driver of the track triangulation's host twin (csrc/msfm_triangulate.h, TriangulateTracks, through libmsfm_host.so): the
records and residuals the device must give for a finished track result, computed in slices on a thread pool as tests/pose_twin.py runs
the two-view records.  Test infrastructure only."""
import numpy as np

import twin_host as th
from twin_host import DP, POINT3D, POSE_RT, WORKERS  # noqa: F401  (the tests take the dtypes from here)

DEFAULTS = (2.0, 1.5, 2)   # max_error (px), min_angle (degrees), min_views: Triangulator::Parameters
COUNT_KEYS = ("attempted", "with_point", "error_ok", "angle_ok", "depth_ok", "succeeded", "observations_used")
load_host = th.load


def run(host, tracks, ids, kps, poses, cam, params=DEFAULTS, select=None, workers=WORKERS):
    """tracks = (offsets, image_ids, point_idx, consistent) of a finished session over the declared images `ids`; kps: dict or sequence
    (by position in ids) of n x (>= 2) keypoint arrays (None allowed for unposed images); poses: dict id -> (R, t) / None.
    select: None (every track) or an iterable of track numbers -- only those are computed, the others stay zero.
    -> (POINT3D array [T], residuals float64 [O])"""
    block, st = th.pack(tracks, ids, kps, poses, cam, params)

    def part(first, count):
        rc = host.twin_triangulate_tracks(th.sliced(block, first, count))
        assert rc == 0, rc

    th.run_sliced(st.T, part, select, workers)
    return st.points[:st.T], st.residuals[:st.O]


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
