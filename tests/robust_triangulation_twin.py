"""ctypes driver of the robust track triangulation's host twin (csrc/msfm_triangulate.h, TriangulateTracksRobust, through
libmsfm_host.so): the records, residuals, inlier bytes and counters the device must give, computed in slices on a thread pool as
tests/triangulation_twin.py runs the plain twin.  Test infrastructure only."""
import numpy as np

import twin_host as th

DEFAULTS = (2.0, 1.5, 2, 64)   # max_error (px), min_angle (degrees), min_views, max_hypotheses
ROBUST_KEYS = ("retried", "rescued", "observations_rejected", "hypotheses")
# msfm_tri::RobustTrace: the route a track took (csrc/msfm_triangulate.h)
TRACE = np.dtype([(k, np.int32) for k in ("retried", "m", "hypotheses", "winner", "best", "valid", "depth_rejected", "depth_rejected_best",
                                          "mask1", "mask2", "refit_stood", "flipped")])
assert TRACE.itemsize == 48
load_host = th.load


def run(host, tracks, ids, kps, poses, cam, params=DEFAULTS, select=None, workers=th.WORKERS, trace=False):
    """As triangulation_twin.run, with params = (max_error, min_angle, min_views, max_hypotheses).
    -> (POINT3D array [T], residuals float64 [O], inlier bytes uint8 [O], dict of ROBUST_KEYS); with trace=True a fifth value, the TRACE
    array [T] (the same outputs otherwise: the trace changes nothing the twin computes)"""
    block, st = th.pack(tracks, ids, kps, poses, cam, params[:3], mask=np.zeros(len(tracks[1]), np.uint8))
    tr = np.zeros(max(st.T, 1), TRACE)

    def part(first, count):
        c4 = np.zeros(4, np.int64)
        rc = host.twin_triangulate_tracks_robust(th.sliced(block, first, count), int(params[3]), c4.ctypes.data,
                                                 tr.ctypes.data if trace else None)
        assert rc == 0, rc
        return (c4,)

    (c4,) = th.total(th.run_sliced(st.T, part, select, workers), np.zeros(4, np.int64))
    out = (st.points[:st.T], st.residuals[:st.O], st.mask[:st.O], dict(zip(ROBUST_KEYS, (int(v) for v in c4))))
    return out + (tr[:st.T],) if trace else out


def sample2(host, track, h, m):
    out = np.zeros(2, np.int32)
    host.host_tri_sample2(int(track), int(h), int(m), out.ctypes.data)
    return [int(out[0]), int(out[1])]
