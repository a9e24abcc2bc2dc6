"""ctypes driver of the point refinement's host twin (csrc/msfm_refine.h, RefinePoints, through libmsfm_host.so): the records,
residuals and counters the device must give after msfm_refine_points, computed in slices on a thread pool as
tests/triangulation_twin.py runs the plain twin.  Test infrastructure only."""
import numpy as np

import twin_host as th

DEFAULTS = (10, 1e-10)   # max_iters, step_tol
COUNT_KEYS = ("eligible", "refined", "gained_error_ok", "rejected_by_verdict", "iterations")
COST_KEYS = ("cost_before", "cost_after")
STOP_NONE, STOP_STEP, STOP_MAX_ITERS, STOP_CEILING = 0, 1, 2, 3
NOT_ELIGIBLE, NO_ACCEPTED_STEP = 1, 2          # verdict: 0 stands, these two, else the status bits that would have been cleared
# msfm_ref::Trace: the route a track took (csrc/msfm_refine.h)
TRACE = np.dtype([("steps", np.int32), ("accepted", np.int32), ("stop", np.int32), ("verdict", np.int32),
                  ("accepted_after_rejected", np.int32), ("depth_rejected", np.int32), ("lambda", np.float64), ("cost", np.float64)])
assert TRACE.itemsize == 40
load_host = th.load


def run(host, tracks, ids, kps, poses, cam, points, residuals, mask=None, thresholds=(2.0, 1.5), params=DEFAULTS, select=None,
        workers=th.WORKERS, trace=False):
    """tracks, ids, kps, poses, cam as triangulation_twin.run takes them; points, residuals (and mask, after the robust call): the
    outputs of the triangulation twin or of an earlier run() -- they are NOT changed; thresholds = (max_error, min_angle) of that
    triangulation; params = (max_iters, step_tol).
    -> (POINT3D array [T], residuals float64 [O], dict of COUNT_KEYS and COST_KEYS); with trace=True a fourth value, the TRACE array."""
    block, st = th.pack(tracks, ids, kps, poses, cam, thresholds, points, residuals, mask)
    tr = np.zeros(max(st.T, 1), TRACE)

    def part(first, count):
        c5, c2 = np.zeros(5, np.int64), np.zeros(2, np.float64)
        rc = host.twin_refine_points(th.sliced(block, first, count), float(params[1]), int(params[0]), c5.ctypes.data, c2.ctypes.data,
                                     tr.ctypes.data if trace else None)
        assert rc == 0, rc
        return c5, c2

    # (the slices' costs in track order)
    c5, c2 = th.total(th.run_sliced(st.T, part, select, workers), np.zeros(5, np.int64), np.zeros(2, np.float64))
    counts = dict(zip(COUNT_KEYS, (int(v) for v in c5)))
    counts.update(zip(COST_KEYS, (float(v) for v in c2)))
    out = (st.points[:st.T], st.residuals[:st.O], counts)
    return out + (tr[:st.T],) if trace else out
