"""ctypes driver of the map extension's host twin (csrc/msfm_extend.h, ExtendPoints, through libmsfm_host.so): the records, residuals,
inlier bytes, pose list and counters the device must give after msfm_extend_points, computed in slices on a thread pool as
tests/refine_points_twin.py runs its twin.  Test infrastructure only."""
import numpy as np

import twin_host as th
from monocularsfm_amd._lib import POSE_RT, TRI_EXTENDED, pose_table

COUNT_KEYS = ("tracks_touched", "continued", "observations_added", "observations_rejected", "created_attempted", "created", "retried")
KIND_UNTOUCHED, KIND_CONTINUE, KIND_CREATE = 0, 1, 2
ROUTE_NONE, ROUTE_PLAIN, ROUTE_ROBUST = 0, 1, 2
# msfm_ext::Trace: the route a track took (csrc/msfm_extend.h)
TRACE = np.dtype([(k, np.int32) for k in ("kind", "new_observations", "accepted", "route")])
assert TRACE.itemsize == 16
load_host = th.load


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
        workers=th.WORKERS, trace=False):
    """tracks (with `consistent`), ids, kps, cam as triangulation_twin.run takes them; pose_list: the session's poses before the call;
    new: the poses the call is given; points, residuals (and mask, where the session has inlier bytes): the state before the call --
    they are NOT changed; thresholds = (max_error, min_angle, min_views) of the triangulation that made the points.
    -> (POINT3D array [T], residuals [O], inlier bytes [O], dict of COUNT_KEYS plus images_added / succeeded / observations_used,
        the enlarged (ids, POSE_RT) list); with trace=True a sixth value, the TRACE array."""
    lst, got = enlarged(pose_list, new)
    gid = np.asarray(got + [0], np.int32)
    packed = th.pack(tracks, ids, kps, lst, cam, thresholds, points, residuals, mask, exact=True)
    out = th.edit(host.twin_extend_points, (gid.ctypes.data, len(got), int(max_hypotheses)), COUNT_KEYS, TRACE, packed, select, workers, trace,
                  extra=dict(images_added=len(got)))
    return out[:4] + (lst,) + out[4:]


def without_bit(points):
    """the records with MSFM_TRI_EXTENDED cleared: what a created track is compared with the full triangulation under"""
    p = np.array(points, copy=True)
    p["status"] &= ~TRI_EXTENDED
    return p
