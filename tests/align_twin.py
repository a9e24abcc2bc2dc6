"""ctypes driver of the map alignment's host twins (csrc/msfm_align.h, EstimateAlignment / TransformMap, through libmsfm_host.so): the
record, the per-prior records, the poses, point records, residuals and counters the device must give after msfm_estimate_alignment and
msfm_transform_map; and AlignTwinContext, tests/twin_context.TwinContext with the three calls of _lib.Context.  Test infrastructure
only."""
import ctypes as C

import numpy as np

import twin_host as th
from monocularsfm_amd import _lib
from twin_context import TwinContext

COUNT_KEYS = ("poses_transformed", "points_transformed", "points_lost", "points_gained", "succeeded")
K_REFITS, K_MIN_SPREAD, K_ROUND = 4, 1e-6, 256
_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
_MP = C.POINTER(th.HostMap)
# the alignment's exports, declared here: tests/twin_host.EXPORTS is the table of the twins that existed before it
EXPORTS = {
    "twin_estimate_alignment": (_i, [_MP, _vp, _vp, _i, _d, _d, _i, _i, _vp, _vp]),
    "twin_transform_map": (_i, [_MP, _vp, _vp]),
    "host_aln_fit": (_i, [_vp, _i, _vp]),
}


def load_host():
    lib = th.load()
    for name, (restype, argtypes) in EXPORTS.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    return lib


def _invalid(what):
    return _lib.MsfmError(_lib.E_INVALID, what)


def fit(host, centres, positions):
    """the plain fit of the pairs (centre, position) in the header's summation order -> (valid, s, Q 3 x 3, d)"""
    pr = np.ascontiguousarray(np.concatenate([np.asarray(centres, np.float64).reshape(-1, 3), np.asarray(positions, np.float64).reshape(-1, 3)], 1))
    g = _lib.Similarity()
    ok = host.host_aln_fit(pr.ctypes.data, len(pr), C.addressof(g))
    return bool(ok), float(g.s), np.array(g.Q, np.float64).reshape(3, 3), np.array(g.d, np.float64)


def estimate(host, ids, poses, positions, max_error=None, confidence=0.9999, max_hypotheses=1024, min_inliers=3, listed=None):
    """ids: the declared images; poses: a dict or an (ids, POSE_RT) pair, the session's pose list; positions: {image id: (x, y, z)}, or
    with `listed` (ids int32, positions [n, 3]) in the caller's own order.  -> what _lib.Context.estimate_alignment returns
    (estimate_ms 0.0).  Raises MsfmError(E_INVALID) where the library does."""
    pid, pos = _lib.prior_table(positions) if listed is None else (np.ascontiguousarray(listed[0], np.int32),
                                                                   np.ascontiguousarray(listed[1], np.float64).reshape(-1, 3))
    block, held = th.pack((np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32)), ids, None, poses, (1.0, 1.0, 0.0, 0.0),
                          (0.0, 0.0))
    robust = max_error is not None
    out = _lib.Alignment()
    rec = np.zeros(max(len(pid), 1), _lib.ALIGNMENT_RESIDUAL)
    rc = host.twin_estimate_alignment(block, pid.ctypes.data if len(pid) else None, pos.ctypes.data if len(pid) else None, len(pid),
                                      float(max_error) if robust else 0.0, float(confidence), int(max_hypotheses) if robust else 0,
                                      int(min_inliers), C.addressof(out), rec.ctypes.data)
    if rc in (3, 4, 5):
        raise _invalid("twin_estimate_alignment: code %d" % rc)
    assert rc == 0, rc
    return _lib.alignment_dict(out), rec[:len(pid)]


def transform(host, tracks, ids, kps, poses, cam, points, residuals, mask, thresholds, s, Q, d):
    """tracks, ids, kps, poses, cam, points, residuals, mask, thresholds = (max_error, min_angle) as refine_camera_twin.run takes them
    (nothing given is changed).  -> ((pose ids, POSE_RT array), POINT3D array [T], residuals [O], dict of COUNT_KEYS).  Raises
    MsfmError(E_INVALID) where the library does; the error carries `held`, the twin's own copies."""
    block, held = th.pack(tracks, ids, kps, poses, cam, thresholds, points, residuals, mask)
    g = _lib.similarity_struct(s, Q, d)
    c5 = np.zeros(5, np.int64)
    rc = host.twin_transform_map(block, C.addressof(g), c5.ctypes.data)
    if rc == 3:
        err = _invalid("twin_transform_map: code 3")
        err.held = held   # the arrays the twin worked on: a test holds them against what it gave
        raise err
    assert rc == 0, rc
    return (held.pose_ids.copy(), held.poses.copy()), held.points[:held.T], held.residuals[:held.O], dict(zip(COUNT_KEYS, (int(v) for v in c5)))


class AlignTwinContext(TwinContext):
    """TwinContext with estimate_alignment, transform_map and align: the twins behind the first two, _lib.Context's own align"""
    align = _lib.Context.align

    def estimate_alignment(self, positions, max_error=None, confidence=0.9999, max_hypotheses=1024, min_inliers=3):
        self._need_map()
        return estimate(load_host(), self._session["ids"], self._pose_list, positions, max_error, confidence, max_hypotheses, min_inliers)

    def transform_map(self, s, Q, d):
        self._need_map()
        lst, pts, res, counts = transform(load_host(), *self._common(), self._pose_list, self._cam, self._points, self._residuals, self._mask,
                                          self._thr[:2], s, Q, d)
        self._pose_list, self._points, self._residuals = lst, pts.copy(), res.copy()
        self._changed()
        return counts
