"""ctypes driver of the two-view geometry's host twin (host/GeometricVerification.cpp, TwoViewGeometry, and the pieces of
csrc/msfm_pose.h, through libmsfm_host.so), and the twin's records over the unverified lists of a context, pair by pair on a thread
pool as tests/verify_twin.py runs the masks."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import twin_host
from twin_host import DP, FP, UP, WORKERS

# msfm_two_view_record (include/msfm_match.h): 144 bytes, no implicit padding
RECORD = np.dtype([("valid", "<i4"), ("reserved", "<i4"), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("n_kept", "<i4"),
                   ("n_positive_depth", "<i4"), ("n_triangulated", "<i4"), ("is_initial_candidate", "<i4"),
                   ("median_tri_angle", "<f8"), ("mean_tri_angle", "<f8"), ("mean_residual", "<f8")])
assert RECORD.itemsize == 144
DEFAULTS = (100, 2.0, 4.0)   # min_num_inliers, tri_max_error (px), tri_min_angle (degrees): the reference's


load_host = twin_host.load


def _dp(a):
    return a.ctypes.data_as(DP)


def decompose(host, E):
    """-> [(R, t)] * 4 or None"""
    E = np.ascontiguousarray(E, np.float64).reshape(9)
    out = np.zeros(48)
    if not host.host_pose_decompose(_dp(E), _dp(out)):
        return None
    return [(out[12 * c:12 * c + 9].reshape(3, 3).copy(), out[12 * c + 9:12 * c + 12].copy()) for c in range(4)]


def triangulate(host, R, t, x1, y1, x2, y2):
    P = np.r_[np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)]
    X = np.zeros(3)
    return X if host.host_pose_triangulate(_dp(P), x1, y1, x2, y2, _dp(X)) else None


def evaluate(host, R, t, f, x1, y1, x2, y2):
    P = np.r_[np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)]
    out = np.zeros(3)
    host.host_pose_evaluate(_dp(P), f, x1, y1, x2, y2, _dp(out))
    return bool(out[0]), float(out[1]), float(out[2])


def acos(host, x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(x)
    host.host_pose_acos(_dp(x), len(x), _dp(out))
    return out


def normalise(host, cam, p):
    """The twin's own normalised coordinates (msfm_emat::undistort) of the float32 pixel points p (n x 2) -> n x 2 doubles"""
    cam = np.asarray(tuple(cam) + (0.0,) * (8 - len(cam)), np.float64)
    uv = np.ascontiguousarray(np.asarray(p, np.float32).reshape(-1, 2), np.float64)
    xy = np.zeros_like(uv)
    host.host_emat_undistort(_dp(cam), _dp(uv), len(uv), _dp(xy))
    return xy


def kept_angles(host, rec, p1, p2, cam):
    """The per-match angles (degrees) of the kept pixel matches p1, p2 under the pose of the record `rec`, as the record's own
    statistics saw them: the twin's normalisation, msfm_pose::evaluate, the focal length (fx + fy) / 2."""
    q1, q2 = normalise(host, cam, p1), normalise(host, cam, p2)
    f = (cam[0] + cam[1]) * 0.5
    return [evaluate(host, rec["R"], rec["t"], f, *a, *b)[2] for a, b in zip(q1, q2)]


def median_rule(values):
    """The record's median: the middle entry of the sorted values, or the mean of the two middle ones."""
    v = sorted(values)
    n = len(v)
    return v[n // 2] if n % 2 else (v[(n - 1) // 2] + v[n // 2]) / 2


def record(host, E, q1, q2, f, params=DEFAULTS):
    """msfm_pose::two_view_record on the winner E and the kept matches q1, q2 (n x 2, normalised) -> (record, winner index)"""
    E = np.ascontiguousarray(E, np.float64).reshape(9)
    q1 = np.asarray(q1, np.float64).reshape(-1, 2)
    q2 = np.asarray(q2, np.float64).reshape(-1, 2)
    cols = [np.ascontiguousarray(a) for a in (q1[:, 0], q1[:, 1], q2[:, 0], q2[:, 1])]
    rec = np.zeros(1, RECORD)
    w = host.host_pose_record(_dp(E), *[_dp(c) for c in cols], len(q1), f, int(params[0]), float(params[1]), float(params[2]),
                              rec.ctypes.data)
    return rec[0], w


def geometry(host, p1, p2, cam, params=DEFAULTS, threshold=3.0, confidence=0.99, max_iters=1000, seed=0x5EED5EED):
    """TwoViewGeometry on pixel points p1, p2 (n x 2) -> (mask as bool[n], record)"""
    n = len(p1)
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    cam = np.asarray(tuple(cam) + (0.0,) * (8 - len(cam)), np.float64)
    mask = np.zeros(max(n, 1), np.uint8)
    rec = np.zeros(1, RECORD)
    k = host.host_two_view_geometry(p1.ctypes.data_as(FP), p2.ctypes.data_as(FP), n, _dp(cam), int(params[0]), float(params[1]),
                                    float(params[2]), threshold, confidence, max_iters, seed, mask.ctypes.data_as(UP), rec.ctypes.data)
    return (mask[:k].astype(bool) if k else np.zeros(n, bool)), rec[0]


def run(host, raw, pairs, kps, cam, params=DEFAULTS, threshold=3.0, confidence=0.99, max_iters=1000, seed=0x5EED5EED):
    """raw: (offsets, qt, dist) of ctx.match_pairs(pairs) on the context whose images have keypoints kps[id] -> the records the
    device must give for the verified call under model 1 without the selection (RECORD array, one per pair)."""
    offs, qt, _ = raw

    def one(p):
        i, j = pairs[p]
        s, e = offs[p], offs[p + 1]
        return geometry(host, kps[i][qt[s:e, 0], :2], kps[j][qt[s:e, 1], :2], cam, params, threshold, confidence, max_iters, seed)[1]

    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        res = list(pool.map(one, range(len(pairs))))
    out = np.zeros(len(pairs), RECORD)
    for p, r in enumerate(res):
        out[p] = r
    return out
