"""ctypes driver of the image registration's host twin (csrc/msfm_register.h, RegisterImages, through libmsfm_host.so): the records,
offsets, track ids, flags and residuals the device must give for a triangulated track result, computed in slices of the image list on
a thread pool.  Test infrastructure only."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import twin_host
from monocularsfm_amd._lib import POINT3D, REGISTRATION
from twin_host import DP, WORKERS

assert REGISTRATION.itemsize == 128
DEFAULTS = dict(max_error=4.0, confidence=0.9999, max_iters=1024, min_inliers=15, refine_iters=10)   # Registrant.h:22-26
ROUND = 64
load_host = twin_host.load


def sample3(host, image_id, it, n):
    out = np.zeros(3, np.int32)
    host.host_register_sample3(int(image_id), int(it), int(n), out.ctypes.data)
    return out


def p3p(host, u, v, X):
    """u, v: 3 normalised observations, X: 3 x 3 points -> list of (R 3 x 3, t 3)"""
    u, v, X = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (u, v, X))
    out = np.zeros(48)
    n = host.host_p3p(u.ctypes.data_as(DP), v.ctypes.data_as(DP), X.ctypes.data_as(DP), out.ctypes.data_as(DP))
    return [(out[12 * s:12 * s + 9].reshape(3, 3).copy(), out[12 * s + 9:12 * s + 12].copy()) for s in range(n)]


def refine(host, cu, cv, X, R, t, steps):
    a = [np.ascontiguousarray(v, np.float64) for v in (cu, cv, X[:, 0], X[:, 1], X[:, 2])]
    R, t = np.array(R, np.float64).reshape(9), np.array(t, np.float64).reshape(3)
    done = host.host_register_refine(*[v.ctypes.data_as(DP) for v in a], len(a[0]), int(steps), R.ctypes.data_as(DP), t.ctypes.data_as(DP))
    return R.reshape(3, 3), t, done


def run(host, tracks, points, list_ids, kps, cam, workers=WORKERS, **params):
    """tracks = (offsets, image_ids, point_idx, consistent) and points (POINT3D) of a triangulated session; kps: dict image id -> n x
    (>= 2) keypoints.  -> (REGISTRATION array, offsets int64 [n + 1], track ids int32, flags uint8, residuals float64)"""
    prm = dict(DEFAULTS, **params)
    offsets = np.ascontiguousarray(tracks[0], np.int64)
    img = np.ascontiguousarray(tracks[1], np.int32)
    idx = np.ascontiguousarray(tracks[2], np.int32)
    points = np.ascontiguousarray(points, POINT3D)
    ids = np.ascontiguousarray(list_ids, np.int32)
    n, T = len(ids), len(offsets) - 1
    keep = [np.ascontiguousarray(np.asarray(kps[int(i)], np.float32)[:, :2]) for i in ids]
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in keep])
    camv = np.asarray(tuple(cam) + (0.0,) * (8 - len(cam)), np.float64)
    counts = np.zeros(max(n, 1), np.int64)
    rc = host.host_register_counts(offsets.ctypes.data, img.ctypes.data, T, points.ctypes.data, ids.ctypes.data, n, counts.ctypes.data)
    assert rc == 0, rc
    out_off = np.concatenate([[0], np.cumsum(counts[:n])]).astype(np.int64)
    M = int(out_off[-1])
    rec = np.zeros(max(n, 1), REGISTRATION)
    tid, flags, res = np.zeros(max(M, 1), np.int32), np.zeros(max(M, 1), np.uint8), np.zeros(max(M, 1), np.float64)

    def part(first, count):
        rc = host.host_register_images(offsets.ctypes.data, img.ctypes.data, idx.ctypes.data, T, points.ctypes.data, ids.ctypes.data, n,
                                       C.cast(ptrs, C.c_void_p), camv.ctypes.data_as(DP), float(prm["max_error"]), float(prm["confidence"]),
                                       int(prm["max_iters"]), int(prm["min_inliers"]), int(prm["refine_iters"]), out_off.ctypes.data, first, count,
                                       rec.ctypes.data, tid.ctypes.data, flags.ctypes.data, res.ctypes.data)
        assert rc == 0, rc

    step = max(1, (n + workers - 1) // workers)
    jobs = [(f, min(step, n - f)) for f in range(0, n, step)]
    if len(jobs) <= 1 or workers <= 1:
        for j in jobs:
            part(*j)
    else:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            list(pool.map(lambda j: part(*j), jobs))
    return rec[:n], out_off, tid[:M], flags[:M], res[:M]


def schedule(records, max_iters=DEFAULTS["max_iters"]):
    """What the staged device form runs for these records: (rounds any image ran, hypotheses solved)."""
    h = records["hypotheses"].astype(np.int64)
    return int(((h + ROUND - 1) // ROUND).max(initial=0)), int(h.sum())
