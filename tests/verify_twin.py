"""The host twins of the device verification (host/GeometricVerification.cpp through libmsfm_host.so) over the unverified lists of
a context, pair by pair on a thread pool: at production sizes the twins' loop over thousands of pairs is the test's cost.  ctypes
drops the GIL for the length of each foreign call and the twins keep no static state, so the pairs run in parallel.

run() returns what the device must give for the same call: the verified lists (offsets, qt, dist), the selection records (model,
nE, nH) and the predicted verification_stats() (solved, rounds) from host_staged_schedule -- the sum of the pairs' solved
hypotheses and the largest of their round counts; under the selection with model 0 the homography's alone (F is not staged), with
model 1 the essential matrix's and the homography's together."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import twin_host
from twin_host import DP, FP, IP, UP, WORKERS  # noqa: F401

load_host = twin_host.load


def _schedule(host, model, a, b, n, cam, threshold, confidence, max_iters, seed):
    rounds, solved = C.c_int(), C.c_longlong()
    rc = host.host_staged_schedule(model, a, b, n, cam, threshold, confidence, max_iters, seed, C.byref(rounds), C.byref(solved))
    assert rc == 0
    return solved.value, rounds.value


def _pair(host, model, select, cam, h_ratio, threshold, confidence, max_iters, seed, p1, p2):
    """-> (mask of the pair's n matches, record or None, [(solved, rounds) of each staged model run])"""
    n = len(p1)
    p1 = np.ascontiguousarray(p1, np.float32)
    p2 = np.ascontiguousarray(p2, np.float32)
    a, b = p1.ctypes.data_as(FP), p2.ctypes.data_as(FP)
    c = cam.ctypes.data_as(DP)
    mask = np.zeros(max(n, 1), np.uint8)
    m = mask.ctypes.data_as(UP)
    rec = None
    if select:
        r = np.zeros(3, np.int32)
        k = host.host_two_view_select(a, b, n, model, c if model == 1 else None, h_ratio, threshold, confidence, max_iters, seed, m,
                                      r.ctypes.data_as(IP))
        rec = tuple(int(v) for v in r)
        staged = ([1] if model == 1 else []) + [2]
    elif model == 1:
        k = host.host_essential_ransac(a, b, n, c, threshold, confidence, max_iters, seed, m)
        staged = [1]
    else:
        k = host.host_homography_ransac(a, b, n, threshold, confidence, max_iters, seed, m)
        staged = [2]
    keep = mask[:k].astype(bool) if k else np.zeros(n, bool)
    sched = [_schedule(host, s, a, b, n, c, threshold, confidence, max_iters, seed) for s in staged]
    return keep, rec, sched


def run(host, raw, pairs, kps, model, cam=None, select=False, h_ratio=0.7, threshold=3.0, confidence=0.99, max_iters=1000,
        seed=0x5eed5eed):
    """raw: (offsets, qt, dist) of ctx.match_pairs(pairs) on the context whose images have keypoints kps[id].  model: 1 or 2, or 0 /
    1 with select.  -> {"lists": (offsets, qt, dist), "records": (model, nE, nH) arrays or None, "stats": (solved, rounds),
    "schedule": per pair [(solved, rounds) of each staged model]}"""
    offs, qt, d = raw
    assert model in ((0, 1) if select else (1, 2))
    cam = np.asarray(tuple(cam) + (0.0,) * (8 - len(cam)) if cam is not None else (0.0,) * 8, np.float64)

    def one(p):
        i, j = pairs[p]
        s, e = offs[p], offs[p + 1]
        return _pair(host, model, select, cam, h_ratio, threshold, confidence, max_iters, seed, kps[i][qt[s:e, 0], :2],
                     kps[j][qt[s:e, 1], :2])

    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        res = list(pool.map(one, range(len(pairs))))
    keep = np.concatenate([r[0] for r in res]) if res else np.zeros(0, bool)
    out_off = np.zeros(len(pairs) + 1, np.int64)
    out_off[1:] = np.cumsum([int(r[0].sum()) for r in res])
    recs = None
    if select:
        r3 = np.asarray([r[1] for r in res], np.int32).reshape(-1, 3)
        recs = tuple(np.ascontiguousarray(r3[:, k]) for k in range(3))
    sched = [r[2] for r in res]
    solved = sum(s for ps in sched for s, _ in ps)
    rounds = max((r for ps in sched for _, r in ps), default=0)
    return {"lists": (out_off, qt[keep].reshape(-1, 2), d[keep]), "records": recs, "stats": (solved, rounds), "schedule": sched}
