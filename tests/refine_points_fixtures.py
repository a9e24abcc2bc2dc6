"""Inputs shared by the point refinement's CPU and GPU tests: a hand-built ring job (the cameras of
tests/test_gpu_robust_triangulation.ring_job, short tracks, 8 px of noise) on which Levenberg-Marquardt leaves the easy path, and the
search that names one track per route from the twin's trace.  Test infrastructure only."""
import numpy as np

import refine_points_twin as rtw
import triangulation_twin as tw

CAM = (2500.0, 2500.0, 1536.0, 1152.0)
ROUTE_THRESHOLDS = (12.0, 1.2)     # max_error (px) near the noise level, min_angle at the ring's 1.2 degrees between neighbours
ROUTE_PARAMS = (10, 1e-4)          # max_iters, step_tol
ROUTE_LENGTHS = [2, 3, 2, 5, 3, 2, 7, 4]
ERROR_OK, ANGLE_OK = 4, 8


def tracks_of(lengths, ids):
    """the track result of a ring job: track j runs through the images 0 .. lengths[j] - 1 at keypoint row j"""
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    img = np.concatenate([ids[:n] for n in lengths]).astype(np.int32)
    idx = np.concatenate([np.full(n, j) for j, n in enumerate(lengths)]).astype(np.int32)
    return offs, img, idx, np.ones(len(lengths), np.uint8)


def ring_list(lengths, ids):
    """the list for tracks_add that makes tracks_of(lengths, ids)"""
    lengths = np.asarray(lengths)
    pairs, offs, qt = [], [0], []
    for i in range(int(lengths.max()) - 1):
        rows = np.nonzero(lengths > i + 1)[0].astype(np.int32)
        pairs.append((ids[i], ids[i + 1]))
        qt.append(np.stack([rows, rows], 1))
        offs.append(offs[-1] + len(rows))
    return (np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(offs, np.int64), np.concatenate(qt).astype(np.int32).reshape(-1, 2))


def routes_job(repeat=250, seed=11, noise_px=8.0):
    """-> (ids, kps list, poses, lengths): 8 * repeat tracks of 2 .. 7 views"""
    # ring_job lives in a GPU test module (which does nothing on import, so the CPU tests may import it too); it would sit better in a
    # fixtures module, but the existing test files are left exactly as they are
    from test_gpu_robust_triangulation import ring_job
    lengths = ROUTE_LENGTHS * repeat
    ids, kps, poses, _ = ring_job(lengths, noise_px=noise_px, seed=seed)
    return ids, kps, poses, lengths


def reordered(kps, lengths, order):
    """the job whose track j is the old track order[j] (keypoint rows permuted in every image)"""
    order = np.asarray(order)
    out = []
    for k in kps:
        k = k.copy()
        k[:len(order)] = k[order]
        out.append(k)
    return out, [int(lengths[i]) for i in order]


ROUTES = ("rejected_then_accepted", "ceiling", "max_iters", "dropped_error_ok", "dropped_angle_ok", "depth_rejected", "two_views",
          "gained_error_ok")


def routes(host, ids, kps, poses, lengths, thresholds=ROUTE_THRESHOLDS, params=ROUTE_PARAMS):
    """The plain triangulation twin and the refinement twin over the job -> (points before, residuals before, points after, residuals
    after, counts, trace, {route: track numbers})"""
    tr_ = tracks_of(lengths, ids)
    pp, pr = tw.run(host, tr_, ids, kps, poses, CAM, thresholds + (2,))
    gp, gr, cnt, tr = rtw.run(host, tr_, ids, kps, poses, CAM, pp, pr, thresholds=thresholds, params=params, trace=True)
    n = np.asarray(lengths)
    gained = ((gp["status"] & ERROR_OK) != 0) & ((pp["status"] & ERROR_OK) == 0)
    found = dict(rejected_then_accepted=np.nonzero((tr["accepted_after_rejected"] > 0) & (tr["verdict"] == 0))[0],
                 ceiling=np.nonzero(tr["stop"] == rtw.STOP_CEILING)[0],
                 max_iters=np.nonzero(tr["stop"] == rtw.STOP_MAX_ITERS)[0],
                 dropped_error_ok=np.nonzero(tr["verdict"] == ERROR_OK)[0],
                 dropped_angle_ok=np.nonzero(tr["verdict"] == ANGLE_OK)[0],
                 depth_rejected=np.nonzero(tr["depth_rejected"] > 0)[0],
                 two_views=np.nonzero((n == 2) & (tr["verdict"] == 0))[0],
                 gained_error_ok=np.nonzero(gained)[0])
    return pp, pr, gp, gr, cnt, tr, found
