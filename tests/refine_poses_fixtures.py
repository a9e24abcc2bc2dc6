"""Inputs shared by the pose refinement's CPU and GPU tests: the ring cameras of tests/test_gpu_robust_triangulation.ring_job with a
free choice of which track is seen in which image (so that every image's fitting set has a chosen size), seeded pose perturbations,
and the search that names one image per route of the Levenberg-Marquardt loop from the twin's trace.  Test infrastructure only."""
import numpy as np

import refine_poses_twin as ptw
import triangulation_twin as tw

CAM = (2500.0, 2500.0, 1536.0, 1152.0)
# max_error: a pose off by 3 mrad and 0.02 units moves a projection by up to 3e-3 x 2500 + 0.02 / 6.5 x 2500 ~ 15 px, two such views
# disagree by up to 30 px: 40 px admits every track of a perturbed job.  min_angle: below the ring's 1.2 degrees between neighbours.
THRESHOLDS = (40.0, 1.0)


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def perturbed(poses, seed, rot=3e-3, trans=0.02, keep=()):
    """every pose (but those of `keep`) turned by `rot` radians about a seeded axis and moved by `trans` in a seeded direction"""
    rng = np.random.default_rng(seed)
    out = {}
    for i in sorted(poses):
        w, d = rng.normal(size=3), rng.normal(size=3)
        if poses[i] is None or i in keep:
            out[i] = poses[i]
            continue
        R, t = poses[i]
        out[i] = (rodrigues(w * rot / np.linalg.norm(w)) @ np.asarray(R, np.float64), np.asarray(t, np.float64) + d * trans / np.linalg.norm(d))
    return out


def membership(sizes, T):
    """seen[j, i]: track j has an observation in image i -- the tracks 0 .. sizes[i] - 1 (a list: exactly those tracks); every track is
    seen in the images 0 and 1, so that track j is the session's kept track j"""
    seen = np.zeros((T, len(sizes)), bool)
    for i, s in enumerate(sizes):
        seen[list(s) if not np.isscalar(s) else np.arange(int(s)), i] = True
    seen[:, :2] = True
    return seen


def match_list(seen, ids):
    """the list for tracks_add that chains every track through the images it is seen in"""
    rows = {}
    for j in range(seen.shape[0]):
        at = np.nonzero(seen[j])[0]
        for a, b in zip(at[:-1], at[1:]):
            rows.setdefault((int(a), int(b)), []).append(j)
    pairs, offs, qt = [], [0], []
    for (a, b) in sorted(rows):
        pairs.append((ids[a], ids[b]))
        r = np.asarray(rows[(a, b)], np.int32)
        qt.append(np.stack([r, r], 1))
        offs.append(offs[-1] + len(r))
    return np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(offs, np.int64), np.concatenate(qt).astype(np.int32).reshape(-1, 2)


def tracks_of(seen, ids):
    """the track result of match_list(seen, ids)"""
    n = seen.sum(1)
    offs = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    img = np.concatenate([ids[np.nonzero(s)[0]] for s in seen]).astype(np.int32)
    idx = np.repeat(np.arange(seen.shape[0]), n).astype(np.int32)
    return offs, img, idx, np.ones(seen.shape[0], np.uint8)


def ring(sizes, T, noise_px=0.3, seed=3, moved=None):
    """-> (ids, kps list, true poses, seen): len(sizes) ring cameras, T points, image i sees the tracks membership() says"""
    # ring_job lives in a GPU test module (which does nothing on import, so the CPU tests may import it too)
    from test_gpu_robust_triangulation import ring_job
    ids, kps, poses, _ = ring_job([len(sizes)] * T, noise_px=noise_px, seed=seed, moved=moved)
    return ids, kps, poses, membership(sizes, T)


def first_records(host, ids, kps, poses, seen, thresholds=THRESHOLDS, cam=CAM):
    """the plain triangulation twin under `poses` -> (tracks, points, residuals)"""
    tracks = tracks_of(seen, ids)
    pp, pr = tw.run(host, tracks, ids, kps, poses, cam, thresholds + (2,))
    return tracks, pp, pr


# ---- the routes the easy data does not reach ----------------------------------------------------------------------------------------
# Found on the CPU through the twin's trace (tests/test_refine_poses_reference.py asserts each on the twin AND on the reference), on the
# ring cameras with 8 px of noise:
#   "ring"    twelve cameras, 120 points; image i sees ROUTE_SIZES[i] tracks (full images, images with few observations, three images
#             that see only a handful of the last tracks); every pose but the first is perturbed, the first is fixed, the last has no
#             valid pose.
#   "single"  twelve cameras that all see 60 points; ONE image is free and starts far from its pose (0.5 rad, 2 units), the others are
#             exact and fixed: the first step at lambda = 1e-3 overshoots.
ROUTE_T = 120
ROUTE_SIZES = [120, 120, 120, 64, 40, 20, 12, 8, 6, list(range(100, 120)), list(range(100, 108)), list(range(100, 106))]
ROUTE_PARAMS = (10, 1e-4, 6)       # max_iters, step_tol, min_observations
ROUTE_CASES = {
    # route: (job, rot, trans, perturbation seed, (max_error, min_angle), what the twin's trace / counters must show)
    "rejected_then_accepted": ("single", 0.5, 2.0, 9, (5000.0, 0.5)),
    "lost_inliers": ("ring", 3e-3, 0.02, 8, (12.0, 1.0)),             # max_error near the noise: an L2 optimum costs a max-norm inlier
    "ceiling_by_depth": ("ring", 0.03, 0.3, 8, (200.0, 1.0)),         # points behind a badly posed camera: every lower cost is refused
    # The re-verdict takes ERROR_OK from points and gives it to others.  A SUCCEEDED track cannot lose it (every one of its fitting
    # observations is an inlier before, and the standing rule keeps the count); a track outside the fitting sets can: min_angle 3
    # degrees leaves the tracks seen in three neighbouring images only (2.4 degrees) with ERROR_OK and without ANGLE_OK.
    "lost_and_gained": ("ring", 3e-3, 0.02, 2, (12.0, 3.0)),
}


def route_case(name):
    """-> (ids, kps, perturbed poses, seen, fixed ids, thresholds, position of the named image in the pose list or None)"""
    job, rot, trans, pseed, thr = ROUTE_CASES[name]
    if job == "single":
        ids, kps, poses, seen = ring([60] * 12, 60, noise_px=8.0, seed=11)
        at = 3 + pseed % 6
        others = tuple(int(i) for i in ids if int(i) != int(ids[at]))
        return ids, kps, perturbed(poses, pseed, rot, trans, keep=others), seen, list(others), thr, at
    ids, kps, poses, seen = ring(ROUTE_SIZES, ROUTE_T, noise_px=8.0, seed=11)
    bad = perturbed(poses, pseed, rot, trans, keep=(int(ids[0]),))
    bad[int(ids[11])] = None
    return ids, kps, bad, seen, [int(ids[0])], thr, None


def routes(trace):
    """{route: positions in the pose list} from the twin's trace"""
    return dict(rejected_then_accepted=np.nonzero((trace["accepted_after_rejected"] > 0) & (trace["verdict"] == 0))[0],
                max_iters=np.nonzero(trace["stop"] == ptw.STOP_MAX_ITERS)[0],
                lost_inliers=np.nonzero(trace["verdict"] == ptw.LOST_INLIERS)[0],
                depth_rejected=np.nonzero(trace["depth_rejected"] > 0)[0],
                ceiling=np.nonzero(trace["stop"] == ptw.STOP_CEILING)[0],
                stands=np.nonzero(trace["verdict"] == 0)[0])
