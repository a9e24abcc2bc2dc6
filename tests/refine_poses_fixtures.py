"""Inputs shared by the pose refinement's CPU and GPU tests: the ring cameras of tests/test_gpu_robust_triangulation.ring_job with a
free choice of which track is seen in which image (so that every image's fitting set has a chosen size), seeded pose perturbations,
the search that names one image per route of the Levenberg-Marquardt loop from the twin's trace, pose lists in other orders than the
ranks', chosen points (a plane, a line, one spot, a camera at the origin, a scaled world) under the same cameras, and the job with more
listed images than the image kernel's grid has waves.  Test infrastructure only."""
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


# ---- pose lists in other orders than the ranks' ------------------------------------------------------------------------------------
def list_orders(ids, fixed_id, seed=5):
    """The orders a pose list over the declared `ids` is tested in, as positions into the ascending list: "sorted"; "permuted" (seeded);
    "dropped" (the first, a middle and the last declared image left out, the rest permuted: list position, rank and the position in
    the ascending list of the same subset -- "dropped_sorted" -- all differ); "fixed_last" (ascending, the fixed image moved to the
    end)."""
    n = len(ids)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    assert n >= 6 and not np.array_equal(perm, np.arange(n))
    sub = np.delete(np.arange(n), [0, n // 2, n - 1])
    sub_perm = sub[rng.permutation(len(sub))]
    assert not np.array_equal(sub_perm, sub)
    at = int(np.nonzero(np.asarray(ids) == fixed_id)[0][0])
    return dict(sorted=np.arange(n), permuted=perm, dropped=sub_perm, dropped_sorted=sub, fixed_last=np.r_[np.delete(np.arange(n), at), at])


def relisted(poses, order):
    """a dict of poses (or an (ids, table) pair in ascending order) -> the (ids, POSE_RT table) pair listing `order`'s positions"""
    pid, tab = ptw.as_pose_list(poses)
    return pid[order].copy(), tab[order].copy()


def by_id(pid, rows):
    """{image id: the bytes of its row}"""
    return {int(i): rows[k].tobytes() for k, i in enumerate(pid)}


def summed_in_list_order(rec):
    """(cost_before, cost_after) as the call adds them: from 0.0, the records in list order"""
    a = b = np.float64(0.0)
    for r in rec:
        a, b = a + r["cost_before"], b + r["cost_after"]
    return float(a), float(b)


# ---- chosen points under the ring cameras ------------------------------------------------------------------------------------------
def ring_cameras(n_img):
    """ids and poses of test_gpu_robust_triangulation.ring_job's cameras: 1.2 degrees apart on a circle of radius 6.5 around the origin"""
    ids = np.arange(n_img, dtype=np.int32) * 3 + 1
    poses = {}
    for i in range(n_img):
        th = 2 * np.pi * i / 300.0
        z = np.asarray([-np.sin(th), 0.0, np.cos(th)])
        x = np.cross([0.0, 1.0, 0.0], z)
        poses[int(ids[i])] = (np.stack([x, np.cross(z, x), z]), np.asarray([0.0, 0.02 * np.sin(5 * th), 6.5]))
    return ids, poses


def chosen_scene(X, sizes, noise_px=0.3, seed=3, frame=None, scale=1.0):
    """The points X [T, 3] under len(sizes) ring cameras, image i seeing the tracks membership() says.  frame: the position of the camera
    whose frame becomes the world's (its pose is R = I, t = 0 exactly); scale: the world (points and translations) scaled.
    -> (ids, kps list, true poses, seen)"""
    from monocularsfm_amd import synth
    rng = np.random.default_rng(seed)
    X = np.asarray(X, np.float64)
    T = len(X)
    ids, poses = ring_cameras(len(sizes))
    if frame is not None:
        R0, t0 = poses[int(ids[frame])]
        X = X @ R0.T + t0
        poses = {i: (R @ R0.T, t - R @ R0.T @ t0) for i, (R, t) in poses.items()}
        poses[int(ids[frame])] = (np.eye(3), np.zeros(3))
    X = X * scale
    poses = {i: (R, t * scale) for i, (R, t) in poses.items()}
    kps = []
    for k, i in enumerate(ids):
        R, t = poses[int(i)]
        kp = synth.keypoints(T, seed=seed + k)
        Y = X @ R.T + t
        kp[:, 0] = (CAM[0] * Y[:, 0] / Y[:, 2] + CAM[2] + rng.normal(0, noise_px, T)).astype(np.float32)
        kp[:, 1] = (CAM[1] * Y[:, 1] / Y[:, 2] + CAM[3] + rng.normal(0, noise_px, T)).astype(np.float32)
        kps.append(kp)
    return ids, kps, poses, membership(sizes, T)


def general_points(T, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (T, 3))


def planar_points(T, seed):
    """on the plane z = 0.2 x - 0.1 y + 0.1 (tilted against every camera's image plane)"""
    xy = np.random.default_rng(seed).uniform(-1.0, 1.0, (T, 2))
    return np.c_[xy, 0.2 * xy[:, 0] - 0.1 * xy[:, 1] + 0.1]


def collinear_points(T, seed):
    """on the line through the origin along z, the first camera's optical axis (of the lines tried -- x, y, z, x + y, a general one --
    the only one that stays degenerate after the triangulation under perturbed poses and 0.3 px of noise has scattered the points)"""
    return np.c_[np.zeros((T, 2)), np.random.default_rng(seed).uniform(-1.0, 1.0, T)]


def coincident_points(T, seed, jitter=1e-9):
    return np.asarray([0.1, -0.2, 0.05]) + jitter * np.random.default_rng(seed).normal(size=(T, 3))


# ---- the twin against the reference off the captures (tests/test_refine_poses_reference.py, 2b of its docstring) --------------------
# Eight ring cameras, 40 points, 0.3 px of noise, the first two images fixed, every other pose perturbed by 3 mrad and 0.02 units (the
# scaled world: 20 units), THRESHOLDS, step_tol 1e-4.
REF_T = 40
REF_CASES = {
    # name: (points, sizes, frame, scale, min_observations, scene seed, perturbation seed)
    "minimal_sets": (general_points, [40, 40, 40, 40, 3, 4, 5, 6], None, 1.0, 3, 3, 31),
    "planar_scene": (planar_points, [40] * 8, None, 1.0, 15, 3, 31),
    "origin_camera": (general_points, [40] * 8, 4, 1.0, 15, 3, 31),
    "scaled_world": (general_points, [40] * 8, None, 1e3, 15, 3, 31),
}


def ref_case(name):
    """-> (ids, kps, perturbed poses, seen, fixed ids, THRESHOLDS, (max_iters, step_tol, min_observations))"""
    points, sizes, frame, scale, min_obs, seed, pseed = REF_CASES[name]
    ids, kps, poses, seen = chosen_scene(points(REF_T, seed + 50), sizes, seed=seed, frame=frame, scale=scale)
    fixed = [int(ids[0]), int(ids[1])]
    return ids, kps, perturbed(poses, pseed, trans=0.02 * scale, keep=tuple(fixed)), seen, fixed, THRESHOLDS, (10, 1e-4, min_obs)


# ---- ill-conditioned fitting sets: routes decided in the last bits of a cost -------------------------------------------------------
# Collinear points leave the rotation about their line free; nearly coincident points (1e-9 apart, triangulated from 0.3 px of noise)
# leave all but the direction to them nearly free.  LM then walks a flat valley: accepted and rejected steps alternate, lambda runs to
# its floor, and each accept / reject is decided by the last bits of two costs.  Fitting sets of 40, 64 and 130 entries: one, exactly
# one and three rounds of the stride-64 partials.
ILL_T = 130
ILL_SIZES = [130, 130, 130, 64, 40, 130, 64, 40]
ILL_CASES = {"collinear": (collinear_points, 3, 31), "coincident": (coincident_points, 3, 31)}   # points, scene seed, perturbation seed
ILL_PARAMS = ((30, 1e-6, 3), (100, 1e-6, 3))


def ill_case(name):
    """-> (ids, kps, perturbed poses, seen, fixed ids, THRESHOLDS)"""
    points, seed, pseed = ILL_CASES[name]
    ids, kps, poses, seen = chosen_scene(points(ILL_T, seed + 50), ILL_SIZES, seed=seed)
    fixed = [int(ids[0]), int(ids[1])]
    return ids, kps, perturbed(poses, pseed, keep=tuple(fixed)), seen, fixed, THRESHOLDS


def assert_ill_routes(rec, tr, max_iters):
    """what tests/refine_poses_fixtures.ILL_CASES were chosen for, on the twin's trace"""
    at_limit = (tr["stop"] == ptw.STOP_MAX_ITERS) & (tr["steps"] == max_iters)
    assert at_limit.any() and (tr["accepted_after_rejected"] >= 10).any(), (tr["steps"], tr["stop"], tr["accepted_after_rejected"])
    if max_iters == 30:     # found: every eligible image, so every size of fitting set, runs to the limit
        for n in (40, 64, 130):
            assert (at_limit & (tr["accepted_after_rejected"] >= 10) & (rec["n_observations"] == n)).any(), n


# ---- more listed images than rp_image_kernel's grid has waves ------------------------------------------------------------------------
GROUP_TRACKS = 6
# max_iters 2: every eligible image takes both steps, accepts them and stands (the twin, which runs each six-entry fitting set through
# all 64 partials, is the largest part of the device test's time; at max_iters 10 it takes 4 steps per image and twice as long);
# min_observations 4: a third image that sees two tracks lies below it, the others see six
LISTED_PARAMS = (2, 1e-6, 4)


def listed_images_job(L, rows=GROUP_TRACKS, seed=7):
    """L images with the ids 0 .. L - 1 and `rows` keypoints each, in groups of three (the last group: what is left); group g shares
    six tracks of its own at the rows 0 .. 5, its cameras stand 2.4 degrees apart as test_gpu_robust_triangulation.second_pass_job's.
    In every 97th group the third image sees the tracks 0 and 1 only.  The match list and the track result are built directly, in
    whole arrays: at this size loops over images cost more than the device call under test.
    -> (ids, kps, true R [L, 3, 3], true t [L, 3], the list for tracks_add, the track result)"""
    rng = np.random.default_rng(seed)
    G = (L + 2) // 3
    Rc, tc = np.empty((3, 3, 3)), np.empty((3, 3))
    for k in range(3):
        th = 2 * np.pi * (2 * k) / 300.0
        z = np.asarray([-np.sin(th), 0.0, np.cos(th)])
        x = np.cross([0.0, 1.0, 0.0], z)
        Rc[k], tc[k] = np.stack([x, np.cross(z, x), z]), (0.0, 0.02 * k, 6.5)
    X = rng.uniform(-1.0, 1.0, (G, GROUP_TRACKS, 3))
    kp = np.empty((G, 3, rows, 4), np.float32)
    kp[..., :2] = rng.uniform(0.0, 2304.0, (G, 3, rows, 2))
    kp[..., 2:] = (2.0, 0.0)
    for k in range(3):
        Y = X @ Rc[k].T + tc[k]
        kp[:, k, :GROUP_TRACKS, 0] = CAM[0] * Y[..., 0] / Y[..., 2] + CAM[2] + rng.normal(0, 0.3, (G, GROUP_TRACKS))
        kp[:, k, :GROUP_TRACKS, 1] = CAM[1] * Y[..., 1] / Y[..., 2] + CAM[3] + rng.normal(0, 0.3, (G, GROUP_TRACKS))
    kps = list(kp.reshape(3 * G, rows, 4)[:L])
    g = np.arange(G)
    m = np.minimum(3, L - 3 * g)                                       # images of the group
    third = np.where(g % 97 == 5, 2, GROUP_TRACKS)                     # tracks its third image sees
    # the match list: (3g, 3g + 1) with six rows, (3g + 1, 3g + 2) with `third` rows, where the images exist
    count = np.stack([np.where(m >= 2, GROUP_TRACKS, 0), np.where(m >= 3, third, 0)], 1).reshape(-1)
    pair = np.stack([np.stack([3 * g, 3 * g + 1], 1), np.stack([3 * g + 1, 3 * g + 2], 1)], 1).reshape(-1, 2)
    pair, count = pair[count > 0], count[count > 0]
    offs = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    row = (np.arange(offs[-1]) - np.repeat(offs[:-1], count)).astype(np.int32)
    lst = (pair.astype(np.int32), offs, np.stack([row, row], 1))
    # the track result: group-major, by row; two or three observations by ascending image
    length = np.where((m[:, None] >= 3) & (np.arange(GROUP_TRACKS)[None] < third[:, None]), 3, 2)[m >= 2].reshape(-1)
    first = np.repeat(3 * g[m >= 2], GROUP_TRACKS)
    t_offs = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    t_img = (np.repeat(first, length) + np.arange(t_offs[-1]) - np.repeat(t_offs[:-1], length)).astype(np.int32)
    t_idx = np.repeat(np.tile(np.arange(GROUP_TRACKS), int((m >= 2).sum())), length).astype(np.int32)
    which = np.arange(L) % 3
    return np.arange(L, dtype=np.int32), kps, Rc[which], tc[which], lst, (t_offs, t_img, t_idx, np.ones(len(length), np.uint8))


def listed_images_case(L, first_pass, rot=3e-3, trans=0.02):
    """listed_images_job(L) with every pose perturbed (as perturbed() does, in whole arrays) and a list of all L images that is not in
    rank order: a seeded permutation in which the list positions first_pass .. first_pass + 4 (the second stride pass of a grid of
    first_pass waves) hold an eligible image, a fixed image, an unposed image, an image below min_observations and a second eligible
    image, and position 0 (the same wave as position first_pass) an eligible image.
    -> (ids, kps, (list ids, POSE_RT table), match list, tracks, fixed ids, {what: list position})"""
    from monocularsfm_amd._lib import POSE_RT
    assert L >= first_pass + 5
    ids, kps, R, t, lst, tracks = listed_images_job(L)
    G = L // 3
    short = [g for g in range(G) if g % 97 == 5]
    special = dict(eligible=3 * (G // 7), fixed=3 * (2 * G // 7) + 1, unposed=3 * (3 * G // 7) + 2, below=3 * short[len(short) // 2] + 2,
                   second_eligible=3 * (5 * G // 7) + 1, first=3 * (6 * G // 7) + 2)
    assert len(set(i // 3 for i in special.values())) == 6 and not any((i // 3) % 97 == 5 for k, i in special.items() if k != "below")
    rng = np.random.default_rng(13)
    w, d = rng.normal(size=(2, L, 3))
    w, d = w / np.linalg.norm(w, axis=1)[:, None], d / np.linalg.norm(d, axis=1)[:, None]
    K = np.zeros((L, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    tab = np.zeros(L, POSE_RT)
    tab["valid"] = 1
    tab["R"] = ((np.eye(3) + np.sin(rot) * K + (1 - np.cos(rot)) * (K @ K)) @ R).reshape(L, 9)
    tab["t"] = t + d * trans
    tab[special["unposed"]] = np.zeros(1, POSE_RT)[0]
    at = dict(first=0, eligible=first_pass, fixed=first_pass + 1, unposed=first_pass + 2, below=first_pass + 3, second_eligible=first_pass + 4)
    perm = np.random.default_rng(17).permutation(L)
    order = np.empty(L, np.int64)
    free = np.ones(L, bool)
    for k, pos in at.items():
        order[pos], free[pos] = special[k], False
    order[free] = perm[~np.isin(perm, list(special.values()))]
    assert np.array_equal(np.sort(order), np.arange(L)) and not np.array_equal(order, np.arange(L))
    return ids, kps, (ids[order].copy(), tab[order].copy()), lst, tracks, [special["fixed"]], at


def assert_placed(at, rec, tr, params=LISTED_PARAMS):
    """the twin's records and trace show what listed_images_case placed"""
    for k in ("first", "eligible", "second_eligible"):
        assert tr[at[k]]["verdict"] == 0 and tr[at[k]]["accepted"] > 0 and rec[at[k]]["status"] == 3, (k, rec[at[k]], tr[at[k]])
    assert rec[at["fixed"]]["status"] == 4 and rec[at["unposed"]]["status"] == 0 and rec[at["unposed"]]["n_observations"] == 0
    assert rec[at["below"]]["status"] == 0 and 0 < rec[at["below"]]["n_observations"] < params[2]
