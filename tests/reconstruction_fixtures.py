"""A capture WITH its ground truth for the end-to-end reconstruction tests (tests/test_reconstruction_reference.py on the host twins,
tests/test_gpu_reconstruction.py on the device): tests/tracks_fixtures.scene_job's 24 x 600 capture plus what scene_job does not
return -- the true world-to-camera poses, the 1500 scene points and the prototype (scene point) of every row -- and the similarity
alignment that compares a reconstruction, which is free up to a gauge, with them.  Test infrastructure only."""
import functools

import numpy as np

import emat_ref
from monocularsfm_amd import synth

CAM = (2500.0, 2500.0, 1536.0, 1152.0)
CAM_D = CAM + (-0.1, 0.02, 1e-3, -5e-4)        # tests/test_gpu_refine_points.py's distorted camera
N_IMAGES, N_DESC, N_PROTO = 24, 600, 1500


@functools.lru_cache(maxsize=None)
def _descriptors(seed):
    """the descriptors depend on the seed alone: every variant of one seed shares the arrays"""
    return synth.rootsift_images(N_IMAGES, N_DESC, seed=seed, n_proto=N_PROTO, return_proto=True)


def true_points(seed):
    """the first three draws of default_rng(seed) that synth.scene_keypoints makes"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-1.6, 1.6, N_PROTO), rng.uniform(-1.1, 1.1, N_PROTO), rng.uniform(-1.0, 1.0, N_PROTO)], 1)


def capture(seed=77, noise_px=0.7, cam=CAM, permute=None, swap_pairs=False):
    """scene_job(seed=seed)'s capture (the same descriptors; with noise_px 0.7 and CAM the same keypoints, bit for bit).  noise_px 0.0
    leaves float32 rounding of the keypoints as the only error.  A camera with distortion: the keypoints are re-made through the Brown
    model.  permute: a seed -- the SAME images under permuted ids (position k gets ids[perm[k]]), so that the pair list, which is
    ids[synth.all_pairs()], no longer has the higher id first in every pair.  swap_pairs: every second pair is given as (b, a).
    -> dict: ids, imgs (by position), kps {id: n x 4}, pairs, cam, poses {id: (R, t)} world-to-camera, X [1500 x 3], protos {id: int
    per row, -1: the row observes nothing}"""
    imgs, protos = _descriptors(seed)
    cams = synth.scene_cameras(N_IMAGES, seed=seed)
    kps = synth.scene_keypoints(protos, cams, N_PROTO, seed=seed, noise_px=noise_px)
    X = true_points(seed)
    cam = tuple(float(c) for c in cam)
    if any(cam[4:]) or cam[:4] != CAM:
        cam8 = cam + (0.0,) * (8 - len(cam))
        nrng = np.random.default_rng(seed + 9)
        for i, k in enumerate(kps):
            sel = np.nonzero(np.asarray(protos[i]) >= 0)[0]
            Y = X[np.asarray(protos[i])[sel]] @ cams[i][0].T + cams[i][1]
            xd, yd = emat_ref.distort(cam8, Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2])
            k[sel, 0] = (cam8[0] * xd + cam8[2] + nrng.normal(0, noise_px, len(sel))).astype(np.float32)
            k[sel, 1] = (cam8[1] * yd + cam8[3] + nrng.normal(0, noise_px, len(sel))).astype(np.float32)
    ids = np.asarray([3 * i + 1 for i in range(N_IMAGES)], np.int32)
    if permute is not None:
        ids = ids[np.random.default_rng(permute).permutation(N_IMAGES)]
    pairs = np.ascontiguousarray(ids[synth.all_pairs(N_IMAGES)])
    if swap_pairs:
        pairs[1::2] = pairs[1::2, ::-1].copy()
    return dict(ids=ids, imgs=list(imgs), kps={int(i): k for i, k in zip(ids, kps)}, pairs=pairs, cam=cam, seed=seed,
                poses={int(i): (c[0].copy(), c[1].copy()) for i, c in zip(ids, cams)}, X=X,
                protos={int(i): np.asarray(p, np.int64) for i, p in zip(ids, protos)})


def reprojection(cap, image_id):
    """the pixel positions of the scene points that the rows of one image observe, through the true pose and the capture's camera
    -> (rows, n x 2 float64)"""
    cam8 = cap["cam"] + (0.0,) * (8 - len(cap["cam"]))
    p = cap["protos"][int(image_id)]
    rows = np.nonzero(p >= 0)[0]
    R, t = cap["poses"][int(image_id)]
    Y = cap["X"][p[rows]] @ R.T + t
    xd, yd = emat_ref.distort(cam8, Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2])
    return rows, np.stack([cam8[0] * xd + cam8[2], cam8[1] * yd + cam8[3]], 1)


def relative_pose(cap, a, b):
    """the true (R, t) with x_b ~ R x_a + t, t of unit length: the record's convention for the pair GIVEN as (a, b)"""
    (Ra, ta), (Rb, tb) = cap["poses"][int(a)], cap["poses"][int(b)]
    R = Rb @ Ra.T
    t = tb - R @ ta
    return R, t / np.linalg.norm(t)


def angle_deg(Ra, Rb):
    """the angle of the rotation Ra Rb^T in degrees"""
    c = (np.trace(np.asarray(Ra).reshape(3, 3) @ np.asarray(Rb).reshape(3, 3).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def direction_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def umeyama(src, dst):
    """the similarity (s, Q, d) that minimises sum |dst - (s Q src + d)|^2 (Umeyama 1991), Q a proper rotation"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    ms, md = src.mean(0), dst.mean(0)
    a, b = src - ms, dst - md
    U, S, Vt = np.linalg.svd(b.T @ a / len(src))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    Q = U @ D @ Vt
    s = float(np.trace(np.diag(S) @ D) / (a * a).sum() * len(src))
    return s, Q, md - s * Q @ ms


def align(cap, poses, tracks, points, inliers):
    """A reconstruction against the capture's ground truth after the similarity alignment of its camera centres onto the true ones.
    poses: {id: (R, t)} (Context.poses()); tracks, points, inliers: Context.tracks(), points3d()[0], point_inliers().
    -> dict: posed (sorted ids), centre [per posed image, scene units], rotation [per posed image, degrees], point [per pure point,
    scene units], n_succeeded, n_pure, n_mixed, share_succeeded (of the kept tracks), share_mixed (of the succeeded points).  A succeeded
    point is pure when its fitting observations (inlier byte 1) all belong to ONE prototype; its error is its distance from that
    prototype's scene point.  The others are counted as mixed."""
    posed = sorted(int(i) for i in poses)
    C_est = np.stack([-poses[i][0].T @ poses[i][1] for i in posed])
    C_true = np.stack([-cap["poses"][i][0].T @ cap["poses"][i][1] for i in posed])
    s, Q, d = umeyama(C_est, C_true)
    centre = np.linalg.norm(C_est @ (s * Q).T + d - C_true, axis=1)
    rotation = np.asarray([angle_deg(poses[i][0] @ Q.T, cap["poses"][i][0]) for i in posed])
    offsets, img, idx = tracks[0], tracks[1], tracks[2]
    proto = np.asarray([cap["protos"][int(i)][int(k)] for i, k in zip(img, idx)], np.int64)
    ok = (np.asarray(points)["status"] & 14) == 14
    err, mixed = [], 0
    for t in np.nonzero(ok)[0]:
        sl = slice(int(offsets[t]), int(offsets[t + 1]))
        p = proto[sl][np.asarray(inliers[sl]) != 0]
        if len(p) == 0 or p.min() < 0 or p.min() != p.max():
            mixed += 1
            continue
        err.append(np.linalg.norm(s * Q @ points[t]["X"] + d - cap["X"][p[0]]))
    n_ok = int(ok.sum())
    return dict(posed=posed, centre=centre, rotation=rotation, point=np.asarray(err), n_succeeded=n_ok, n_pure=len(err), n_mixed=mixed,
                share_succeeded=n_ok / max(len(ok), 1), share_mixed=mixed / max(n_ok, 1), similarity=(s, Q, d))


# ---- the chain: the same calls on a _lib.Context and on tests/twin_context.TwinContext ----------------------------------------------------
TWO_VIEW = (30, 2.0, 4.0)              # min_num_inliers, tri_max_error, tri_min_angle of the two-view records
MIN_POINTS = 65                        # initialize(): a pair of this capture shares about 60 .. 75 scene points
REGISTER = dict(min_inliers=8)         # register_images(): an unposed image sees 15 .. 20 points of a young map
LOOP = dict(max_images=1, window=5, rounds=2, complete_params={}, register_params=REGISTER)     # the reference's loop
BATCH = dict(rounds=2, complete_params={}, register_params=REGISTER)                            # grow's default batching
ALL_CAMERA = ("fx_fy", "cx_cy", "k1_k2")

VARIANTS = {
    "s77": dict(seed=77), "s5": dict(seed=5), "s77-clean": dict(seed=77, noise_px=0.0), "s5-clean": dict(seed=5, noise_px=0.0),
    "s77-distorted": dict(seed=77, cam=CAM_D), "s5-distorted": dict(seed=5, cam=CAM_D),
    "s77-permuted": dict(seed=77, permute=3), "s77-swapped": dict(seed=77, swap_pairs=True),
}


@functools.lru_cache(maxsize=None)
def variant(name):
    return capture(**VARIANTS[name])


def open_session(ctx, cap, cam=None, stream=False):
    """upload, verified matching under VERIFY_ESSENTIAL with two-view records over all pairs inside a track session, tracks_finish.
    stream: the verified streaming form (every chunk folds as it is handed out).  -> (lists, records [one per pair], track stats)"""
    from monocularsfm_amd import _lib
    cam = cap["cam"] if cam is None else cam
    for k, i in enumerate(cap["ids"]):
        ctx.upload_image(int(i), cap["imgs"][k])
        ctx.upload_keypoints(int(i), cap["kps"][int(i)])
    ctx.set_verification_model(_lib.VERIFY_ESSENTIAL, cam)
    ctx.set_two_view_geometry(True, *TWO_VIEW)
    ctx.tracks_begin(cap["ids"])
    if stream:
        chunks = list(ctx.match_pairs_stream(cap["pairs"], verified=True))
        assert sum(c["n_pairs"] for c in chunks) == len(cap["pairs"])
        offsets = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(c["offsets"]) for c in chunks]))]).astype(np.int64)
        lists = (offsets, np.concatenate([c["qt"] for c in chunks]), np.concatenate([c["dist"] for c in chunks]))
        records = np.concatenate([c["two_view_geometry"] for c in chunks])
    else:
        lists = ctx.match_pairs_verified(cap["pairs"])
        records = ctx.two_view_geometry(len(cap["pairs"]))
    return lists, records, ctx.tracks_finish()


def two_view_dict(cap, records):
    """{(id1, id2) as the pair was GIVEN: its record}: what initialize takes"""
    return {(int(a), int(b)): records[p] for p, (a, b) in enumerate(cap["pairs"])}


def increments(ctx, cam, camera_params=None):
    """the reference's loop, then grow's default batching, one increment a step (reconstruct(max_increments=1) until nothing registers:
    the same calls in the same order as the two whole runs) -> yields reconstruct's dict per increment"""
    extra = {} if camera_params is None else dict(camera_params=camera_params)
    for kw in (LOOP, BATCH):
        while True:
            out = ctx.reconstruct(cam, max_increments=1, **kw, **extra)
            if not out:
                break
            yield out[0]


def snapshot(ctx):
    """the session's map as bytes: points3d(), point_inliers() (None while the session has no inlier bytes: behind a plain
    triangulation), pose_list(), camera()"""
    from monocularsfm_amd import _lib
    pts, res = ctx.points3d()
    ids, tab = ctx.pose_list()
    cam = ctx.camera()
    try:
        inliers = ctx.point_inliers().tobytes()
    except _lib.MsfmError as e:
        assert e.code == _lib.E_STATE
        inliers = None
    return dict(points=pts.tobytes(), residuals=res.tobytes(), inliers=inliers, pose_ids=ids.tobytes(), poses=tab.tobytes(),
                camera=np.asarray([cam[k] for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")]).tobytes())


def measure(cap, ctx):
    return figures(align(cap, ctx.poses(), ctx.tracks(), ctx.points3d()[0], ctx.point_inliers()))


FIGURES = ("centre_max", "rotation_max", "point_median", "point_p95", "share_succeeded", "share_mixed")


def within(f, name, measured=None):
    """The bound of both end-to-end tests: the figures f of a run against 2 x the figures MEASURED[name] on the twin chain (never
    against the device's own output).  The four errors and the mixed share may at most double; of the kept tracks the share WITHOUT a
    succeeded point may at most double.  The two shares move in steps of one track (1 / 1400), which is allowed on top of a measured 0.
    -> list of the figures that miss (empty: all hold)"""
    m = (measured or MEASURED)[name]
    step = 1.0 / 1400
    miss = [k for k in ("centre_max", "rotation_max", "point_median", "point_p95") if not f[k] <= 2.0 * m[k]]
    if not f["share_mixed"] <= 2.0 * m["share_mixed"] + step:
        miss.append("share_mixed")
    if not 1.0 - f["share_succeeded"] <= 2.0 * (1.0 - m["share_succeeded"]) + step:
        miss.append("share_succeeded")
    return [(k, f[k], m[k]) for k in miss]


def figures(a):
    """align()'s result as the six figures the tests bound"""
    return dict(centre_max=float(a["centre"].max()), rotation_max=float(a["rotation"].max()), point_median=float(np.median(a["point"])),
                point_p95=float(np.percentile(a["point"], 95)), share_succeeded=float(a["share_succeeded"]),
                share_mixed=float(a["share_mixed"]))


# ---- what the twin chain gives (tests/test_reconstruction_reference.py measured it; DESIGN.md has the table) --------------------------------
# per variant: median and maximum rotation error, median and maximum translation direction error of the 276 two-view records, degrees
RECORDS = {
    "s77": (0.7941, 5.016, 0.8241, 10.52),
    "s5": (0.7149, 4.594, 0.8303, 28.98),
    "s77-distorted": (0.7501, 3.608, 0.7407, 12.77),
    "s5-distorted": (0.7689, 4.381, 0.8176, 25.73),
    "s77-permuted": (0.7941, 5.016, 0.8241, 10.52),
    "s77-swapped": (0.7726, 5.016, 0.7937, 10.99),
    "s77-clean": (9.364e-05, 0.0808, 0.0001041, 1.283),
    "s5-clean": (0.0001202, 1.488, 0.0001239, 9.114),
    "s77-clean-reversed": (0.0001074, 2.104, 9.242e-05, 6.106),          # every pair of s77-clean given as (b, a)
}
# per variant, after the whole chain and the similarity alignment: centre and point errors in scene units (the scene is a box of
# 3.2 x 2.2 x 2, the cameras stand 5.5 .. 7 away), rotation in degrees; "-offcamera": started from bad(CAM), refine_camera on fx, fy
MEASURED = {
    "s77": dict(centre_max=0.006214, rotation_max=0.1487, point_median=0.02529, point_p95=0.04361, share_succeeded=0.9993, share_mixed=0),
    "s5": dict(centre_max=0.06301, rotation_max=1.136, point_median=0.1965, point_p95=0.2686, share_succeeded=0.9896, share_mixed=0),
    "s77-distorted": dict(centre_max=0.2113, rotation_max=2.603, point_median=0.3557, point_p95=0.4856, share_succeeded=0.8528, share_mixed=0),
    "s5-distorted": dict(centre_max=0.08846, rotation_max=2.162, point_median=0.3816, point_p95=0.5028, share_succeeded=0.8921, share_mixed=0),
    "s77-permuted": dict(centre_max=0.02078, rotation_max=0.5208, point_median=0.09689, point_p95=0.1298, share_succeeded=0.9986, share_mixed=0),
    "s77-swapped": dict(centre_max=0.00475, rotation_max=0.07802, point_median=0.0123, point_p95=0.02957, share_succeeded=0.9993, share_mixed=0),
    "s77-clean": dict(centre_max=2.921e-05, rotation_max=0.0006499, point_median=0.0001243, point_p95=0.0001607, share_succeeded=0.9993, share_mixed=0),
    "s5-clean": dict(centre_max=6.309e-07, rotation_max=1.1e-05, point_median=1.934e-06, point_p95=2.674e-06, share_succeeded=1, share_mixed=0),
    "s77-offcamera": dict(centre_max=0.0505, rotation_max=0.9792, point_median=0.1539, point_p95=0.2198, share_succeeded=0.9986, share_mixed=0),
    "s5-offcamera": dict(centre_max=0.04103, rotation_max=1.046, point_median=0.08789, point_p95=0.1243, share_succeeded=0.9937, share_mixed=0),
}
