"""The track triangulation's host twin (monocularsfm_amd/csrc/msfm_triangulate.h through libmsfm_host.so, tests/triangulation_twin.py)
against the independent numpy reference tests/triangulation_ref.py (stacked rows + numpy.linalg.svd, Newton undistortion, np.arccos):
on tests/tracks_fixtures.scene_job with its cameras as poses and the ground-truth prototype tracks, on the same capture with 0.3 px of
noise (truth recovery, a planted outlier), and on the edge cases of the definition.  CPU only.

Tolerances.  Worst differences twin - reference measured on the CPU over the captures below (seeds 77 and 5, with and without
distortion, 0.7 and 0.3 px of noise; python tests/test_triangulation_reference.py prints them):
    X              4.9e-13 (absolute; a scene of extent ~3 at distance ~6)
    residuals      5.3e-12 px  (mean_residual 1.2e-12)
    tri_angle      5.0e-13 degrees
The bounds are 16 x those, the margin of tests/test_pose_reference.py:  TOL_X = 7.8e-12,  TOL_RES = 8.5e-11 px,  TOL_ANGLE = 8.0e-12
degrees.  (The twin solves the 4 x 4 normal equations by Jacobi where the reference takes the SVD of the stacked rows; the condition
number enters squared, and these well-conditioned captures still leave four digits of fp64 to spare.)
Truth recovery (0.3 px of noise, seed 5): the reference's points lie within 0.0434 of the true points (worst over the 1439 pure
tracks); the twin's must lie within 16 x that, 0.70 -- and within TOL_X of the reference's, which is the sharper statement.  Seed 77
is not used there: its capture holds one two-view track whose cameras subtend 1.37 degrees at the point, below min_angle by geometry,
whatever the noise."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import emat_ref  # noqa: E402
import tracks_fixtures as fx  # noqa: E402
import triangulation_ref as ref  # noqa: E402
import triangulation_twin as tw  # noqa: E402

TOL_X = 7.8e-12
TOL_RES = 8.5e-11
TOL_ANGLE = 8.0e-12
TRUTH_REF = 0.0434
TRUTH_BOUND = 16 * TRUTH_REF
CAM = (2500.0, 2500.0, 1536.0, 1152.0)
CAM_D = CAM + (-0.1, 0.02, 1e-3, -5e-4)
SEEDS = (77, 5)


@pytest.fixture(scope="module")
def host():
    return tw.load_host()


def capture(seed=77, noise_px=0.7, cam=CAM, n_images=24, n_desc=600, n_proto=1500):
    """fx.scene_job's capture with what it does not return: the prototype of every row, the cameras, the true points.  With a distorted
    camera, or one whose focal lengths or centre are not CAM's, the keypoints are re-made through the Brown model.  -> dict"""
    from monocularsfm_amd import synth
    _, protos = synth.rootsift_images(n_images, n_desc, seed=seed, n_proto=n_proto, return_proto=True)
    cams = synth.scene_cameras(n_images, seed=seed)
    kps = synth.scene_keypoints(protos, cams, n_proto, seed=seed, noise_px=noise_px)
    ids = np.asarray([3 * i + 1 for i in range(n_images)], np.int32)
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.6, 1.6, n_proto), rng.uniform(-1.1, 1.1, n_proto), rng.uniform(-1.0, 1.0, n_proto)], 1)
    if any(cam[4:]) or tuple(cam[:4]) != CAM:
        nrng = np.random.default_rng(seed + 9)
        for i, k in enumerate(kps):
            sel = np.nonzero(np.asarray(protos[i]) >= 0)[0]
            R, t = cams[i][0], cams[i][1]
            Y = X[np.asarray(protos[i])[sel]] @ R.T + t
            xd, yd = emat_ref.distort(tuple(cam) + (0.0,) * (8 - len(cam)), Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2])
            k[sel, 0] = (cam[0] * xd + cam[2] + nrng.normal(0, noise_px, len(sel))).astype(np.float32)
            k[sel, 1] = (cam[1] * yd + cam[3] + nrng.normal(0, noise_px, len(sel))).astype(np.float32)
    tracks, track_proto = ref.proto_tracks(ids, protos)
    return dict(ids=ids, kps={int(i): k for i, k in zip(ids, kps)}, poses={int(i): (c[0], c[1]) for i, c in zip(ids, cams)}, cam=cam,
                tracks=tracks, X=X[np.asarray(track_proto)])


def worst(want, got):
    """reference list, twin (points, residuals), offsets -> dict of the worst differences; asserts equal status and n_views"""
    pts, res = got
    w = dict(X=0.0, res=0.0, mean=0.0, angle=0.0)
    at = 0
    for t, r in enumerate(want):
        n = len(r["residuals"])
        assert int(pts[t]["status"]) == r["status"], (t, int(pts[t]["status"]), r["status"])
        assert int(pts[t]["n_views"]) == r["n_views"], t
        assert np.array_equal(res[at:at + n] < 0, r["residuals"] < 0), t
        if r["status"] & ref.POINT:
            w["X"] = max(w["X"], float(np.abs(pts[t]["X"] - r["X"]).max()))
            used = r["residuals"] >= 0
            w["res"] = max(w["res"], float(np.abs(res[at:at + n][used] - r["residuals"][used]).max()))
            w["mean"] = max(w["mean"], abs(float(pts[t]["mean_residual"]) - r["mean_residual"]))
            w["angle"] = max(w["angle"], abs(float(pts[t]["tri_angle"]) - r["tri_angle"]))
        at += n
    return w


def margins_hold(want):
    """on the reference alone: no residual within the tolerance of max_error, no scanned angle within it of min_angle (the margins
    are triangulation_ref.track's, against the parameters it ran with).  A track without a point has no residual and no scanned angle:
    its margins are infinite and it is judged by its status bits alone."""
    assert min(r["error_margin"] for r in want) > 16 * TOL_RES
    assert min(r["angle_margin"] for r in want) > 16 * TOL_ANGLE


def within(w):
    assert w["X"] <= TOL_X and w["res"] <= TOL_RES and w["mean"] <= TOL_RES and w["angle"] <= TOL_ANGLE, w


@pytest.mark.parametrize("seed", SEEDS)
def test_twin_equals_reference_on_the_scene_job(host, seed):
    """Every track of the capture: the status bits agree on EVERY track (none is left out: the margins are asserted on the reference
    first), X, residuals and angle within the tolerances of the module docstring."""
    c = capture(seed)
    if seed == 77:   # the capture IS scene_job's
        ids, _, kps, _ = fx.scene_job()
        assert np.array_equal(ids, c["ids"]) and all(np.array_equal(k, c["kps"][int(i)]) for i, k in zip(ids, kps))
    want = ref.run(c["tracks"], c["kps"], c["poses"], c["cam"])
    margins_hold(want)
    st = np.asarray([r["status"] for r in want])
    assert len(want) > 1000 and ((st & ref.SUCCESS) == ref.SUCCESS).sum() > 500 and ((st & ref.ERROR_OK) == 0).sum() > 20   # both verdicts
    got = tw.run(host, c["tracks"], c["ids"], c["kps"], c["poses"], c["cam"])
    w = worst(want, got)
    print("seed %d: worst twin - reference %s" % (seed, w))
    within(w)


@pytest.mark.parametrize("params", [(1.0, 4.0, 2), (2.0, 1.5, 3), (0.5, 12.0, 4)])
def test_other_parameters(host, params):
    c = capture(77)
    want = ref.run(c["tracks"], c["kps"], c["poses"], c["cam"], *params)
    margins_hold(want)
    st = np.asarray([r["status"] for r in want])
    assert (st == 0).sum() > 0 if params[2] > 2 else True
    assert ((st & ref.ANGLE_OK) == 0).sum() > 0 if params[1] > 10 else True
    within(worst(want, tw.run(host, c["tracks"], c["ids"], c["kps"], c["poses"], c["cam"], params)))


def test_distortion_against_the_reference_undistortion(host):
    c = capture(77, cam=CAM_D)
    want = ref.run(c["tracks"], c["kps"], c["poses"], c["cam"])
    margins_hold(want)
    st = np.asarray([r["status"] for r in want])
    assert ((st & ref.SUCCESS) == ref.SUCCESS).sum() > 500
    plain = ref.run(c["tracks"], c["kps"], c["poses"], CAM)   # (the distortion matters: ignoring it fails hundreds of tracks more)
    assert sum((r["status"] & ref.ERROR_OK) != 0 for r in plain) < ((st & ref.ERROR_OK) != 0).sum() - 200
    w = worst(want, tw.run(host, c["tracks"], c["ids"], c["kps"], c["poses"], c["cam"]))
    print("distorted camera: worst twin - reference %s" % w)
    within(w)


def test_truth_recovery_and_a_planted_outlier(host):
    c = capture(5, noise_px=0.3)
    want = ref.run(c["tracks"], c["kps"], c["poses"], c["cam"])
    assert all((r["status"] & ref.SUCCESS) == ref.SUCCESS for r in want)          # every pure track succeeds in the reference
    d_ref = max(float(np.linalg.norm(r["X"] - x)) for r, x in zip(want, c["X"]))
    print("truth recovery: reference within %.4g of the true points" % d_ref)
    assert d_ref <= TRUTH_REF
    pts, res = tw.run(host, c["tracks"], c["ids"], c["kps"], c["poses"], c["cam"])
    assert np.all(tw.counts(pts)["succeeded"] == len(want))
    assert np.linalg.norm(pts["X"] - c["X"], axis=1).max() <= TRUTH_BOUND
    within(worst(want, (pts, res)))
    # one observation of a track of >= 3 views moved by 50 px: the point stays, the error test fails
    o = c["tracks"][0]
    t = int(np.nonzero(np.diff(o) >= 3)[0][0])
    img, idx = int(c["tracks"][1][o[t] + 1]), int(c["tracks"][2][o[t] + 1])
    kps = {i: k.copy() for i, k in c["kps"].items()}
    kps[img][idx, 0] += 50.0
    r = ref.track(c["tracks"][1][o[t]:o[t + 1]], c["tracks"][2][o[t]:o[t + 1]], True, kps, c["poses"], c["cam"])
    pts2, _ = tw.run(host, c["tracks"], c["ids"], kps, c["poses"], c["cam"], select=[t])
    for s in (r["status"], int(pts2[t]["status"])):
        assert s & ref.POINT and not s & ref.ERROR_OK
    assert int(pts2[t]["status"]) == r["status"]


def hand(host, kps, poses, tracks, cam=CAM, params=tw.DEFAULTS):
    ids = np.asarray(sorted(kps), np.int32)
    return tw.run(host, tracks, ids, kps, poses, cam, params), ref.run(tracks, kps, poses, cam, *params)


def test_edge_cases(host):
    c = capture(77)
    o, img, idx, cons = c["tracks"]
    # unposed elements are skipped: without the pose of one image the track equals, bit for bit, the track without that element
    t = int(np.nonzero(np.diff(o) >= 4)[0][0])
    e = slice(int(o[t]), int(o[t + 1]))
    gone = int(img[e][1])
    poses = {i: (None if i == gone else p) for i, p in c["poses"].items()}
    one = (np.asarray([0, e.stop - e.start], np.int64), img[e], idx[e], np.ones(1, np.uint8))
    cut = (np.asarray([0, e.stop - e.start - 1], np.int64), np.delete(img[e], 1), np.delete(idx[e], 1), np.ones(1, np.uint8))
    (p1, r1), w1 = hand(host, c["kps"], poses, one)
    (p2, r2), _ = hand(host, c["kps"], c["poses"], cut)
    assert p1.tobytes() == p2.tobytes() and r1[1] == -1.0 and np.delete(r1, 1).tobytes() == r2.tobytes()
    assert int(p1[0]["n_views"]) == e.stop - e.start - 1 == w1[0]["n_views"] and w1[0]["residuals"][1] == -1.0
    no_key = dict(poses)
    del no_key[gone]                                        # (not listed at all: the same)
    assert hand(host, c["kps"], no_key, one)[0][0].tobytes() == p1.tobytes()
    # fewer posed views than min_views, and fewer than 2: status 0, everything 0, residuals -1
    for prm, ps in (((2.0, 1.5, e.stop - e.start), poses), ((2.0, 1.5, 2), {int(img[e][0]): c["poses"][int(img[e][0])]})):
        (p, r), w = hand(host, c["kps"], ps, one, params=prm)
        assert p.tobytes() == bytes(48) and np.all(r == -1.0) and w[0]["status"] == 0
    # an inconsistent track: status 0
    (p, r), w = hand(host, c["kps"], c["poses"], one[:3] + (np.zeros(1, np.uint8),))
    assert p.tobytes() == bytes(48) and np.all(r == -1.0) and w[0]["status"] == 0
    # identical cameras: no parallax
    same = {i: c["poses"][int(img[e][0])] for i in c["poses"]}
    (p, _), w = hand(host, c["kps"], same, one)
    for s, a in ((int(p[0]["status"]), float(p[0]["tri_angle"])), (w[0]["status"], w[0]["tri_angle"])):
        assert s & ref.ATTEMPTED and not s & ref.ANGLE_OK and (s & ref.SUCCESS) != ref.SUCCESS and a < 1e-3
    # a point behind one camera: DEPTH_OK clear, the verdict follows the reference (which has no depth test)
    X = np.asarray([0.5, 0.3, 5.0])
    P = {1: (np.eye(3), np.zeros(3)), 2: (np.diag([-1.0, 1.0, -1.0]), np.asarray([3.0, 0.0, -2.0]))}
    kp = {}
    for i, (R, tt) in P.items():
        Y = R @ X + tt
        kp[i] = np.asarray([[CAM[0] * Y[0] / Y[2] + CAM[2], CAM[1] * Y[1] / Y[2] + CAM[3]]], np.float32)
    two = (np.asarray([0, 2], np.int64), np.asarray([1, 2], np.int32), np.zeros(2, np.int32), np.ones(1, np.uint8))
    (p, r), w = hand(host, kp, P, two)
    assert int(p[0]["status"]) == w[0]["status"] and w[0]["status"] & ref.POINT and not w[0]["status"] & ref.DEPTH_OK
    assert (w[0]["status"] & ref.SUCCESS) == ref.SUCCESS and np.abs(p[0]["X"] - X).max() < 1e-3
    within(worst(w, (p, r)))


def identical_tracks():
    """Tracks whose cameras AND pixels are all the same (2, 3 and 5 views, two poses): every row of the DLT is one of two rows, the
    normal matrix has rank 2 and the point is whatever the Jacobi sweep leaves in the null space.  As (poses per element, pixels
    float32 [n, 2]) per track, the layout of tests/test_gpu_robust_triangulation.py's laid_out."""
    c, s = np.cos(0.3), np.sin(0.3)
    poses = [(np.eye(3), np.asarray([0.0, 0.0, 6.5])), (np.asarray([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]]), np.asarray([0.2, -0.1, 6.0]))]
    return [([p] * m, np.tile(np.asarray([[1600.25, 1100.5]], np.float32), (m, 1))) for p in poses for m in (2, 3, 5)]


def laid_job(laid):
    """identical_tracks' layout -> (tracks, ids, kps, poses) for the twins: every element an image of its own, its keypoint row 0"""
    n = [len(p) for p, _ in laid]
    ids = np.arange(sum(n), dtype=np.int32) * 3 + 1
    kps = {int(i): np.asarray([xy], np.float32) for i, xy in zip(ids, np.concatenate([xy for _, xy in laid]))}
    poses = {int(i): p for i, p in zip(ids, [p for ps, _ in laid for p in ps]) if p is not None}
    tracks = (np.concatenate([[0], np.cumsum(n)]).astype(np.int64), ids.copy(), np.zeros(len(ids), np.int32), np.ones(len(n), np.uint8))
    return tracks, ids, kps, poses


def test_identical_cameras_and_pixels(host):
    """What the definition fixes on a rank-2 normal matrix: ATTEMPTED, no ANGLE_OK (the centres coincide), and either no POINT or a
    finite X -- in the plain twin and in the robust one (which retries the tracks of three and five views that have no ERROR_OK)."""
    import robust_triangulation_twin as rtw
    tracks, ids, kps, poses = laid_job(identical_tracks())
    pts, res = tw.run(host, tracks, ids, kps, poses, CAM)
    rp = rtw.run(rtw.load_host(), tracks, ids, kps, poses, CAM)[0]
    for p in list(pts) + list(rp):
        s = int(p["status"])
        assert s & ref.ATTEMPTED and not s & ref.ANGLE_OK and (not s & ref.POINT or np.all(np.isfinite(p["X"])))
    print("identical cameras and pixels: status %s (plain), %s (robust)" % (pts["status"].tolist(), rp["status"].tolist()))


# ---- the plain DLT where the conditioning is bad: against mpmath at 50 digits (triangulation_ref.mp_point) --------------------------------
# Worst |X_twin - X_mp| measured on the CPU over the 1439 tracks of the seed-5 capture (0.3 px), python tests/test_triangulation_reference.py
# prints them; the bounds are 16 x the measured values.  (For orientation only: twin - float64 SVD reference is 6.2e-11, 6.9e-8 and 9.9e-4
# at the three shifts, and at 1e6 the SVD reference is the side that drifts.)
#     scene shifted by (mag, -0.7 mag, 0.4 mag)   mag 1e2: 4.7e-11    1e4: 7.6e-9    1e6: 2.9e-7   (the float64 SVD reference: 1.6e-11, 7.0e-8, 9.9e-4)
#     world scaled                                   1e-3: 1.4e-16     1e6: 3.5e-7 (of |X| ~ 6e6)     (the float64 SVD reference: 9.0e-15, 1.2e-3)
MP_BOUNDS = {"shift 1e2": 7.5e-10, "shift 1e4": 1.2e-7, "shift 1e6": 4.6e-6, "scale 1e-3": 2.3e-15, "scale 1e6": 5.6e-6}


def shifted(poses, mag):
    """the scene moved by s = (mag, -0.7 mag, 0.4 mag): X' = X + s, t' = t - R s"""
    s = np.asarray([mag, -0.7 * mag, 0.4 * mag])
    return {i: (R, t - R @ s) for i, (R, t) in poses.items()}


def scaled(poses, k):
    """the world scaled by k: X' = k X, t' = k t"""
    return {i: (R, k * t) for i, (R, t) in poses.items()}


MP_CASES = [("shift 1e2", shifted, 1e2), ("shift 1e4", shifted, 1e4), ("shift 1e6", shifted, 1e6), ("scale 1e-3", scaled, 1e-3), ("scale 1e6", scaled, 1e6)]
_MP = {}


def mp_case(host, name):
    """the twin, the float64 reference and mp_point on the seed-5 capture under one of MP_CASES -> (twin points, reference list, X_mp)"""
    if name not in _MP:
        from concurrent.futures import ProcessPoolExecutor
        import multiprocessing
        _, fn, mag = [m for m in MP_CASES if m[0] == name][0]
        c = capture(5, noise_px=0.3)
        poses = fn(c["poses"], mag)
        pts, _ = tw.run(host, c["tracks"], c["ids"], c["kps"], poses, c["cam"])
        want = ref.run(c["tracks"], c["kps"], poses, c["cam"])
        o, img, idx, _ = c["tracks"]
        jobs = [[ref.observation(c["cam"], c["kps"][int(img[e])][int(idx[e]), :2]) + (np.c_[poses[int(img[e])][0], poses[int(img[e])][1]],)
                 for e in range(int(o[t]), int(o[t + 1]))] for t in range(len(o) - 1)]
        step = 48
        with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1), mp_context=multiprocessing.get_context("fork")) as pool:
            X = np.concatenate(list(pool.map(ref.mp_points, [jobs[a:a + step] for a in range(0, len(jobs), step)])))
        _MP[name] = (pts, want, X)
    return _MP[name]


@pytest.mark.parametrize("name", [m[0] for m in MP_CASES])
def test_shifted_and_scaled_scene_against_mpmath(host, name):
    """Status and n_views equal the reference's on EVERY track; the twin's point within the bound of the 50-digit solution of the same
    stacked rows on every track."""
    pts, want, X = mp_case(host, name)
    for t, r in enumerate(want):
        assert int(pts[t]["status"]) == r["status"] and int(pts[t]["n_views"]) == r["n_views"], (t, int(pts[t]["status"]), r["status"])
    assert np.all(pts["status"] & ref.POINT) and np.all(np.isfinite(X))
    d = float(np.abs(pts["X"] - X).max())
    print("%s: worst |X_twin - X_mp| %.3g, worst |X_ref - X_mp| %.3g" % (name, d, float(np.abs(np.asarray([r["X"] for r in want]) - X).max())))
    assert d <= MP_BOUNDS[name], (d, MP_BOUNDS[name])


def parallax_tracks(thetas, depth=6.5):
    """Two views per track whose rays meet exactly: camera 1 at the origin looks along z, camera 2 is camera 1 turned by theta degrees
    about y around the point (0, 0, depth); both observe the point at the principal point (an exact fp32 pixel), so the angle between
    the rays is theta whatever the pixels' rounding.  -> laid_job's layout"""
    out = []
    xy = np.asarray([[CAM[2], CAM[3]]] * 2, np.float32)
    for th in thetas:
        a = np.deg2rad(th)
        R = np.asarray([[np.cos(a), 0.0, -np.sin(a)], [0.0, 1.0, 0.0], [np.sin(a), 0.0, np.cos(a)]])
        X = np.asarray([0.0, 0.0, depth])
        out.append(([(np.eye(3), np.zeros(3)), (R, np.asarray([0.0, 0.0, depth]) - R @ X)], xy))
    return out


def small_parallax_tracks():
    """two and three views with unit baselines, depth 1e1 .. 1e5, noise-free fp32 pixels"""
    out, depths = [], []
    O = [np.zeros(3), np.asarray([1.0, 0.0, 0.0]), np.asarray([0.0, 1.0, 0.0])]
    for z in (1e1, 1e2, 1e3, 1e4, 1e5):
        X = np.asarray([0.3, 0.2, z])
        for n in (2, 3):
            xy = np.asarray([[CAM[0] * (X - o)[0] / z + CAM[2], CAM[1] * (X - o)[1] / z + CAM[3]] for o in O[:n]], np.float32)
            out.append(([(np.eye(3), -o) for o in O[:n]], xy))
            depths.append(z)
    return out, depths


# Measured on the CPU (test_small_parallax_against_mpmath prints them):
#     depth 1e1 .. 1e5 over unit baselines: relative depth error against mp_point at most 5.8e-16 -> the bound 16 x that
#     tri_angle - the law of cosines in mpmath at the twin's point = tri_angle - the true angle (atan2) in every case: the law of cosines
#     itself is exact to 50 digits there, the loss is the twin's fp64 evaluation of it (the cancellation r1^2 + r2^2 - b^2 under acos):
#     3.6e-15 degrees at 5.7 degrees, 1.2e-13 at 0.57, 2.5e-13 at 0.057, 6.8e-12 at 5.7e-3, 8.9e-10 at 5.7e-4 degrees of parallax
#     at min_angle = 1.5 degrees: |tri_angle - true angle| at most 5.2e-13 degrees over the 240 tracks
ANGLE_ERR = 5.2e-13
DEPTH_REL = 16 * 5.8e-16


def laid_obs(laid):
    return [[ref.observation(CAM, xy[k]) + (np.c_[ps[k][0], ps[k][1]],) for k in range(len(ps))] for ps, xy in laid]


def test_small_parallax_against_mpmath(host):
    """Depth 1e1 .. 1e5 over unit baselines (parallax 5.7 degrees .. 5.7e-4 degrees), min_angle = 0: the twin's depth against mp_point's
    within 16 x the measured relative error; tri_angle against the mpmath evaluation of the SAME law of cosines at the twin's point
    (what the arithmetic loses) and against the true angle by atan2 of cross and dot products (what the definition loses): recorded.
    Then the verdict: 240 two-view tracks whose true angle lies within 1e-6 degrees of min_angle = 1.5 and farther than 16 x the
    measured angle error from it -- ANGLE_OK equals the mpmath verdict on every one."""
    laid, depths = small_parallax_tracks()
    tracks, ids, kps, poses = laid_job(laid)
    pts, _ = tw.run(host, tracks, ids, kps, poses, CAM, (2.0, 0.0, 2))
    Xm = ref.mp_points(laid_obs(laid))
    for t, (ps, _) in enumerate(laid):
        assert int(pts[t]["status"]) & ref.SUCCESS == ref.SUCCESS
        rel = abs(float(pts[t]["X"][2]) - Xm[t][2]) / Xm[t][2]
        cen = [-(R.T @ tt) for R, tt in ps]
        law = float(ref.mp_angle(pts[t]["X"], cen[1], cen[0], True))
        true = float(ref.mp_angle(pts[t]["X"], cen[1], cen[0], False))
        got = float(pts[t]["tri_angle"])
        print("depth %.0e, %d views: relative depth error %.3g, tri_angle %.6g, - law of cosines in mpmath %.3g, - true angle %.3g" % (
            depths[t], len(ps), rel, got, abs(got - law), abs(got - true)))
        assert rel <= DEPTH_REL, rel
    rng = np.random.default_rng(11)
    d = rng.uniform(16 * ANGLE_ERR, 1e-6, 240) * np.where(np.arange(240) % 2, 1.0, -1.0)
    assert len(d) >= 200 and np.all(np.abs(d) > 16 * ANGLE_ERR) and np.all(np.abs(d) <= 1e-6)
    laid = parallax_tracks(1.5 + d)
    tracks, ids, kps, poses = laid_job(laid)
    pts, _ = tw.run(host, tracks, ids, kps, poses, CAM)
    Xm = ref.mp_points(laid_obs(laid))
    worst_err, verdicts = 0.0, [0, 0]
    for t, (ps, _) in enumerate(laid):
        cen = [-(R.T @ tt) for R, tt in ps]
        true = ref.mp_angle(Xm[t], cen[1], cen[0], False)
        assert abs(float(true) - 1.5) <= 1e-6 + 1e-9 and abs(float(true - 1.5)) > 16 * ANGLE_ERR, (t, float(true - 1.5))
        worst_err = max(worst_err, abs(float(pts[t]["tri_angle"] - true)))
        ok = bool(true >= 1.5)
        verdicts[ok] += 1
        assert bool(int(pts[t]["status"]) & ref.ANGLE_OK) == ok, (t, float(true - 1.5), float(pts[t]["tri_angle"]) - 1.5)
    print("at min_angle: worst |tri_angle - true angle| %.3g degrees over %d tracks, verdicts %s" % (worst_err, len(laid), verdicts))
    assert min(verdicts) >= 100


def test_mean_residual_is_the_sum_in_observation_order(host):
    c = capture(77)
    pts, res = tw.run(host, c["tracks"], c["ids"], c["kps"], c["poses"], c["cam"])
    o = c["tracks"][0]
    differs = 0
    for t in range(len(o) - 1):
        s = 0.0
        for v in res[o[t]:o[t + 1]]:
            s = s + float(v)
        assert float(pts[t]["mean_residual"]) == s / float(o[t + 1] - o[t]), t
        differs += float(np.sum(res[o[t]:o[t + 1]][::-1])) / float(o[t + 1] - o[t]) != float(pts[t]["mean_residual"])
    assert differs > 0   # (the order is visible in the bits of this data)


def test_centres_and_angle_pieces(host):
    rng = np.random.default_rng(3)
    for _ in range(200):
        R, t = np.linalg.qr(rng.normal(size=(3, 3)))[0], rng.normal(size=3) * 5
        assert np.abs(tw.centre(host, R, t) - (-R.T @ t)).max() < 1e-14
        X, a, b = rng.normal(size=3) * 3, rng.normal(size=3), rng.normal(size=3)
        assert abs(tw.parallax(host, X, a, b) - ref.angle(X, a, b)) < 1e-9
    assert tw.parallax(host, np.zeros(3), np.zeros(3), np.ones(3)) == 0.0   # NaN -> 0


def test_header_and_library(tmp_path, built_lib):
    from monocularsfm_amd import _lib
    src = tmp_path / "sizes.cpp"
    src.write_text('#include "msfm_match.h"\nstatic_assert(sizeof(msfm_point3d) == 48 && sizeof(msfm_pose_rt) == 104 && '
                   'sizeof(msfm_triangulation_params) == 24 && sizeof(msfm_triangulation_stats) == 80, "sizes");\n'
                   'int main() { return (MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | MSFM_TRI_ERROR_OK | MSFM_TRI_ANGLE_OK | MSFM_TRI_DEPTH_OK) == 31 ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sizes")])
    assert subprocess.run([str(tmp_path / "sizes")]).returncode == 0
    for name in ("msfm_triangulate_tracks", "msfm_fetch_points3d"):
        assert hasattr(built_lib, name) and name in _lib.EXPORTS
    assert _lib.POINT3D.itemsize == 48 and _lib.POSE_RT.itemsize == 104 and _lib.POINT3D is tw.POINT3D and _lib.POSE_RT is tw.POSE_RT
    assert built_lib.msfm_triangulate_tracks(None, None, None, None, 0, None, None) == 1 and built_lib.msfm_fetch_points3d(None, None, None) == 1
    assert list(_lib.succeeded(np.asarray([(31, 2, (0, 0, 0), 0, 0), (19, 2, (0, 0, 0), 0, 0)], _lib.POINT3D))) == [True, False]


if __name__ == "__main__":   # the figures of the module docstring
    h = tw.load_host()
    for args in [dict(seed=s) for s in SEEDS] + [dict(seed=77, cam=CAM_D), dict(seed=5, cam=CAM_D), dict(seed=77, noise_px=0.3), dict(seed=5, noise_px=0.3)]:
        c = capture(**args)
        want = ref.run(c["tracks"], c["kps"], c["poses"], c["cam"])
        print(args, worst(want, tw.run(h, c["tracks"], c["ids"], c["kps"], c["poses"], c["cam"])),
              "margins", min(r["error_margin"] for r in want), min(r["angle_margin"] for r in want),
              "truth", max(float(np.linalg.norm(r["X"] - x)) for r, x in zip(want, c["X"])),
              "succeeded", sum((r["status"] & ref.SUCCESS) == ref.SUCCESS for r in want), "of", len(want))
    for name, _, _ in MP_CASES:   # against mpmath: the figures next to MP_BOUNDS
        pts, want, X = mp_case(h, name)
        print(name, "worst |X_twin - X_mp|", float(np.abs(pts["X"] - X).max()), "worst |X_ref - X_mp|",
              float(np.abs(np.asarray([r["X"] for r in want]) - X).max()))
    test_small_parallax_against_mpmath(h)
