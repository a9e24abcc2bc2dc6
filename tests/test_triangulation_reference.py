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
    camera the keypoints are re-made through the Brown model.  -> dict"""
    from monocularsfm_amd import synth
    _, protos = synth.rootsift_images(n_images, n_desc, seed=seed, n_proto=n_proto, return_proto=True)
    cams = synth.scene_cameras(n_images, seed=seed)
    kps = synth.scene_keypoints(protos, cams, n_proto, seed=seed, noise_px=noise_px)
    ids = np.asarray([3 * i + 1 for i in range(n_images)], np.int32)
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.6, 1.6, n_proto), rng.uniform(-1.1, 1.1, n_proto), rng.uniform(-1.0, 1.0, n_proto)], 1)
    if any(cam[4:]):
        nrng = np.random.default_rng(seed + 9)
        for i, k in enumerate(kps):
            sel = np.nonzero(np.asarray(protos[i]) >= 0)[0]
            R, t = cams[i][0], cams[i][1]
            Y = X[np.asarray(protos[i])[sel]] @ R.T + t
            xd, yd = emat_ref.distort(cam, Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2])
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
