"""The two-view geometry on the device (msfm_set_two_view_geometry, csrc/msfm_verify_pose.hip.h) against its host twin
(TwoViewGeometry, host/GeometricVerification.cpp; the arithmetic of both is csrc/msfm_pose.h):

  * the device's record equals the twin's BYTE FOR BYTE (valid, every integer, every double's bit pattern) over general, planar,
    rotation-only and mixed pairs, pairs of 0 .. 8 matches, batched and streamed, with sub-batch cuts forced by msfm_set_limits;
  * under the model selection a pair whose homography list was kept has valid = 0, the others equal the run without selection;
  * with the feature on, the match lists, verification_stats() and the selection records equal those with it off;
  * a production-shaped call: thousands of pairs in one call (the persistent grid walks its list several times), one of them with
    thousands of kept matches (the selection always runs over global memory: there is no LDS-capacity fallback to miss);
  * the errors of the two entry points, and the records' lifetime across _next / _end."""
import numpy as np
import pytest

import pose_twin
from monocularsfm_amd import _lib, synth
from test_gpu_verify_homography import load, same, two_view

pytestmark = pytest.mark.gpu
CAM = (2500.0, 2500.0, 1536.0, 1152.0)


@pytest.fixture(scope="module")
def host(built_lib):
    return pose_twin.load_host()


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    ctx.set_verification_model(_lib.VERIFY_ESSENTIAL, CAM)
    yield ctx
    ctx.close()


def same_records(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def no_nan(rec):
    return all(np.all(np.isfinite(rec[k])) for k in ("R", "t", "median_tri_angle", "mean_tri_angle", "mean_residual"))


def scenes_mixed():
    return [two_view("general", 300, 100, 150, seed=31), two_view("planar", 300, 80, 50, seed=32),
            two_view("rotation", 250, 60, 40, seed=33), two_view("general", 600, 60, 50, seed=34),
            two_view("general", 120, 140, 40, seed=35), two_view("general", 40, 10, 20, seed=36)]


def all_pairs(n_scenes):
    # each scene's own pair both ways, and cross pairs of different scenes (mixed: few or no consistent matches)
    p = [(2 * s, 2 * s + 1) for s in range(n_scenes)] + [(2 * s + 1, 2 * s) for s in range(n_scenes)]
    p += [(2 * s, 2 * ((s + 1) % n_scenes) + 1) for s in range(n_scenes)]
    return np.asarray(p, np.int32)


def test_records_equal_the_twin_byte_for_byte(tctx, host):
    kps, _ = load(tctx, scenes_mixed())
    pairs = all_pairs(6)
    raw = tctx.match_pairs(pairs)
    want = pose_twin.run(host, raw, pairs, kps, CAM)
    off = tctx.match_pairs_verified(pairs)
    tctx.set_two_view_geometry(True)
    on = tctx.match_pairs_verified(pairs)
    got = tctx.two_view_geometry(len(pairs))
    assert same(on, off)                      # the lists do not change
    assert same_records(got, want)
    assert no_nan(got)
    assert int(got["valid"].sum()) >= 8 and got["is_initial_candidate"].any()
    for p in range(len(pairs)):
        if got["valid"][p]:
            assert got["n_kept"][p] == on[0][p + 1] - on[0][p]
            R = got["R"][p].reshape(3, 3)
            assert abs(np.linalg.det(R) - 1) < 1e-12 and abs(np.linalg.norm(got["t"][p]) - 1) < 1e-12
    # other parameters: the same pose and counts of depth, other statistics' verdicts
    tctx.set_two_view_geometry(True, min_num_inliers=10, tri_max_error=0.8, tri_min_angle=1.0)
    tctx.match_pairs_verified(pairs)
    got2 = tctx.two_view_geometry(len(pairs))
    assert same_records(got2, pose_twin.run(host, raw, pairs, kps, CAM, params=(10, 0.8, 1.0)))
    assert not same_records(got2, got)


def test_tiny_pairs(tctx, host):
    """nE from nothing to the smallest lists: pairs of 0 .. 8 matches (below 5 there is no E), and every list size the RANSAC leaves."""
    scenes = [two_view("general", n, 0, 30, seed=50 + n, noise=0.2) for n in range(0, 9)] + [two_view("general", 12, 3, 30, seed=70)]
    kps, _ = load(tctx, scenes)
    pairs = np.asarray([(2 * s, 2 * s + 1) for s in range(len(scenes))], np.int32)
    raw = tctx.match_pairs(pairs)
    tctx.set_two_view_geometry(True, min_num_inliers=5)
    tctx.match_pairs_verified(pairs)
    got = tctx.two_view_geometry(len(pairs))
    assert same_records(got, pose_twin.run(host, raw, pairs, kps, CAM, params=(5, 2.0, 4.0)))
    counts = np.diff(raw[0])
    assert not got["valid"][counts < 5].any() and no_nan(got)
    assert got["valid"].any()


def test_cuts_and_streaming(tctx, host):
    kps, _ = load(tctx, scenes_mixed())
    pairs = all_pairs(6)
    want = pose_twin.run(host, tctx.match_pairs(pairs), pairs, kps, CAM)
    tctx.set_two_view_geometry(True)
    for limit in (1, 2, 5):
        tctx.set_limits(max_pairs_per_batch=limit)
        tctx.match_pairs_verified(pairs)
        assert same_records(tctx.two_view_geometry(len(pairs)), want)
        recs = []
        for ch in tctx.match_pairs_stream(pairs, verified=True):
            assert ch["n_pairs"] <= limit and len(ch["two_view_geometry"]) == ch["n_pairs"]
            recs.append(ch["two_view_geometry"].copy())
        assert same_records(np.concatenate(recs), want)
    tctx.set_limits()
    gen = tctx.match_pairs_stream(pairs[:1], verified=False)
    assert "two_view_geometry" not in next(gen)
    gen.close()


def test_with_model_selection(tctx):
    load(tctx, scenes_mixed())
    pairs = all_pairs(6)
    tctx.set_two_view_geometry(True)
    tctx.match_pairs_verified(pairs)
    plain = tctx.two_view_geometry(len(pairs)).copy()
    stats_plain = tctx.verification_stats()
    tctx.set_two_view_geometry(False)
    tctx.set_model_selection(True, 0.7)
    sel_off = tctx.match_pairs_verified(pairs)
    rec_off = tctx.model_selection(len(pairs))
    stats_off = tctx.verification_stats()
    tctx.set_two_view_geometry(True)
    sel_on = tctx.match_pairs_verified(pairs)
    rec_on = tctx.model_selection(len(pairs))
    assert same(sel_on, sel_off) and all(np.array_equal(a, b) for a, b in zip(rec_on, rec_off))
    assert tctx.verification_stats() == stats_off
    got = tctx.two_view_geometry(len(pairs))
    h_kept = rec_on[0] == _lib.VERIFY_HOMOGRAPHY
    assert 0 < int(h_kept.sum()) < len(pairs)
    assert not got["valid"][h_kept].any() and got[h_kept].tobytes() == np.zeros(int(h_kept.sum()), got.dtype).tobytes()
    assert same_records(got[~h_kept], plain[~h_kept])
    # and with the feature off the stats of the plain call are what they were
    tctx.set_model_selection(False)
    tctx.set_two_view_geometry(False)
    tctx.match_pairs_verified(pairs)
    assert tctx.verification_stats() == stats_plain


def test_production_shape(tctx, host):
    """2560 pairs in one call over 64 images of ~700 rows (the grid of one workgroup per CU walks its list about ten times), and one
    pair of two 9000-row images with ~8000 kept matches (more angles than 64 KiB of LDS would hold)."""
    n_img = 64
    cams = synth.scene_cameras(n_img, seed=5)
    rng = np.random.default_rng(5)
    n_points = 1200
    ids = [np.sort(rng.choice(n_points, 700, replace=False)) for _ in range(n_img)]
    kps = synth.scene_keypoints(ids, cams, n_points, seed=5, noise_px=0.5)
    proto = synth.rootsift_images(1, [n_points], seed=5, n_proto=4 * n_points)[0]
    for i in range(n_img):
        d = np.abs(proto[ids[i]] + rng.normal(0, 0.004, (700, 128)).astype(np.float32))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        tctx.upload_image(i, d.astype(np.float32))
        tctx.upload_keypoints(i, kps[i])
    big = two_view("general", 8400, 300, 300, seed=77)
    tctx.upload_image(n_img, big[0])
    tctx.upload_keypoints(n_img, big[1])
    tctx.upload_image(n_img + 1, big[2])
    tctx.upload_keypoints(n_img + 1, big[3])
    kps = list(kps) + [big[1], big[3]]
    pairs = [(i, j) for i in range(n_img) for j in range(n_img) if i != j][:2559] + [(n_img, n_img + 1)]
    pairs = np.asarray(pairs, np.int32)
    raw = tctx.match_pairs(pairs)
    want = pose_twin.run(host, raw, pairs, kps, CAM)
    off = tctx.match_pairs_verified(pairs)
    tctx.set_two_view_geometry(True)
    on = tctx.match_pairs_verified(pairs)
    got = tctx.two_view_geometry(len(pairs))
    assert same(on, off)
    assert same_records(got, want)
    assert got["n_kept"][-1] > 8192 - 1000 and got["valid"][-1] == 1
    assert int(got["valid"].sum()) > 2000 and no_nan(got)


def test_errors_and_lifetime(tctx):
    load(tctx, scenes_mixed()[:2])
    pairs = np.asarray([(0, 1), (2, 3), (1, 0)], np.int32)
    L, h = tctx._L, tctx._h

    def code(enable, mi=100, err=2.0, ang=4.0):
        return L.msfm_set_two_view_geometry(h, int(enable), _lib.C.byref(_lib.TwoViewParams(mi, 0, err, ang)))

    for bad in (dict(mi=-1), dict(err=-1.0), dict(err=float("nan")), dict(ang=float("inf")), dict(ang=-0.5)):
        assert code(1, **bad) == _lib.E_INVALID
    assert L.msfm_set_two_view_geometry(h, 2, None) == _lib.E_INVALID
    assert L.msfm_set_two_view_geometry(h, 1, None) == _lib.OK      # NULL: the defaults
    # the model cannot leave E while the feature is on
    assert L.msfm_set_verification_model(h, _lib.VERIFY_FUNDAMENTAL, None) == _lib.E_INVALID
    assert L.msfm_set_verification_model(h, _lib.VERIFY_HOMOGRAPHY, None) == _lib.E_INVALID
    assert code(0) == _lib.OK
    tctx.set_verification_model(_lib.VERIFY_FUNDAMENTAL)
    assert code(1) == _lib.E_INVALID                                   # enabled without the essential-matrix model
    tctx.set_verification_model(_lib.VERIFY_ESSENTIAL, CAM)
    # fetch: E_STATE until a verified call has run with it
    tctx.match_pairs_verified(pairs)
    assert L.msfm_fetch_two_view_geometry(h, None) == _lib.E_STATE
    assert code(1) == _lib.OK
    assert L.msfm_fetch_two_view_geometry(h, None) == _lib.E_STATE
    tctx.match_pairs_verified(pairs)
    whole = tctx.two_view_geometry(3).copy()
    tctx.match_pairs(pairs)                                            # an unverified call: no records
    assert L.msfm_fetch_two_view_geometry(h, None) == _lib.E_STATE
    # the streaming form: the records are the last chunk's; a setter inside the series is E_STATE
    tctx.set_limits(max_pairs_per_batch=1)
    gen = tctx.match_pairs_stream(pairs, verified=True)
    first = next(gen)
    assert same_records(first["two_view_geometry"], whole[:1]) and same_records(tctx.two_view_geometry(1), whole[:1])
    assert code(0) == _lib.E_STATE
    second = next(gen)
    assert same_records(second["two_view_geometry"], whole[1:2])
    gen.close()                                                        # msfm_match_pairs_end
    tctx.set_limits()
    assert code(0) == _lib.OK
    tctx.match_pairs_verified(pairs)
    assert L.msfm_fetch_two_view_geometry(h, None) == _lib.E_STATE
