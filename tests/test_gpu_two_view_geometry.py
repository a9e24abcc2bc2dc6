"""The two-view geometry on the device (msfm_set_two_view_geometry, csrc/msfm_verify_pose.hip.h) against its host twin
(TwoViewGeometry, host/GeometricVerification.cpp; the arithmetic of both is csrc/msfm_pose.h):

  * the device's record equals the twin's BYTE FOR BYTE (valid, every integer, every double's bit pattern) over general, planar,
    rotation-only and mixed pairs, pairs of 0 .. 8 matches, batched and streamed, with sub-batch cuts forced by msfm_set_limits;
  * under the model selection a pair whose homography list was kept has valid = 0, the others equal the run without selection;
  * with the feature on, the match lists, verification_stats() and the selection records equal those with it off;
  * a production-shaped call: thousands of pairs in one call (the persistent grid walks its list several times), one of them with
    thousands of kept matches (the selection always runs over global memory: there is no LDS-capacity fallback to miss);
  * the kernel's structural edges (tests/two_view_fixtures.py): staged and kept counts at the ballot's 64 and the passes' 256, rejected
    matches on both sides of those boundaries, tied and widely spread angles under the median's radix selection, tri_max_error = 0,
    and a grid that walks through valid, invalid and H-kept pairs in one sub-batch;
  * the errors of the two entry points, and the records' lifetime across _next / _end."""
import numpy as np
import pytest

import pose_twin
import two_view_fixtures
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


# ---- the edges of tv_pose_kernel (tests/two_view_fixtures.py; tests/test_pose_reference.py checks without a GPU that every scene
# reaches the edge it is named for) ------------------------------------------------------------------------------------------------

def load_cases(ctx, cases):
    kps, _ = load(ctx, [c["scene"] + (None,) for c in cases])
    return kps, np.asarray([(2 * s, 2 * s + 1) for s in range(len(cases))], np.int32)


def removed(raw, cases):
    """The raw lists without the cases' rejected staged positions, in order: what the verified call must return."""
    offs, qt, d = raw
    keep = np.ones(len(qt), bool)
    for p, c in enumerate(cases):
        keep[offs[p] + c["rejected"]] = False
    new = np.r_[0, np.cumsum([c["n"] - len(c["rejected"]) for c in cases])].astype(np.int64)
    return new, qt[keep], d[keep]


def test_kept_list_and_strides_at_their_edges(tctx, host):
    """Staged and kept counts at 63 / 64 / 65, 127 / 128 / 129 (the ballot of 64 that writes the kept list), 255 / 256 / 257, 511 /
    512 / 513 and 769 (the passes strided by 256: a tail of dead lanes, none, one live lane, a third and a fourth stride), with the
    rejected matches on both sides of the 64-boundaries, a whole rejected chunk and the last staged match rejected."""
    cases = two_view_fixtures.exact_sizes() + two_view_fixtures.staged_vs_kept()
    kps, pairs = load_cases(tctx, cases)
    raw = tctx.match_pairs(pairs)
    assert np.diff(raw[0]).tolist() == [c["n"] for c in cases]                      # the staged counts
    assert np.array_equal(raw[1], np.concatenate([c["qt"] for c in cases]))         # and lists: the planted ones
    want = pose_twin.run(host, raw, pairs, kps, CAM)
    lists = removed(raw, cases)
    tctx.set_two_view_geometry(True)

    def check(on, got):
        assert same_records(got, want)
        assert got["n_kept"].tolist() == [c["nk"] for c in cases] and got["valid"].all() and no_nan(got)
        assert got["n_triangulated"].tolist() == [c["nk"] for c in cases]
        assert same(on, lists)

    check(tctx.match_pairs_verified(pairs), tctx.two_view_geometry(len(pairs)))
    tctx.set_limits(max_pairs_per_batch=1)
    check(tctx.match_pairs_verified(pairs), tctx.two_view_geometry(len(pairs)))
    recs, qts, ds, offs = [], [], [], [0]
    for ch in tctx.match_pairs_stream(pairs, verified=True):
        assert ch["n_pairs"] == 1
        recs.append(ch["two_view_geometry"].copy())
        qts.append(ch["qt"])
        ds.append(ch["dist"])
        offs += (offs[-1] + ch["offsets"][1:]).tolist()
    check((np.asarray(offs, np.int64), np.concatenate(qts), np.concatenate(ds)), np.concatenate(recs))
    tctx.set_limits()


def test_median_with_ties_and_spread(tctx, host):
    """The radix selection on runs of equal keys (the remaining rank lands inside a bin on every pass; both middle ranks of an even
    list in one run, and in two), on keys that differ in their exponent bytes, and with tri_max_error = 0: nothing triangulated,
    both means exactly 0, the median what it was."""
    cases = two_view_fixtures.tied_angles() + [two_view_fixtures.depth_spread()]
    kps, pairs = load_cases(tctx, cases)
    raw = tctx.match_pairs(pairs)
    assert np.array_equal(raw[1], np.concatenate([c["qt"] for c in cases]))
    want = pose_twin.run(host, raw, pairs, kps, CAM)
    tctx.set_two_view_geometry(True)
    tctx.match_pairs_verified(pairs)
    got = tctx.two_view_geometry(len(pairs)).copy()
    assert same_records(got, want) and got["valid"].all() and no_nan(got)
    assert got["n_kept"].tolist() == [c["nk"] for c in cases]
    assert {int(n) % 2 for n in got["n_kept"]} == {0, 1}
    for p, c in enumerate(cases):
        p1, p2 = kps[2 * p][c["qt"][:, 0], :2], kps[2 * p + 1][c["qt"][:, 1], :2]
        mask, _ = pose_twin.geometry(host, p1, p2, CAM)
        angles = pose_twin.kept_angles(host, got[p], p1[mask], p2[mask], CAM)
        assert len(set(angles)) == c.get("distinct", c["nk"])
        assert got["median_tri_angle"][p] == pose_twin.median_rule(angles), c["name"]
    assert got["is_initial_candidate"].any() and (got["n_triangulated"] > 0).all()
    tctx.set_two_view_geometry(True, tri_max_error=0.0)
    tctx.match_pairs_verified(pairs)
    got0 = tctx.two_view_geometry(len(pairs))
    assert same_records(got0, pose_twin.run(host, raw, pairs, kps, CAM, params=(100, 0.0, 4.0)))
    assert got0["valid"].all() and not got0["n_triangulated"].any() and not got0["is_initial_candidate"].any()
    assert got0["mean_tri_angle"].tobytes() == got0["mean_residual"].tobytes() == np.zeros(len(pairs)).tobytes()
    assert got0["median_tri_angle"].tobytes() == got["median_tri_angle"].tobytes() and (got0["median_tri_angle"] > 0).all()
    assert got0["R"].tobytes() == got["R"].tobytes() and np.array_equal(got0["n_positive_depth"], got["n_positive_depth"])


def test_grid_walks_through_invalid_and_valid_pairs(tctx, host):
    """One sub-batch of 3 * CUs + 7 pairs, most of them cross pairs that leave the kernel early, the valid own-scene pairs spread over
    the three thirds: workgroups walk valid, invalid, valid and invalid, valid, invalid (the LDS state of one pair must not reach the
    next).  Then with planar scenes under the model selection: H-kept pairs (a third early exit) between E-kept ones."""
    cu = tctx.device_info()["cu_count"]
    zero = np.zeros(1, pose_twin.RECORD).tobytes()
    plain = {}
    for planar_every in (0, 3):
        job = two_view_fixtures.walk_job(cu, planar_every)
        pairs, own = job["pairs"], job["own"]
        tctx.clear_images()
        kps, _ = load(tctx, job["scenes"])
        tctx.set_pipeline(1)
        tctx.set_limits(max_pairs_per_batch=len(pairs))
        tctx.set_model_selection(False)
        raw = tctx.match_pairs(pairs)
        assert sorted(set(np.diff(raw[0])[job["staged_only"]].tolist())) == [3, 4]     # staged, but fewer than an E needs
        want = pose_twin.run(host, raw, pairs, kps, CAM)
        tctx.set_two_view_geometry(True)
        tctx.match_pairs_verified(pairs)
        assert tctx.profile()["sub_batches"] == 1
        got = tctx.two_view_geometry(len(pairs)).copy()
        assert same_records(got, want) and no_nan(got)
        valid = got["valid"] == 1
        assert all(valid[k * cu:(k + 1) * cu].any() for k in range(3)) and valid[3 * cu:].sum() == 0
        assert all(got[p:p + 1].tobytes() == zero for p in np.nonzero(~valid)[0])
        is_own = np.zeros(len(pairs), bool)
        is_own[own] = True
        assert int(valid.sum()) == int(want["valid"][is_own].sum()) >= 40 and not valid[~is_own].any()
        walks = {tuple(valid[b::cu][:3]) for b in range(cu)}
        assert {(True, False, True), (False, True, False)} <= walks
        plain[planar_every] = (got, valid, pairs, job)
    # the planar variant under the selection
    got, valid, pairs, job = plain[3]
    tctx.set_model_selection(True, 0.7)
    tctx.match_pairs_verified(pairs)
    assert tctx.profile()["sub_batches"] == 1
    sel = tctx.two_view_geometry(len(pairs))
    h_kept = tctx.model_selection(len(pairs))[0] == _lib.VERIFY_HOMOGRAPHY
    assert h_kept[job["planar"]].sum() >= 8 and not h_kept[job["own"]][~job["planar"][job["own"]]].any()
    assert not sel["valid"][h_kept].any() and sel[h_kept].tobytes() == zero * int(h_kept.sum())
    assert same_records(sel[~h_kept], got[~h_kept])
    e_own = np.nonzero(sel["valid"] == 1)[0]
    h_own = np.nonzero(h_kept & valid)[0]                      # valid without the selection, H-kept (cleared) with it
    assert len(h_own) >= 8 and any(e_own[0] < p < e_own[-1] for p in h_own)
    walks = {tuple(sel["valid"][b::cu][:3].tolist()) for b in range(cu) if h_kept[b::cu][:3].any()}
    assert any(sum(w) >= 1 for w in walks)                     # a workgroup meets an H-kept pair and an E-kept one
    tctx.set_model_selection(False)
    tctx.set_pipeline()
    tctx.set_limits()
