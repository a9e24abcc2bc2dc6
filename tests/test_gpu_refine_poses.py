"""Pose refinement on the device (msfm_refine_poses, csrc/msfm_refine_poses.hip.h) against the host twin (csrc/msfm_refine_poses.h,
RefinePoses, through tests/refine_poses_twin.py) BYTE FOR BYTE: the pose list, the per-image records, the point records, the
residuals, every integer counter and both cost sums (bit-equal by the fixed summation order).  The twin is fed the device's own
triangulation outputs and the session's own pose list.  Where a test is about a route of the LM loop the twin's trace is asserted next
to the byte comparison: the routes are found on the CPU (tests/refine_poses_fixtures.py, tests/test_refine_poses_reference.py).  The
twin itself is checked against the independent numpy reference in tests/test_refine_poses_reference.py."""
import time

import numpy as np
import pytest

import refine_points_twin as rtw
import refine_poses_fixtures as pfx
import refine_poses_twin as ptw
import registration_twin as regtw
from monocularsfm_amd import _lib
from test_gpu_robust_triangulation import open_ring, second_pass_job

pytestmark = pytest.mark.gpu
CAM = pfx.CAM
THR = pfx.THRESHOLDS


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return ptw.load_host()


def opened(ctx, ids, kps, seen):
    open_ring(ctx, ids, kps, pfx.match_list(seen, ids), seen.shape[0])
    tracks = ctx.tracks()
    assert all(np.array_equal(a, b) for a, b in zip(tracks, pfx.tracks_of(seen, ids)))
    return tracks


def state(ctx, robust):
    pts, res = ctx.points3d()
    return pts, res, (ctx.point_inliers() if robust else None), ctx.pose_list()


def poses_same(ctx, host, ids, kps, tracks, params=ptw.DEFAULTS, fixed=(), thresholds=THR, cam=CAM, robust=False):
    """one msfm_refine_poses on the session's current state against the twin run from that state -> (stats, points, residuals, pose
    list, records, the twin's trace)"""
    p0, r0, m0, l0 = state(ctx, robust)
    st = ctx.refine_poses(*params, fixed=fixed)
    pts, res, m1, l1 = state(ctx, robust)
    rec = ctx.pose_refinements()
    wp, wr, wl, wrec, wc, tr = ptw.run(host, tracks, ids, kps, l0, cam, p0, r0, m0, thresholds, params, fixed, trace=True)
    assert np.array_equal(l1[0], wl[0]) and l1[1].tobytes() == wl[1].tobytes(), np.nonzero(l1[1] != wl[1])[0][:8]
    assert rec.tobytes() == wrec.tobytes(), (rec, wrec)
    assert pts.tobytes() == wp.tobytes(), np.nonzero(pts != wp)[0][:8]
    assert res.tobytes() == wr.tobytes(), np.nonzero(res != wr)[0][:8]
    assert {k: st[k] for k in ptw.COUNT_KEYS} == {k: wc[k] for k in ptw.COUNT_KEYS}, (st, wc)
    assert all(np.float64(st[k]).tobytes() == np.float64(wc[k]).tobytes() for k in ptw.COST_KEYS), (st, wc)
    assert st["refine_ms"] >= st["prepare_ms"] >= 0.0
    if robust:
        assert m1.tobytes() == m0.tobytes()                                                  # the inlier bytes never change
    # what the call may not touch
    moved = (rec["status"] & _lib.POSE_REFINED) != 0
    assert l1[1][~moved].tobytes() == l0[1][~moved].tobytes()                                # a pose that does not stand: not one byte
    assert st["refined"] == moved.sum() and st["cost_after"] <= st["cost_before"]
    assert np.array_equal(pts["X"], p0["X"]) and np.array_equal(pts["n_views"], p0["n_views"])
    keep = _lib.TRI_ROBUST | _lib.TRI_REFINED
    assert np.array_equal(pts["status"] & keep, p0["status"] & keep)
    changed_ids = set(int(i) for i in l1[0][moved])
    o, img = tracks[0], tracks[1]
    in_changed = np.isin(img, sorted(changed_ids)).astype(np.int64)                          # (every kept track has observations)
    touched = (np.add.reduceat(in_changed, o[:-1]) > 0 if len(o) > 1 else np.zeros(0, bool)) & ((p0["status"] & 3) == 3)
    if not moved.any():
        touched[:] = False
    now = _lib.reposed(pts) & ~(_lib.reposed(p0) & ~touched)
    assert np.array_equal(now, touched) and st["points_reposed"] == touched.sum()
    assert pts[~touched].tobytes() == p0[~touched].tobytes()                                 # tracks that touch no changed image
    same_res = ~np.repeat(touched, np.diff(o))
    assert res[same_res].tobytes() == r0[same_res].tobytes()
    ok0, ok1 = _lib.succeeded(p0), _lib.succeeded(pts)
    assert st["points_lost"] == (ok0 & ~ok1).sum() and st["points_gained"] == (~ok0 & ok1).sum()
    return st, pts, res, l1, rec, tr


SIZES = [200, 200, 0, 129, 128, 127, 65, 64, 63, 15, 14, 3, 2, 200]


@pytest.mark.parametrize("min_observations", [15, 3])
def test_fitting_set_sizes_around_the_partials_and_the_butterfly(tctx, host, min_observations):
    """Fourteen listed images whose fitting sets have 200 (image 1 and the LAST image), 0 (image 2: posed, between two full ones --
    equal offsets), 129, 128, 127, 65, 64, 63, 15, 14, 3 and 2 entries: the stride-64 partials with one, two, three and four rounds and
    the butterfly with empty lanes; image 0 is fixed.  min_observations 15 (the 14, 3, 2 are not eligible) and 3 (the 2 is not)."""
    ids, kps, poses, seen = pfx.ring(SIZES, 200)
    tracks = opened(tctx, ids, kps, seen)
    tctx.triangulate_tracks(CAM, pfx.perturbed(poses, 7, keep=(int(ids[0]),)), *THR)
    st, pts, res, lst, rec, tr = poses_same(tctx, host, ids, kps, tracks, (10, 1e-6, min_observations), fixed=[int(ids[0])])
    assert list(rec["n_observations"]) == [0] + SIZES[1:]
    eligible = [n >= min_observations for n in rec["n_observations"]]
    assert list((rec["status"] & _lib.POSE_ATTEMPTED) != 0) == eligible and rec["status"][0] == _lib.POSE_FIXED
    assert st["eligible"] == sum(eligible) == st["refined"] and st["observations"] == sum(SIZES[1:]) and st["images"] == 14
    assert np.all(tr["stop"][eligible] == ptw.STOP_STEP) and st["points_reposed"] == 200
    st2, *_ = poses_same(tctx, host, ids, kps, tracks, (10, 1e-6, min_observations), fixed=[int(ids[0])])      # a repeated call
    assert np.float64(st2["cost_before"]).tobytes() == np.float64(st["cost_after"]).tobytes()
    tctx.tracks_end()


@pytest.mark.parametrize("listed", [1, 4, 5, 24])
def test_listed_images_against_the_waves_of_a_workgroup(tctx, host, listed):
    """24 declared images of which 1, 4, 5 and 24 are listed (one wave each, four waves per workgroup: one wave of one workgroup, a
    full workgroup, a second workgroup with one wave, six workgroups); the last listed image is eligible; max_iters 0, 1, 2 and 10."""
    ids, kps, poses, seen = pfx.ring([80] * 24, 80)
    tracks = opened(tctx, ids, kps, seen)
    some = {int(i): p for i, p in list(sorted(pfx.perturbed(poses, 9).items()))[:listed]}
    for mi in (0, 1, 2, 10):
        tctx.triangulate_tracks(CAM, some, *THR)
        before = [a.tobytes() for a in tctx.points3d()] + [tctx.pose_list()[1].tobytes()]
        assert tctx.pose_list()[1].tobytes() == _lib.pose_table(some)[1].tobytes()            # the caller's poses bit for bit
        st, pts, res, lst, rec, tr = poses_same(tctx, host, ids, kps, tracks, (mi, 1e-6, 15))
        assert st["images"] == listed and st["eligible"] == (listed if listed > 1 else 0)     # (one view triangulates nothing)
        if mi == 0:
            assert [pts.tobytes(), res.tobytes(), lst[1].tobytes()] == before and st["refined"] == 0 == st["points_reposed"]
            assert st["cost_before"] == st["cost_after"] and np.all(rec["stop"][rec["status"] != 0] == ptw.STOP_MAX_ITERS)
        elif listed > 1:
            assert np.all(tr["steps"] <= mi) and (rec[-1]["status"] & _lib.POSE_REFINED)
            assert mi == 10 or np.all(tr["stop"] == ptw.STOP_MAX_ITERS)
    tctx.tracks_end()


@pytest.mark.parametrize("T", [257, 256, 255])
def test_re_verdicted_tracks_at_the_verdict_kernels_lane_edges(tctx, host, T):
    """One image is free, every other one fixed; it sees the tracks 0, 63, 64, 255, 256 (those that exist) and 100 .. 115: the
    re-verdict runs at lanes 0, 63 | 64 and 255 | 256 of rp_verdict_kernel and its neighbours fall through."""
    inside = [t for t in (0, 63, 64, 255, 256) + tuple(range(100, 116)) if t < T]
    ids, kps, poses, seen = pfx.ring([T, T, T, inside, T], T)
    tracks = opened(tctx, ids, kps, seen)
    free = int(ids[3])
    tctx.triangulate_tracks(CAM, pfx.perturbed(poses, 4, keep=tuple(int(i) for i in ids if int(i) != free)), *THR)
    st, pts, *_ = poses_same(tctx, host, ids, kps, tracks, (10, 1e-6, 15), fixed=[int(i) for i in ids if int(i) != free])
    assert st["refined"] == 1 and list(np.nonzero(_lib.reposed(pts))[0]) == sorted(inside)
    tctx.tracks_end()


@pytest.mark.parametrize("name", sorted(pfx.ROUTE_CASES))
def test_routes_found_on_the_cpu(tctx, host, name):
    """The CPU-found routes (tests/refine_poses_fixtures.ROUTE_CASES, asserted against the reference in
    tests/test_refine_poses_reference.py) on their named images, with max_iters 10, 1 and 2: a rejected step followed by an accepted
    one; a pose dropped by the inlier rule beside images below min_observations, a fixed image and an invalid pose; depth-rejected
    steps up to the lambda ceiling; a re-verdict that takes ERROR_OK from points and gives it to others."""
    ids, kps, bad, seen, fixed, thr, at = pfx.route_case(name)
    tracks = opened(tctx, ids, kps, seen)
    for params in (pfx.ROUTE_PARAMS, (1, 1e-4, 6), (2, 1e-4, 6)):
        tctx.triangulate_tracks(CAM, bad, *thr)
        p0 = tctx.points3d()[0]
        st, pts, res, lst, rec, tr = poses_same(tctx, host, ids, kps, tracks, params, fixed=fixed, thresholds=thr)
        if params[0] < 10:
            assert np.all(tr["steps"] <= params[0]) and (tr["stop"] == ptw.STOP_MAX_ITERS).any()
            continue
        if name == "rejected_then_accepted":
            assert tr[at]["accepted_after_rejected"] == 1 and tr[at]["steps"] == 7 and rec[at]["status"] == 3 and st["eligible"] == 1
        elif name == "lost_inliers":
            assert tr[2]["verdict"] == ptw.LOST_INLIERS and rec[2]["inliers_after"] < rec[2]["inliers_before"] and st["rejected_by_inliers"] == 1
            assert rec[0]["status"] == _lib.POSE_FIXED and rec[11]["status"] == 0 and not lst[1][11]["valid"]
            assert ((rec["n_observations"] > 0) & (rec["n_observations"] < 6) & (rec["status"] == 0)).sum() >= 2
        elif name == "ceiling_by_depth":
            assert np.all(tr["stop"][1:6] == ptw.STOP_CEILING) and np.all(tr["depth_rejected"][1:6] == 8) and np.all(rec["iterations"][1:6] == 8)
        else:
            a, b = p0["status"], pts["status"]
            assert list(np.nonzero(((a & 4) != 0) & ((b & 4) == 0))[0]) == [66, 82, 95, 96]
            assert list(np.nonzero(((a & 7) == 3) & ((b & 4) != 0))[0]) == [15, 98, 101, 106] and (st["points_lost"], st["points_gained"]) == (2, 4)
    tctx.tracks_end()


def corrupted_ring(ids, kps, seen, every=5):
    """every `every`-th track's observation in its LAST image moved by 40 px: the robust call rejects it (inlier byte 0)"""
    kps = [k.copy() for k in kps]
    hit = []
    for j in range(0, seen.shape[0], every):
        i = int(np.nonzero(seen[j])[0][-1])
        if seen[j].sum() >= 4:
            kps[i][j, 0] += np.float32(40.0)
            hit.append((j, i))
    return kps, hit


def test_after_the_robust_call_follow_on_calls_and_invalidation(tctx, host):
    """After msfm_triangulate_tracks_robust: rejected observations in changed images get new errors and stay outside every sum, the
    inlier bytes are unchanged; registrations() raises E_STATE after the call while points3d() and point_inliers() work; a following
    refine_points and a following register_images equal their twins fed the new poses; a distorted camera with fx != fy."""
    cam = (2500.0, 2380.0, 1536.0, 1152.0, -0.1, 0.02, 1e-3, -5e-4)
    ids, kps, poses, seen = pfx.ring([150, 150, 150, 100, 70, 40, 150, 20], 150)
    kps, hit = corrupted_ring(ids, kps, seen)
    tracks = opened(tctx, ids, kps, seen)
    thr = (12.0, 1.0)
    tctx.triangulate_tracks(cam, pfx.perturbed(poses, 21, rot=5e-4, trans=3e-3, keep=(int(ids[0]),)), *thr, robust=True)
    m0, r0 = tctx.point_inliers(), tctx.points3d()[1]
    assert (m0 == 0).sum() > 10
    tctx.register_images(cam, [int(ids[2])])
    tctx.registrations()
    st, pts, res, lst, rec, tr = poses_same(tctx, host, ids, kps, tracks, (10, 1e-6, 15), fixed=[int(ids[0])], thresholds=thr, cam=cam, robust=True)
    with pytest.raises(_lib.MsfmError) as e:
        tctx.registrations()
    assert e.value.code == _lib.E_STATE and st["refined"] >= 6
    rejected = (m0 == 0) & (r0 >= 0)
    assert np.all(res[rejected] != r0[rejected])                                             # rewritten ...
    o = tracks[0]
    for t in np.nonzero(_lib.reposed(pts))[0][:40]:                                          # ... and outside the sums
        e_ = res[o[t]:o[t + 1]][m0[o[t]:o[t + 1]] == 1]
        assert abs(pts[t]["mean_residual"] - e_.mean()) < 1e-9
    # a following refine_points sees the new poses
    new = ptw.poses_dict(*lst)
    assert {i: None if p is None else (p[0].tobytes(), p[1].tobytes()) for i, p in new.items() if p is not None} == \
           {i: (p[0].tobytes(), p[1].tobytes()) for i, p in tctx.poses().items()}
    s2 = tctx.refine_points(10, 1e-4)
    p2, r2 = tctx.points3d()
    wp, wr, wc = rtw.run(host, tracks, ids, kps, new, cam, pts, res, m0, thr, (10, 1e-4))
    assert p2.tobytes() == wp.tobytes() and r2.tobytes() == wr.tobytes() and s2["refined"] == wc["refined"] > 0
    assert tctx.pose_list()[1].tobytes() == lst[1].tobytes()
    with pytest.raises(_lib.MsfmError) as e:
        tctx.pose_refinements()                                                              # the point call rebuilt the pose tables
    assert e.value.code == _lib.E_STATE
    # ... and a following register_images the re-verdicted and refined records
    rst = tctx.register_images(cam, [int(ids[2])])
    got = tctx.registrations()
    want = regtw.run(regtw.load_host(), tracks, p2, [int(ids[2])], {int(i): k for i, k in zip(ids, kps)}, cam)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and rst["attempted"] == 1
    tctx.tracks_end()


def test_alternate_three_rounds_equals_the_twins_in_turn(tctx, host):
    ids, kps, poses, seen = pfx.ring([120] * 8, 120)
    tracks = opened(tctx, ids, kps, seen)
    tctx.triangulate_tracks(CAM, pfx.perturbed(poses, 3, keep=(int(ids[0]),)), *THR)
    pts, res, _, lst = state(tctx, False)
    rounds = tctx.alternate(3, fixed=[int(ids[0])], point_params=dict(max_iters=5, step_tol=1e-6), pose_params=dict(max_iters=10, step_tol=1e-6))
    assert len(rounds) == 3
    for a, b in rounds:
        pts, res, wa = rtw.run(host, tracks, ids, kps, ptw.poses_dict(*lst), CAM, pts, res, None, THR, (5, 1e-6))
        pts, res, lst, rec, wb = ptw.run(host, tracks, ids, kps, lst, CAM, pts, res, None, THR, (10, 1e-6, 15), [int(ids[0])])
        assert {k: a[k] for k in rtw.COUNT_KEYS} == {k: wa[k] for k in rtw.COUNT_KEYS}
        assert {k: b[k] for k in ptw.COUNT_KEYS + ptw.COST_KEYS} == {k: wb[k] for k in ptw.COUNT_KEYS + ptw.COST_KEYS}
        assert b["cost_after"] <= b["cost_before"] and b["refined"] == 7
    got = state(tctx, False)
    assert got[0].tobytes() == pts.tobytes() and got[1].tobytes() == res.tobytes() and got[3][1].tobytes() == lst[1].tobytes()
    assert tctx.pose_refinements().tobytes() == rec.tobytes()
    assert rounds[2][1]["cost_after"] < 0.05 * rounds[0][1]["cost_before"]
    tctx.tracks_end()


# ---- the pose list in other orders than the ranks' -------------------------------------------------------------------------------------
def order_job(which):
    if which == "sizes":
        ids, kps, poses, seen = pfx.ring(SIZES, 200)
        return ids, kps, pfx.perturbed(poses, 7, keep=(int(ids[0]),)), seen, [int(ids[0])], THR, (10, 1e-6, 3)
    ids, kps, bad, seen, fixed, thr, _ = pfx.route_case("lost_inliers")
    return ids, kps, bad, seen, fixed, thr, pfx.ROUTE_PARAMS


@pytest.mark.parametrize("which", ["sizes", "lost_inliers"])
def test_pose_list_in_other_orders_than_the_ranks(tctx, host, which):
    """The pose list as an (ids, table) pair in a seeded permutation, with the first, a middle and the last declared image dropped
    (permuted) and with the fixed image last: list position k and pose rank differ, so a mix-up of the two in rp_image_kernel or in
    the host's write-back shows.  Device against twin byte for byte; per image id the device's records and pose entries equal the
    device's own run from the ascending list of the same images; pose_list() returns the caller's order; from the permuted list a
    repeated call and a following refine_points against their twins."""
    t0 = time.perf_counter()
    ids, kps, bad, seen, fixed, thr, params = order_job(which)
    tracks = opened(tctx, ids, kps, seen)
    full = ptw.as_pose_list(bad)
    orders = pfx.list_orders(full[0], fixed[0])
    got = {}
    for name in ("sorted", "dropped_sorted", "fixed_last", "dropped", "permuted"):
        lst = pfx.relisted(full, orders[name])
        tctx.triangulate_tracks(CAM, lst, *thr)
        l0 = tctx.pose_list()
        assert np.array_equal(l0[0], lst[0]) and l0[1].tobytes() == lst[1].tobytes()          # the caller's order, the caller's bytes
        st, pts, res, l1, rec, tr = poses_same(tctx, host, ids, kps, tracks, params, fixed=fixed, thresholds=thr)
        assert list(rec["image_id"]) == list(lst[0]) and st["refined"] >= 3
        assert (st["cost_before"], st["cost_after"]) == pfx.summed_in_list_order(rec)
        got[name] = (st, pts, res, l1, rec)
    for name, base in (("permuted", "sorted"), ("fixed_last", "sorted"), ("dropped", "dropped_sorted")):
        st, pts, res, l1, rec = got[name]
        wst, wpts, wres, wl, wrec = got[base]
        assert list(l1[0]) != list(wl[0])
        assert pfx.by_id(l1[0], rec) == pfx.by_id(wl[0], wrec) and pfx.by_id(l1[0], l1[1]) == pfx.by_id(wl[0], wl[1])
        assert pts.tobytes() == wpts.tobytes() and res.tobytes() == wres.tobytes()
        assert {k: st[k] for k in ptw.COUNT_KEYS} == {k: wst[k] for k in ptw.COUNT_KEYS}
    if which == "lost_inliers":
        assert got["permuted"][0]["rejected_by_inliers"] == 1
    # (the permuted list ran last) a repeated call, then the point refinement under the new poses
    st2, pts, res, lst, rec, tr = poses_same(tctx, host, ids, kps, tracks, params, fixed=fixed, thresholds=thr)
    assert np.array_equal(lst[0], full[0][orders["permuted"]])
    s3 = tctx.refine_points(10, 1e-4)
    p3, r3 = tctx.points3d()
    wp, wr, wc = rtw.run(host, tracks, ids, kps, ptw.poses_dict(*lst), CAM, pts, res, None, thr, (10, 1e-4))
    assert p3.tobytes() == wp.tobytes() and r3.tobytes() == wr.tobytes() and s3["refined"] == wc["refined"] > 0
    after = tctx.pose_list()
    assert np.array_equal(after[0], lst[0]) and after[1].tobytes() == lst[1].tobytes()
    tctx.tracks_end()
    print("list orders (%s): %.2f s" % (which, time.perf_counter() - t0))


def test_alternate_two_rounds_on_a_permuted_list(tctx, host):
    t0 = time.perf_counter()
    ids, kps, poses, seen = pfx.ring([120] * 8, 120)
    tracks = opened(tctx, ids, kps, seen)
    full = ptw.as_pose_list(pfx.perturbed(poses, 3, keep=(int(ids[0]),)))
    given = pfx.relisted(full, pfx.list_orders(full[0], int(ids[0]))["permuted"])
    tctx.triangulate_tracks(CAM, given, *THR)
    pts, res, _, lst = state(tctx, False)
    assert np.array_equal(lst[0], given[0])
    rounds = tctx.alternate(2, fixed=[int(ids[0])], point_params=dict(max_iters=5, step_tol=1e-6), pose_params=dict(max_iters=10, step_tol=1e-6))
    assert len(rounds) == 2
    for a, b in rounds:
        pts, res, wa = rtw.run(host, tracks, ids, kps, ptw.poses_dict(*lst), CAM, pts, res, None, THR, (5, 1e-6))
        pts, res, lst, rec, wb = ptw.run(host, tracks, ids, kps, lst, CAM, pts, res, None, THR, (10, 1e-6, 15), [int(ids[0])])
        assert {k: a[k] for k in rtw.COUNT_KEYS} == {k: wa[k] for k in rtw.COUNT_KEYS}
        assert {k: b[k] for k in ptw.COUNT_KEYS + ptw.COST_KEYS} == {k: wb[k] for k in ptw.COUNT_KEYS + ptw.COST_KEYS}
        assert b["cost_after"] <= b["cost_before"] and b["refined"] == 7
    got = state(tctx, False)
    assert got[0].tobytes() == pts.tobytes() and got[1].tobytes() == res.tobytes()
    assert np.array_equal(got[3][0], given[0]) and got[3][1].tobytes() == lst[1].tobytes()
    assert tctx.pose_refinements().tobytes() == rec.tobytes()
    tctx.tracks_end()
    print("alternate on a permuted list: %.2f s" % (time.perf_counter() - t0))


# ---- the second pass of every grid-stride loop ----------------------------------------------------------------------------------------
def test_image_kernel_second_stride_pass(tctx, host):
    """rp_image_kernel's grid holds at most 8 x CUs workgroups of four waves: with 32 x CUs + 5 listed images the first five waves walk
    to a second image and add its counters to the first one's in registers.  The list is not in rank order; behind the first pass lie
    an eligible image that stands, a fixed one, an unposed one, one below min_observations and a second eligible one, and position
    0 -- the same wave as position 32 x CUs -- is eligible (tests/refine_poses_fixtures.listed_images_case; the placement is asserted
    on the twin's trace, here and in tests/test_refine_poses_reference.py)."""
    t0 = time.perf_counter()
    cus = tctx.device_info()["cu_count"]
    L = 32 * cus + 5
    assert L <= _lib.MAX_IMAGES, "a device of %d CUs needs %d listed images for a second pass: more than MSFM_MAX_IMAGES" % (cus, L)
    ids, kps, lst, matches, want_tracks, fixed, at = pfx.listed_images_case(L, 32 * cus)
    d = np.random.default_rng(1).integers(0, 256, (kps[0].shape[0], 128), dtype=np.uint8)
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), d)
        tctx.upload_keypoints(int(i), kps[k])
    tctx.tracks_begin(ids, add_only=True)
    tctx.tracks_add(*matches)
    tctx.tracks_finish()
    tracks = tctx.tracks()
    assert all(np.array_equal(a, b) for a, b in zip(tracks, want_tracks))
    t1 = time.perf_counter()
    tctx.triangulate_tracks(CAM, lst, *THR)
    st, pts, res, l1, rec, tr = poses_same(tctx, host, ids, kps, tracks, pfx.LISTED_PARAMS, fixed=fixed)
    pfx.assert_placed(at, rec, tr)
    assert st["images"] == L and np.array_equal(l1[0], lst[0]) and not np.array_equal(lst[0], np.sort(lst[0]))
    assert st["eligible"] == (tr["verdict"] != ptw.NOT_ELIGIBLE).sum() > L - 100 and st["iterations"] == tr["steps"].sum()
    tctx.tracks_end()
    print("image kernel's second pass: %d CUs, %d listed images (32 x CUs + 5), %d eligible, refine_ms %.3f; uploads and tracks %.2f s, test %.2f s"
          % (cus, L, st["eligible"], st["refine_ms"], t1 - t0, time.perf_counter() - t0))


def test_key_fill_and_verdict_kernels_second_pass_and_long_partials(tctx, host):
    """rp_key_kernel, rp_fill_kernel and rp_verdict_kernel walk their inputs with a grid of 8 x CUs x 256 lanes: second_pass_job's
    8 x 256 x CUs + 8192 three-view tracks give more observations in the fitting sets, and more tracks, than that; its images hold
    8192 keypoints, so a fitting set runs through 64 and more rounds of the stride-64 partials.  After the robust call, every pose but
    the first of each group turned by 0.2 mrad and moved by 1e-3 units (chosen on the CPU with the twins: every track still succeeds
    under the default 2 px and some images lose an inlier), the first image of each group fixed, default parameters."""
    t0 = time.perf_counter()
    cus = tctx.device_info()["cu_count"]
    lanes = 8 * 256 * cus
    T = lanes + 8192
    ids, kps, poses, lists = second_pass_job(T)
    d = np.random.default_rng(1).integers(0, 256, (8192, 128), dtype=np.uint8)
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), d)
        tctx.upload_keypoints(int(i), kps[k])
    tctx.tracks_begin(ids, add_only=True)
    for l in lists:
        tctx.tracks_add(*l)
    assert tctx.tracks_finish()["tracks_kept"] == T
    tracks = tctx.tracks()
    fixed = [int(i) for i in ids[0::3]]
    tctx.triangulate_tracks(CAM, pfx.perturbed(poses, 23, rot=2e-4, trans=1e-3, keep=tuple(fixed)), robust=True)
    st, pts, res, lst, rec, tr = poses_same(tctx, host, ids, kps, tracks, fixed=fixed, thresholds=(2.0, 1.5), robust=True)
    longest = int(rec["n_observations"][(rec["status"] & _lib.POSE_REFINED) != 0].max())
    print("second pass: %d CUs, T %d, observations in the fitting sets %d (grid %d lanes), re-verdicted behind the grid %d, longest refined "
          "fitting set %d, refined %d of %d, refine_ms %.3f of which prepare %.3f; test %.2f s"
          % (cus, T, st["observations"], lanes, int(_lib.reposed(pts)[lanes:].sum()), longest, st["refined"], st["eligible"], st["refine_ms"],
             st["prepare_ms"], time.perf_counter() - t0))
    assert st["observations"] > lanes                                                        # rp_key's and rp_fill's second pass
    assert _lib.reposed(pts)[lanes:].any()                                                   # rp_verdict's second pass
    assert longest >= 4096                                                                   # 64 and more rounds per partial
    assert st["eligible"] == 2 * len(fixed) and st["refined"] > st["eligible"] // 2
    tctx.tracks_end()


# ---- routes decided by rounding, and the chosen scenes of the reference tests -----------------------------------------------------------
@pytest.mark.parametrize("params", pfx.ILL_PARAMS)
@pytest.mark.parametrize("name", sorted(pfx.ILL_CASES))
def test_ill_conditioned_routes(tctx, host, name, params):
    """Collinear and nearly coincident points (tests/refine_poses_fixtures.ILL_CASES; found and asserted on the twin in
    tests/test_refine_poses_reference.py): 30 and up to 100 evaluated steps per image, a dozen and more accepts directly after a
    reject, each decided in the last bits of a cost -- one ulp of difference between the device's and the twin's arithmetic changes
    the route and every byte after it."""
    t0 = time.perf_counter()
    ids, kps, bad, seen, fixed, thr = pfx.ill_case(name)
    tracks = opened(tctx, ids, kps, seen)
    tctx.triangulate_tracks(CAM, bad, *thr)
    st, pts, res, lst, rec, tr = poses_same(tctx, host, ids, kps, tracks, params, fixed=fixed, thresholds=thr)
    pfx.assert_ill_routes(rec, tr, params[0])
    assert st["eligible"] == 6 and st["iterations"] == tr["steps"].sum() >= 6 * 30
    tctx.tracks_end()
    print("ill-conditioned %s %s: steps %s, accepted after rejected %s; %.2f s"
          % (name, params, tr["steps"].tolist(), tr["accepted_after_rejected"].tolist(), time.perf_counter() - t0))


@pytest.mark.parametrize("name", sorted(pfx.REF_CASES))
def test_chosen_scenes_of_the_reference_tests(tctx, host, name):
    """Fitting sets of 3, 4, 5 and 6 entries, a planar scene, a free camera at the origin and a world of 1e3 units
    (tests/refine_poses_fixtures.REF_CASES): where tests/test_refine_poses_reference.py holds the twin to the reference."""
    t0 = time.perf_counter()
    ids, kps, bad, seen, fixed, thr, params = pfx.ref_case(name)
    tracks = opened(tctx, ids, kps, seen)
    tctx.triangulate_tracks(CAM, bad, *thr)
    st, pts, res, lst, rec, tr = poses_same(tctx, host, ids, kps, tracks, params, fixed=fixed, thresholds=thr)
    assert st["eligible"] == st["refined"] == 6 and np.all(tr["stop"][2:] == ptw.STOP_STEP) and st["points_reposed"] == pfx.REF_T
    if name == "minimal_sets":
        assert list(rec["n_observations"][4:]) == [3, 4, 5, 6]
    tctx.tracks_end()
    print("chosen scene %s: steps %s; %.2f s" % (name, tr["steps"].tolist(), time.perf_counter() - t0))


def test_errors_and_state(tctx):
    def code(fn, *a, **k):
        with pytest.raises(_lib.MsfmError) as e:
            fn(*a, **k)
        return e.value.code

    E = _lib
    ids, kps, poses, seen = pfx.ring([20] * 4, 20)
    for fn in (tctx.refine_poses, tctx.pose_list, tctx.pose_refinements):
        assert code(fn) == E.E_STATE                                                         # no session
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), 20)
    for fn in (tctx.refine_poses, tctx.pose_list, tctx.pose_refinements):
        assert code(fn) == E.E_STATE                                                         # finished, not triangulated
    some = dict(poses)
    some[int(ids[3])] = None                                                                 # an invalid pose in the list
    tctx.triangulate_tracks(CAM, some, *THR)
    assert code(tctx.pose_refinements) == E.E_STATE                                          # no msfm_refine_poses yet
    for kw in (dict(max_iters=-1), dict(max_iters=101), dict(step_tol=-1e-3), dict(step_tol=float("nan")), dict(step_tol=float("inf")),
               dict(min_observations=2), dict(fixed=[5]), dict(fixed=[-1]), dict(fixed=[int(ids[0]), int(ids[0])])):
        assert code(tctx.refine_poses, **kw) == E.E_INVALID
    assert tctx._L.msfm_refine_poses(tctx._h, None, None, -1, None) == E.E_INVALID
    assert tctx._L.msfm_refine_poses(tctx._h, None, None, 0, None) == E.OK                   # NULL params, list and stats
    st = tctx.refine_poses(max_iters=100, step_tol=0.0, min_observations=3, fixed=[int(ids[1])])
    rec = tctx.pose_refinements()
    assert st["images"] == 4 and st["eligible"] == 2 and list(rec["status"] & E.POSE_FIXED) == [0, 4, 0, 0] and rec[3]["status"] == 0
    assert set(tctx.poses()) == set(int(i) for i in ids[:3]) and not tctx.pose_list()[1][3]["valid"]
    tctx.register_images(CAM, [int(ids[0])], min_inliers=3)
    tctx.registrations()
    tctx.refine_poses()
    assert code(tctx.registrations) == E.E_STATE and len(tctx.points3d()[0]) == 20           # registrations gone, points stay
    tctx.tracks_finish()
    for fn in (tctx.refine_poses, tctx.pose_list, tctx.pose_refinements):
        assert code(fn) == E.E_STATE                                                         # after tracks_finish
    tctx.triangulate_tracks(CAM, some, *THR, robust=True)
    tctx.refine_poses(min_observations=3)
    assert len(tctx.point_inliers()) == 80 and len(tctx.pose_refinements()) == 4             # the inlier bytes stay valid
    tctx.set_limits(max_pairs_per_batch=1)
    gen = tctx.match_pairs_stream([(int(ids[0]), int(ids[1])), (int(ids[1]), int(ids[2]))], max_distance=1e9)
    next(gen)
    assert code(tctx.refine_poses) == E.E_STATE                                              # while a series is open
    gen.close()
    tctx.tracks_end()
    assert code(tctx.refine_poses) == E.E_STATE
