"""Map extension on the device (msfm_extend_points, csrc/msfm_extend.hip.h) against the host twin (csrc/msfm_extend.h, ExtendPoints,
through tests/extend_twin.py): records, residuals, inlier bytes, the pose list and every counter BYTE FOR BYTE.  The twin is fed the
device's own state before the call (records, residuals, bytes where the session has them, the pose list), which the earlier GPU tests
hold equal to their twins.  Where a test is about a route, the twin's trace is asserted next to the byte comparison.  The twin itself
is checked against the independent numpy reference in tests/test_extend_points_reference.py."""
import time

import numpy as np
import pytest

import extend_fixtures as efx
import extend_twin as etw
import refine_points_twin as rtw
import refine_poses_fixtures as pfx
import refine_poses_twin as ptw
import registration_twin as regtw
from monocularsfm_amd import _lib
from test_gpu_robust_triangulation import open_ring, ring_job, second_pass_job

pytestmark = pytest.mark.gpu
CAM = efx.CAM
THR = efx.THRESHOLDS


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return etw.load_host()


def code(fn, *a, **k):
    with pytest.raises(_lib.MsfmError) as e:
        fn(*a, **k)
    return e.value.code


def bytes_or_none(ctx):
    try:
        return ctx.point_inliers()
    except _lib.MsfmError as e:
        assert e.code == _lib.E_STATE
        return None


def state(ctx):
    """(points, residuals, bytes or None, (ids, POSE_RT list)) of the session"""
    return ctx.points3d() + (bytes_or_none(ctx), ctx.pose_list())


def same_state(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and \
        a[3][0].tobytes() == b[3][0].tobytes() and a[3][1].tobytes() == b[3][1].tobytes()


def extend_same(ctx, host, ids, kps, tracks, new, mh, cam=CAM, thr=THR):
    """one msfm_extend_points on the session's current state against the twin run from that state
    -> (stats, points, residuals, bytes, the twin's trace, the state before)"""
    p0, r0, m0, lst0 = before = state(ctx)
    st = ctx.extend_points(new, mh)
    if mh is None:
        mh = ctx._tri_route                      # the route of the context's last triangulate_tracks
    pts, res, mask, lst = state(ctx)
    wp, wr, wm, wc, wl, tr = etw.run(host, tracks, ids, kps, lst0, new, cam, p0, r0, m0, thr, mh, trace=True)
    assert pts.tobytes() == wp.tobytes(), np.nonzero(pts != wp)[0][:8]
    assert res.tobytes() == wr.tobytes(), np.nonzero(res != wr)[0][:8]
    assert mask is not None and mask.tobytes() == wm.tobytes(), np.nonzero(mask != wm)[0][:8]
    assert lst[0].tobytes() == wl[0].tobytes() and lst[1].tobytes() == wl[1].tobytes(), (lst[0], wl[0])
    keys = etw.COUNT_KEYS + ("images_added", "succeeded", "observations_used")
    assert {k: st[k] for k in keys} == {k: wc[k] for k in keys}, (st, wc)
    assert st["extend_ms"] >= st["prepare_ms"] >= 0.0
    # untouched tracks bit for bit, continued ones keep X and every bit
    o = tracks[0]
    per_obs = np.repeat(tr["kind"], np.diff(o))
    same = tr["kind"] == etw.KIND_UNTOUCHED
    assert pts[same].tobytes() == p0[same].tobytes() and res[per_obs == 0].tobytes() == r0[per_obs == 0].tobytes()
    if m0 is not None:
        assert mask[per_obs == 0].tobytes() == m0[per_obs == 0].tobytes()
    cont = tr["kind"] == etw.KIND_CONTINUE
    assert pts["X"][cont].tobytes() == p0["X"][cont].tobytes() and np.all((pts["status"][cont] & p0["status"][cont]) == p0["status"][cont])
    return st, pts, res, mask, tr, before


def full_equals_created(host, ids, kps, lst, rows, tracks_list, pts, res, mask, tr, mh, cam=CAM, thr=THR):
    """the device invariant: on a second context with the same tracks, the full triangulation under the enlarged pose list gives every
    created track's record (minus the bit), residuals and bytes"""
    ctx2 = _lib.Context(0)
    try:
        open_ring(ctx2, ids, kps, tracks_list, rows)
        ctx2.triangulate_tracks(cam, lst, *thr, robust=mh > 0, max_hypotheses=max(mh, 1))
        fp, fr = ctx2.points3d()
        o = ctx2.tracks()[0]
        made = tr["kind"] == etw.KIND_CREATE
        per = np.repeat(made, np.diff(o))
        assert made.any() and etw.without_bit(pts[made]).tobytes() == fp[made].tobytes() and res[per].tobytes() == fr[per].tobytes()
        if mh > 0:
            assert mask[per].tobytes() == ctx2.point_inliers()[per].tobytes()
        else:
            used = np.repeat((fp["status"] & 1) != 0, np.diff(o)) & np.isin(ctx2.tracks()[1], [int(i) for i, p in zip(*lst) if p["valid"]])
            assert np.array_equal(mask[per], used[per].astype(np.uint8))
    finally:
        ctx2.close()


def some(poses, ids, positions):
    return {int(ids[p]): poses[int(ids[p])] for p in positions}


# ---- track counts: the wave and block edges of ext_track_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("robust_session", (False, True))
def test_track_counts_at_the_wave_and_block_edges(tctx, host, robust_session):
    """T = 1, 63, 64, 65, 255, 256, 257 kept tracks; the touched tracks sit at the lanes 0, 63 | 64, 255 | 256 (length 5: they see the new
    images 3 and 4), every other track has length 3 and stays untouched.  Lanes 0, 64 and 256 are continued; lanes 63 and 255 carry an
    observation moved by 30 px across the epipolar lines in image 1 -- no ERROR_OK on the plain session: created, and retried with
    max_hypotheses 8; on the robust session (max_hypotheses 0) the triangulation has rescued them: continued."""
    for T in (257, 256, 255, 65, 64, 63, 1):
        lengths = [5 if j in (0, 63, 64, 255, 256) else 3 for j in range(T)]
        moved = {j: [(1, 0.0, 30.0)] for j in (63, 255) if j < T}
        ids, kps, poses, lst = ring_job(lengths, moved=moved)
        assert open_ring(tctx, ids, kps, lst, T)["tracks_kept"] == T
        tracks = tctx.tracks()
        tctx.triangulate_tracks(CAM, some(poses, ids, (0, 1, 2)), *THR, robust=robust_session, max_hypotheses=8)
        mh = 0 if robust_session else 8
        st, pts, res, mask, tr, _ = extend_same(tctx, host, ids, kps, tracks, some(poses, ids, (3, 4)), mh)
        touched = [j for j in (0, 63, 64, 255, 256) if j < T]
        assert np.array_equal(np.nonzero(tr["kind"])[0], touched) and st["tracks_touched"] == len(touched) and st["images_added"] == 2
        for j in touched:
            want = etw.KIND_CREATE if (j in moved and not robust_session) else etw.KIND_CONTINUE
            assert tr[j]["kind"] == want and tr[j]["new_observations"] == 2, (T, j, tr[j])
            assert _lib.extended(pts)[j] and _lib.succeeded(pts)[j]
        if not robust_session:
            assert st["retried"] == len(moved) and all(tr[j]["route"] == etw.ROUTE_ROBUST for j in moved)
        tctx.tracks_end()


def test_second_grid_stride_pass(tctx, host):
    """ext_track_kernel's grid holds 8 x CUs x 256 lanes: with 8192 tracks more its first 32 workgroups run a second pass of the
    wave-uniform t0 loop; ref_obs_kernel runs its second pass too.  Every other group has the images 0 and 1 posed at the triangulation
    (2.4 degrees, min_angle 3: a point without ANGLE_OK, created by the third image), the groups between 0 and 2 (4.8 degrees:
    standing, continued into image 1).  Every track of the last 8192 has an observation moved by 40 px: the created ones are retried from the
    second pass' list (the last group is a created one), the continued ones reject it."""
    t0 = time.time()
    cus = tctx.device_info()["cu_count"]
    T = 8 * 256 * cus + 8192
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
    g = np.arange(len(ids)) // 3
    late = np.where((g[-1] - g) % 2 == 0, 2, 1)           # the position within its group of the image that arrives late (last group: 2)
    first = {int(i): poses[int(i)] for k, i in enumerate(ids) if k % 3 != late[k]}
    new = {int(i): poses[int(i)] for k, i in enumerate(ids) if k % 3 == late[k]}
    thr = (2.0, 3.0, 2)
    tctx.triangulate_tracks(CAM, first, *thr)
    st, pts, _, _, tr, _ = extend_same(tctx, host, ids, kps, tracks, new, 8, thr=thr)
    assert st["tracks_touched"] == T and st["created_attempted"] >= T // 8 and st["continued"] >= T // 8
    tail = tr[T - 8192:]
    # (where the moved observation is one of the two posed at the triangulation, their point absorbs it and may stand: continued)
    assert (tail["route"] == etw.ROUTE_ROBUST).sum() > 2048 and _lib.extended(pts)[T - 8192:].any()
    print("second pass: T %d, extend_ms %.3f of which prepare %.3f, retried %d, wall %.1f s" %
          (T, st["extend_ms"], st["prepare_ms"], st["retried"], time.time() - t0))
    tctx.tracks_end()


# ---- where the new observation sits in its track ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("where,new_at", (("first", (0,)), ("middle", (1, 32)), ("last", (1, 2, 63, 64, 128))))
def test_new_observation_first_middle_last(tctx, host, where, new_at):
    """Tracks of 2, 3, 64, 65 and 129 elements (two of each; the second 65-view track has an observation moved across the epipolar lines
    in image 5) on a plain session with max_hypotheses 8.  The new images are the first element of every track; a middle one (image 1
    of the 3-view tracks, 1 and 32 of the long ones); the last one of every track (1, 2, 63, 64, 128).  A 2-element track has one old
    view plus one new: created.  The moved 65-view track fails ERROR_OK at the triangulation: created, retried over two LDS tiles."""
    lengths = [2, 3, 64, 65, 129, 2, 3, 64, 65, 129]
    ids, kps, poses, lst = ring_job(lengths, moved={8: [(5, 0.0, 30.0)]})
    open_ring(tctx, ids, kps, lst, len(lengths))
    tracks = tctx.tracks()
    old = [p for p in range(129) if p not in new_at]
    tctx.triangulate_tracks(CAM, some(poses, ids, old), *THR)
    p0 = tctx.points3d()[0]
    assert p0[0]["status"] == 0 and p0[5]["status"] == 0 and not (p0[8]["status"] & _lib.TRI_ERROR_OK)
    st, pts, res, mask, tr, _ = extend_same(tctx, host, ids, kps, tracks, some(poses, ids, new_at), 8)
    o = tracks[0]
    for t, n in enumerate(lengths):
        at = [k for k in range(n) if k in new_at]
        assert tr[t]["new_observations"] == len(at)
        if where == "first":
            assert at == [0]
        if where == "last":
            assert at[-1] == n - 1
    assert tr[0]["kind"] == tr[5]["kind"] == etw.KIND_CREATE and _lib.extended(pts)[0] and pts[0]["n_views"] == 2
    assert tr[8]["kind"] == etw.KIND_CREATE and tr[8]["route"] == etw.ROUTE_ROBUST and pts[8]["n_views"] == 64 and _lib.succeeded(pts)[8]
    assert mask[o[8] + 5] == 0 and st["retried"] >= 1
    for t in (2, 3, 4, 7, 9):
        assert tr[t]["kind"] == etw.KIND_CONTINUE and tr[t]["accepted"] == tr[t]["new_observations"] and pts[t]["n_views"] == lengths[t]
    tctx.tracks_end()


# ---- continue routes --------------------------------------------------------------------------------------------------------------------
def test_continue_routes(tctx, host):
    """Six tracks through the images 0 .. 5, of which 1, 2, 3 are posed at the robust triangulation; the new images are 0, 4 and 5.
    Image 5's camera is turned round (the scene lies behind it and projects onto its keypoints): every track's observation there is
    rejected by DEPTH, with a small error.  Track 0: its two other new observations are accepted.  Track 1: its observation in image 4
    is 30 px off: rejected by error.  The session went through refine_points and refine_poses first, and track 4 was retried at the
    triangulation: the continued tracks keep REFINED, REPOSED and ROBUST.  tri_angle changes: image 0 arrives in front of the old
    views, and the scan now stops at an earlier pair than (3, 1).  A second session, whose tracks see the images 1, 2, 3 and the
    turned one alone: none accepted, the record stays bit for bit, the new slot and byte are written."""
    lengths = [6] * 6
    ids, kps, poses, lst = ring_job(lengths, moved={1: [(4, 30.0, 30.0)], 4: [(2, 0.0, 30.0)]}, turned=(5,))
    open_ring(tctx, ids, kps, lst, 6)
    tracks = tctx.tracks()
    o = tracks[0]
    tctx.triangulate_tracks(CAM, some(poses, ids, (1, 2, 3)), *THR, robust=True, max_hypotheses=8)
    tctx.refine_points()
    tctx.refine_poses(min_observations=3, fixed=[int(ids[1])])
    p0 = tctx.points3d()[0]
    bits = _lib.TRI_REFINED | _lib.TRI_REPOSED
    assert (p0["status"][4] & _lib.TRI_ROBUST) and np.all((p0["status"] & bits) == bits) and np.all(_lib.succeeded(p0))
    st, pts, res, mask, tr, before = extend_same(tctx, host, ids, kps, tracks, some(poses, ids, (0, 4, 5)), 0)
    assert np.all(tr["kind"] == etw.KIND_CONTINUE) and st["continued"] == 6 and st["created_attempted"] == 0
    assert np.all((pts["status"] & bits) == bits) and (pts["status"][4] & _lib.TRI_ROBUST) and np.all(_lib.extended(pts))
    assert tr[0]["accepted"] == 2 and tr[1]["accepted"] == 1                                  # image 5 by depth; track 1's image 4 by error
    assert mask[o[1] + 4] == 0 and res[o[1] + 4] > THR[0] and np.all(mask[o[:-1] + 5] == 0) and np.all(res[o[:-1] + 5] < THR[0])
    assert st["observations_rejected"] == 7 and st["observations_added"] == 11
    assert np.all(pts["tri_angle"] != p0["tri_angle"]) and np.all(pts["n_views"] == p0["n_views"] + tr["accepted"])
    tctx.tracks_end()
    # none accepted: tracks through 1, 2, 3 and the turned image alone
    ids, kps, poses, seen = pfx.ring([4, 4, 4, 4, 0, 4], 4)
    seen[:, 0] = False
    _, turned_kps, turned_poses, _ = ring_job([6] * 4, turned=(5,))
    kps[5], poses[int(ids[5])] = turned_kps[5], turned_poses[int(ids[5])]
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), 4)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, ids, (1, 2, 3)), *THR)
    st, pts, res, mask, tr, before = extend_same(tctx, host, ids, kps, tracks, some(poses, ids, (5,)), 0)
    assert np.all(tr["kind"] == etw.KIND_CONTINUE) and np.all(tr["accepted"] == 0) and st["continued"] == 0 and st["observations_rejected"] == 4
    assert pts.tobytes() == before[0].tobytes() and not _lib.extended(pts).any()
    last = tracks[0][1:] - 1
    assert np.all(before[1][last] == -1.0) and np.all(res[last] >= 0.0) and np.all(mask[last] == 0)
    tctx.tracks_end()


# ---- create routes and the retry list -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("retried", (0, 1, 4, 5))
def test_create_routes_and_the_retry_list(tctx, host, retried):
    """The images 1, 2, 3 are posed at the plain triangulation, 0 and 4 arrive.  Tracks of length 2 (images 0, 1: one posed view, never
    attempted), 3 (images 0, 1, 2: a point below min_angle that gains ANGLE_OK with image 0) and 5; `retried` of the 5-view tracks have
    an observation moved across the epipolar lines in image 2: no ERROR_OK at the triangulation, created and -- max_hypotheses 8 --
    retried: 0 entries (trr_retry_kernel is not launched), 1 (one wave), 4 (a full workgroup), 5 (a second workgroup with one live wave)."""
    lengths = [2, 3, 5, 5, 5, 5, 5, 5, 2, 3]
    moved = {t: [(2, 0.0, 30.0)] for t in range(2, 2 + retried)}
    ids, kps, poses, lst = ring_job(lengths, moved=moved)
    open_ring(tctx, ids, kps, lst, len(lengths))
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, ids, (1, 2, 3)), *THR)
    p0 = tctx.points3d()[0]
    assert p0["status"][0] == 0 and (p0["status"][1] & 10) == 2 and all(not (p0["status"][t] & 4) for t in moved)
    st, pts, res, mask, tr, _ = extend_same(tctx, host, ids, kps, tracks, some(poses, ids, (0, 4)), 8)
    assert st["retried"] == retried and [t for t in range(10) if tr[t]["route"] == etw.ROUTE_ROBUST] == sorted(moved)
    # (a 2-element track is created from two views 1.2 degrees apart: below min_angle, it does not succeed)
    assert st["created_attempted"] == 4 + retried and st["created"] == 2 + retried and np.all(_lib.extended(pts))
    assert np.array_equal(np.nonzero(~_lib.succeeded(pts))[0], [0, 8])
    assert (pts["status"][1] & _lib.TRI_ANGLE_OK) and pts["n_views"][0] == 2 and all(pts["n_views"][t] == 4 for t in moved)
    full_equals_created(host, ids, kps, tctx.pose_list(), len(lengths), lst, pts, res, mask, tr, 8)
    tctx.tracks_end()


def test_plain_route_on_a_robust_session(tctx, host):
    """max_hypotheses 0 after the robust triangulation: created tracks take the plain route (no ROBUST bit, bytes 1 on every used
    observation), the device invariant against the plain full triangulation"""
    ids, kps, poses, tracks_, seen = efx.scene()
    lst = pfx.match_list(seen, ids)
    open_ring(tctx, ids, kps, lst, efx.T)
    tracks = tctx.tracks()
    assert np.array_equal(tracks[1], tracks_[1])
    tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR, robust=True, max_hypotheses=64)
    st, pts, res, mask, tr, _ = extend_same(tctx, host, ids, kps, tracks, some(poses, ids, efx.ONE[0]), 0)
    made = tr["kind"] == etw.KIND_CREATE
    assert made.sum() >= 32 and st["retried"] == 0 and not (pts["status"][made] & _lib.TRI_ROBUST).any() and st["observations_rejected"] >= 3
    full_equals_created(host, ids, kps, tctx.pose_list(), efx.T, lst, pts, res, mask, tr, 0)
    tctx.tracks_end()


# ---- no-ops, poses and order ------------------------------------------------------------------------------------------------------------
def test_no_op_calls_and_the_bytes_of_a_plain_session(tctx, host):
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR)
    s0 = state(tctx)
    assert s0[2] is None
    for new in ({}, {int(ids[0]): None, int(ids[5]): None}):
        st, pts, res, mask, tr, _ = extend_same(tctx, host, ids, kps, tracks, new, 8)
        s1 = state(tctx)
        assert same_state(s0[:2] + (None,) + s0[3:], s1[:2] + (None,) + s1[3:]) and st["tracks_touched"] == st["images_added"] == 0
        want = np.repeat((pts["status"] & 1) != 0, np.diff(tracks[0])) & np.isin(tracks[1], [int(ids[p]) for p in efx.FIRST])
        assert np.array_equal(mask, want.astype(np.uint8))                      # fetchable, and equal to their definition
        assert st["succeeded"] == int(_lib.succeeded(pts).sum()) and st["observations_used"] == int(pts["n_views"].sum())
    # the refinements take their fitting sets from the bytes now: the same results as on the plain session without them
    pr = tctx.refine_points()
    got = tctx.points3d()
    tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR)
    assert tctx.refine_points()["refined"] == pr["refined"] and all(a.tobytes() == b.tobytes() for a, b in zip(got, tctx.points3d()))
    tctx.tracks_end()


@pytest.mark.parametrize("robust_session", (False, True))
def test_every_call_on_a_map_without_tracks(tctx, robust_session):
    """min_length above every track's length: the session finishes with no kept track.  After the triangulation every call of the
    reconstruction stage succeeds without a launch over tracks or observations: one new pose is taken into the list, every other count
    is zero (refine_poses counts the listed images), the points and the bytes are empty."""
    ids, kps, poses, lst = ring_job([3] * 5)
    assert open_ring(tctx, ids, kps, lst, 5)["tracks_kept"] == 5
    st = tctx.tracks_finish(min_length=4)
    assert st["tracks_kept"] == st["observations_kept"] == 0

    def counts(st, **nonzero):
        got = {k: v for k, v in st.items() if isinstance(v, int)}
        assert len(got) >= 5 and got == dict({k: 0 for k in got}, **nonzero), st

    tctx.triangulate_tracks(CAM, some(poses, ids, (0, 1)), *THR, robust=robust_session, max_hypotheses=8)
    counts(tctx.extend_points(some(poses, ids, (2,))), images_added=1)
    counts(tctx.filter_points())
    counts(tctx.complete_points())
    counts(tctx.refine_points())
    counts(tctx.refine_poses(), images=3)
    pts, res = tctx.points3d()
    assert len(pts) == 0 and len(res) == 0 and len(tctx.point_inliers()) == 0
    pid, tab = tctx.pose_list()
    assert pid.tolist() == [int(i) for i in ids] and np.all(tab["valid"] == 1)
    tctx.tracks_end()


def test_two_increments_order_and_replacement(tctx, host):
    """two increments against the twin's two; the second list permuted (nothing but the pose list's order depends on it); a
    valid == 0 entry of the triangulation's list replaced in place"""
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    first = some(poses, ids, efx.FIRST)
    first[int(ids[6])] = None                                                   # listed, not valid
    results = []
    for order in (None, [3, 1, 4, 0, 2]):
        tctx.triangulate_tracks(CAM, first, *THR, robust=True, max_hypotheses=16)
        extend_same(tctx, host, ids, kps, tracks, some(poses, ids, efx.TWO[0]), None)      # None: the session's route (16)
        new = _lib.pose_table(some(poses, ids, efx.TWO[1]))
        if order:
            new = (new[0][order].copy(), new[1][order].copy())
        st, pts, res, mask, tr, before = extend_same(tctx, host, ids, kps, tracks, new, 16)
        pid, tab = tctx.pose_list()
        want = [int(ids[p]) for p in (1, 2, 3, 6, 4, 5)] + [int(i) for i in new[0] if int(i) != int(ids[6])]
        assert pid.tolist() == want and np.all(tab["valid"] == 1) and st["images_added"] == 5
        results.append((pts, res, mask, {k: v for k, v in st.items() if not k.endswith("_ms")}))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(results[0][:3], results[1][:3])) and results[0][3] == results[1][3]
    assert _lib.succeeded(results[0][0]).sum() >= 90
    tctx.tracks_end()


# ---- the calls that follow ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust_session", (False, True))
def test_following_calls_see_the_extended_state(tctx, host, robust_session):
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    kd = {int(i): k for i, k in zip(ids, kps)}
    bad = pfx.perturbed(poses, 5, rot=2e-4, trans=1e-3, keep=(int(ids[1]),))
    tctx.triangulate_tracks(CAM, some(bad, ids, efx.FIRST), *THR, robust=robust_session, max_hypotheses=16)
    tctx.refine_poses(min_observations=6)
    tctx.pose_refinements()
    tctx.register_images(CAM, [int(ids[4])], min_inliers=6)
    tctx.registrations()
    extend_same(tctx, host, ids, kps, tracks, some(bad, ids, efx.TWO[0]), 16 if robust_session else 0)
    assert code(tctx.registrations) == _lib.E_STATE and code(tctx.pose_refinements) == _lib.E_STATE
    p0, r0, m0, lst0 = state(tctx)
    st = tctx.refine_points()
    wp, wr, wc = rtw.run(host, tracks, ids, kps, lst0, CAM, p0, r0, m0, THR[:2])
    pts, res = tctx.points3d()
    assert pts.tobytes() == wp.tobytes() and res.tobytes() == wr.tobytes() and st["refined"] == wc["refined"] > 0
    st = tctx.refine_poses(min_observations=6, fixed=[int(ids[1])])
    wp, wr, wl, wrec, wc = ptw.run(host, tracks, ids, kps, lst0, CAM, pts, res, m0, THR[:2], (10, 1e-6, 6), [int(ids[1])])
    pts, res = tctx.points3d()
    lst = tctx.pose_list()
    assert pts.tobytes() == wp.tobytes() and res.tobytes() == wr.tobytes() and lst[1].tobytes() == wl[1].tobytes()
    assert tctx.pose_refinements().tobytes() == wrec.tobytes() and st["refined"] == wc["refined"] > 0
    assert tctx.point_inliers().tobytes() == m0.tobytes()
    rest = [int(ids[p]) for p in efx.TWO[1]]
    tctx.register_images(CAM, rest, min_inliers=6)
    got = tctx.registrations()
    want = regtw.run(regtw.load_host(), tracks, pts, rest, kd, CAM, min_inliers=6)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and _lib.registered(got[0]).all()
    # a later triangulation and tracks_finish invalidate as documented
    tctx.triangulate_tracks(CAM, some(bad, ids, efx.FIRST), *THR)
    assert code(tctx.point_inliers) == _lib.E_STATE and len(tctx.pose_list()[0]) == 3
    tctx.extend_points({})
    assert len(tctx.point_inliers()) == len(tracks[1])
    tctx.tracks_finish()
    assert code(tctx.extend_points, {}) == _lib.E_STATE and code(tctx.point_inliers) == _lib.E_STATE
    tctx.tracks_end()


def test_errors_leave_the_session_alone(tctx, host):
    E = _lib
    ids, kps, poses, _, seen = efx.scene()
    assert code(tctx.extend_points, {}) == E.E_STATE                                          # no session
    d = np.random.default_rng(1).integers(0, 256, (efx.T, 128), dtype=np.uint8)
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), d)
        if k != 9:                                                                            # the last image never gets keypoints
            tctx.upload_keypoints(int(i), kps[k])
    tctx.tracks_begin(ids, add_only=True)
    tctx.tracks_add(*pfx.match_list(seen, ids))
    tctx.tracks_finish()
    assert code(tctx.extend_points, {}) == E.E_STATE                                          # finished, not triangulated
    first = some(poses, ids, efx.FIRST)
    first[int(ids[6])] = None
    tctx.triangulate_tracks(CAM, first, *THR, robust=True)
    tctx.register_images(CAM, [int(ids[4])], min_inliers=6)
    s0 = state(tctx)
    R, t = poses[int(ids[4])]
    nan_R, inf_t = np.array(R), np.array(t)
    nan_R[1, 1], inf_t[2] = np.nan, np.inf
    ok = {int(ids[4]): (R, t)}
    twice = (np.asarray([ids[4], ids[4]], np.int32), np.repeat(_lib.pose_table(ok)[1], 2))
    for new, kw, want in (({77: (R, t)}, {}, E.E_INVALID),                                     # not declared
                          ({20000: (R, t)}, {}, E.E_INVALID), ({-1: (R, t)}, {}, E.E_INVALID),
                          (twice, {}, E.E_INVALID),                                            # given twice
                          ({int(ids[1]): (R, t)}, {}, E.E_INVALID),                            # already posed
                          ({int(ids[4]): (nan_R, t)}, {}, E.E_INVALID), ({int(ids[4]): (R, inf_t)}, {}, E.E_INVALID),
                          (ok, dict(max_hypotheses=-1), E.E_INVALID), (ok, dict(max_hypotheses=1025), E.E_INVALID)):
        assert code(tctx.extend_points, new, **kw) == want, (new, kw)
        assert same_state(s0, state(tctx))
        tctx.registrations()                                                                  # still valid: nothing was touched
    assert tctx._L.msfm_extend_points(tctx._h, None, None, 1, None, None) == E.E_INVALID      # a NULL list with n_poses > 0
    assert tctx._L.msfm_extend_points(tctx._h, None, None, -1, None, None) == E.E_INVALID
    # a newly posed image with fewer keypoints than rows: listed behind a good one, nothing of which may have been taken
    both = dict(ok)
    both[int(ids[9])] = poses[int(ids[9])]
    assert code(tctx.extend_points, both) == E.E_NOIMAGE and same_state(s0, state(tctx))
    tctx.registrations()
    assert tctx.extend_points({int(ids[9]): None})["images_added"] == 0                      # valid == 0: accepted, nothing asked of it
    assert tctx._L.msfm_extend_points(tctx._h, None, None, 0, None, None) == E.OK             # NULL params and stats, an empty list
    assert code(tctx.registrations) == E.E_STATE                                              # a successful call invalidates them
    extend_same(tctx, host, ids, kps, tctx.tracks(), {int(ids[6]): poses[int(ids[6])], int(ids[4]): None}, 4)
    assert tctx.pose_list()[0].tolist() == [int(ids[p]) for p in (1, 2, 3, 6)] and np.all(tctx.pose_list()[1]["valid"] == 1)
    tctx.tracks_end()
    assert code(tctx.extend_points, {}) == E.E_STATE


# ---- the increment ----------------------------------------------------------------------------------------------------------------------
def test_grow_until_no_image_registers(tctx, host):
    """A ring scene with 0.3 px of noise, three images posed, grown until no image registers: every image ends registered; every
    increment's device state equals the twins run in the same order (registration, extension, point refinement, pose refinement);
    points that were REFINED before an increment and only continued by it keep their X bytes; the final RMS over the fitting
    observations is at or below twice the noise's own RMS, the bound tests/test_refine_poses_reference.py::
    test_alternation_recovers_perturbed_poses uses for this noise level."""
    n_img, T = 9, 120
    ids, kps, poses, seen = pfx.chosen_scene(pfx.general_points(T, 53), [T] * n_img, noise_px=0.3, seed=3)
    # an image sees the tracks of a window that moves along the ring: later images share few tracks with the first three
    for i in range(n_img):
        seen[:, i] = False
        seen[max(0, 12 * i - 30):12 * i + 54, i] = True
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), T)
    tracks = tctx.tracks()
    assert len(tracks[0]) - 1 == T
    kd = {int(i): k for i, k in zip(ids, kps)}
    reg_host = regtw.load_host()
    tctx.triangulate_tracks(CAM, some(poses, ids, (0, 1, 2)), *THR)
    tctx.refine_points()
    fixed = [int(ids[0])]
    rounds, done = 0, []
    while True:
        p0, r0, m0, lst0 = state(tctx)
        todo = [int(i) for i in ids if int(i) not in tctx.poses()]
        reg, ext, alt, new_ids = tctx.grow(CAM, register_params=dict(min_inliers=15), rounds=2, fixed=fixed, pose_params=dict(min_observations=15))
        if not new_ids:
            assert ext is None and alt == [] and same_state((p0, r0, m0, lst0), state(tctx))  # nothing changed
            break
        rounds += 1
        done += new_ids
        # the twins in the same order
        rec = regtw.run(reg_host, tracks, p0, todo, kd, CAM, min_inliers=15)[0]
        new = _lib.registered_poses(rec)
        assert sorted(new) == new_ids
        wp, wr, wm, wc, wl, tr = etw.run(host, tracks, ids, kps, lst0, new, CAM, p0, r0, m0, THR, 0, trace=True)
        assert {k: ext[k] for k in etw.COUNT_KEYS} == {k: wc[k] for k in etw.COUNT_KEYS}
        only = (tr["kind"] == etw.KIND_CONTINUE) & _lib.refined(p0)
        assert only.any() and wp["X"][only].tobytes() == p0["X"][only].tobytes() and np.all(_lib.refined(wp)[only])
        cost = obs = 0
        for a, b in alt:
            wp, wr, c1 = rtw.run(host, tracks, ids, kps, wl, CAM, wp, wr, wm, THR[:2])
            wp, wr, wl, _, c2 = ptw.run(host, tracks, ids, kps, wl, CAM, wp, wr, wm, THR[:2], (10, 1e-6, 15), fixed)
            assert a["refined"] == c1["refined"] and b["refined"] == c2["refined"]
            cost, obs = c2["cost_after"], c2["observations"]
        pts, res, mask, lst = state(tctx)
        assert pts.tobytes() == wp.tobytes() and res.tobytes() == wr.tobytes() and mask.tobytes() == wm.tobytes()
        assert lst[0].tobytes() == wl[0].tobytes() and lst[1].tobytes() == wl[1].tobytes()
    assert sorted(done + [int(ids[p]) for p in (0, 1, 2)]) == [int(i) for i in ids] and rounds >= 2
    rms = float(np.sqrt(cost / obs))
    print("grow: %d increments, final RMS %.3f px over %d observations" % (rounds, rms, obs))
    assert rms <= 2 * 0.3 * np.sqrt(2.0)
    tctx.tracks_end()
