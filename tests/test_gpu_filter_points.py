"""Map filtering on the device (msfm_filter_points, csrc/msfm_filter.hip.h) against the host twin (csrc/msfm_filter.h, FilterPoints,
through tests/filter_twin.py): records, residuals, inlier bytes, the pose list and all nine counters BYTE FOR BYTE.  The twin is fed the
device's own state before the call (records, residuals, bytes where the session has them, the pose list), which the earlier GPU tests
hold equal to their twins.  Where a test is about a route, the twin's trace is asserted next to the byte comparison.  Every call is
repeated once: the second call changes not one byte.  The twin itself is checked against the independent numpy reference in
tests/test_filter_points_reference.py."""
import time

import numpy as np
import pytest

import extend_fixtures as efx
import extend_twin as etw
import filter_twin as ftw
import refine_points_twin as rtw
import refine_poses_fixtures as pfx
import refine_poses_twin as ptw
import registration_twin as regtw
from monocularsfm_amd import _lib
from test_gpu_extend_points import code, extend_same, full_equals_created, same_state, some, state
from test_gpu_robust_triangulation import open_ring, ring_job, second_pass_job

pytestmark = pytest.mark.gpu
CAM = efx.CAM
THR = efx.THRESHOLDS
LOOSE = (40.0, 1.0, 2)
TIGHT = (2.0, 1.5)
KEEP = _lib.TRI_ROBUST | _lib.TRI_REFINED | _lib.TRI_REPOSED | _lib.TRI_EXTENDED
QUIET = [k for k in ftw.ALL_KEYS if k not in ("eligible", "succeeded", "observations_used")]


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return ftw.load_host()


def filter_same(ctx, host, ids, kps, tracks, thr, params=None, scope=None, cam=CAM, again=True):
    """one msfm_filter_points on the session's current state against the twin run from that state, and a second, idempotent call
    -> (stats, points, residuals, bytes, the twin's trace, the state before)"""
    p0, r0, m0, lst0 = before = state(ctx)
    kw = {} if params is None else dict(max_error=params[0], min_angle=params[1])
    st = ctx.filter_points(image_ids=scope, **kw)
    pts, res, mask, lst = state(ctx)
    wp, wr, wm, wc, tr = ftw.run(host, tracks, ids, kps, lst0, cam, p0, r0, m0, thr, params, scope or (), trace=True)
    assert pts.tobytes() == wp.tobytes(), np.nonzero(pts != wp)[0][:8]
    assert res.tobytes() == wr.tobytes(), np.nonzero(res != wr)[0][:8]
    assert mask is not None and mask.tobytes() == wm.tobytes(), np.nonzero(mask != wm)[0][:8]
    assert lst[0].tobytes() == lst0[0].tobytes() and lst[1].tobytes() == lst0[1].tobytes()
    assert {k: st[k] for k in ftw.ALL_KEYS} == {k: wc[k] for k in ftw.ALL_KEYS}, (st, wc)
    assert st["filter_ms"] >= st["prepare_ms"] >= 0.0
    # untouched and ineligible tracks bit for bit, trimmed ones keep X and the four history bits, removed ones have the stated shape
    o = tracks[0]
    per_obs = np.repeat(tr["kind"], np.diff(o))
    same = tr["kind"] <= ftw.KIND_UNTOUCHED
    assert pts[same].tobytes() == p0[same].tobytes() and res[per_obs <= 1].tobytes() == r0[per_obs <= 1].tobytes()
    if m0 is not None:
        assert mask[per_obs <= 1].tobytes() == m0[per_obs <= 1].tobytes()
    trim, gone = tr["kind"] == ftw.KIND_TRIMMED, tr["kind"] >= ftw.KIND_REMOVED_BY_VIEWS
    assert pts["X"][trim].tobytes() == p0["X"][trim].tobytes() and np.array_equal(pts["status"][trim] & KEEP, p0["status"][trim] & KEEP)
    assert np.all(_lib.filtered(pts)[trim | gone]) and np.all(pts["status"][gone] == (_lib.TRI_ATTEMPTED | _lib.TRI_FILTERED))
    assert not pts["n_views"][gone].any() and np.all(res[per_obs >= 3] == -1.0) and not mask[per_obs >= 3].any()
    if params is None:
        assert np.all((pts["status"][trim] & 28) == 28)
    if again:
        st2 = ctx.filter_points(image_ids=scope, **kw)
        assert same_state((pts, res, mask, lst), state(ctx)) and all(st2[k] == 0 for k in QUIET), st2
        assert st2["succeeded"] == st["succeeded"] and st2["observations_used"] == st["observations_used"]
    return st, pts, res, mask, tr, before


# ---- track counts: the wave and block edges of flt_track_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("robust_session", (False, True))
def test_track_counts_at_the_wave_and_block_edges(tctx, host, robust_session):
    """T = 1, 63, 64, 65, 255, 256, 257 kept tracks under a loose (40 px, 1 degree) session; the tracks at the lanes 0, 63 | 64, 255 | 256
    have length 5, every other track has length 3 and stays untouched.  Lanes 0, 64 and 256 carry one observation moved by 5 px across
    the epipolar lines (its error ~4 px, the others' ~1 px): trimmed at (2 px, 1.5 degrees).  Lanes 63 and 255 carry two moved by 30 px
    the same way (the point follows them: no error stays below 2 px): removed by views -- unless the robust call retried the track,
    whose point is then a clean two-view hypothesis' and only the two are dropped.  On the plain session the bytes are created by the
    call; on the robust one they stand."""
    for T in (257, 256, 255, 65, 64, 63, 1):
        lengths = [5 if j in (0, 63, 64, 255, 256) else 3 for j in range(T)]
        moved = {j: [(2, 0.0, 5.0)] for j in (0, 64, 256) if j < T}
        moved.update({j: [(1, 0.0, 30.0), (3, 0.0, 30.0)] for j in (63, 255) if j < T})
        ids, kps, poses, lst = ring_job(lengths, moved=moved, noise_px=0.1)
        assert open_ring(tctx, ids, kps, lst, T)["tracks_kept"] == T
        tracks = tctx.tracks()
        tctx.triangulate_tracks(CAM, poses, *LOOSE, robust=robust_session, max_hypotheses=8)
        assert (code(tctx.point_inliers) == _lib.E_STATE) if not robust_session else tctx.point_inliers().all()
        st, pts, res, mask, tr, before = filter_same(tctx, host, ids, kps, tracks, LOOSE, TIGHT)
        touched = [j for j in (0, 63, 64, 255, 256) if j < T]
        assert np.array_equal(np.nonzero(tr["kind"] > ftw.KIND_UNTOUCHED)[0], touched) and st["eligible"] == T
        for j in touched:
            # (where the robust call retried a lane 63 | 255 its point is a two-view hypothesis': the two moved observations are dropped
            # and the other three stand)
            rescued = bool(before[0]["status"][j] & _lib.TRI_ROBUST)
            want = ftw.KIND_TRIMMED if j in (0, 64, 256) or rescued else ftw.KIND_REMOVED_BY_VIEWS
            assert tr[j]["kind"] == want and not (rescued and not robust_session), (T, j, tr[j])
            # (a point that follows two moved observations may end behind the cameras: dropped by depth then)
            assert tr[j]["dropped_by_depth"] + tr[j]["dropped_by_error"] == (1 if j in (0, 64, 256) else 2 if rescued else 5)
        assert st["trimmed"] + st["removed_by_views"] == len(touched) and st["removed_by_angle"] == 0
        assert all(pts[j]["n_views"] == 4 and mask[tracks[0][j] + 2] == 0 for j in touched if j in (0, 64, 256))
        tctx.tracks_end()


def test_second_grid_stride_pass(tctx, host):
    """flt_track_kernel's grid holds 8 x CUs x 256 lanes: with 8192 tracks more its first 32 workgroups run a second pass of the
    wave-uniform t0 loop; ext_mask_kernel and ref_obs_kernel run their second pass too.  Under a loose session every third track and
    every track of the last 8192 stands on an observation moved by 40 px: at (2 px, 1.5 degrees) the second pass drops and removes."""
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
    thr = (60.0, 1.0, 2)
    tctx.triangulate_tracks(CAM, poses, *thr)
    st, pts, _, _, tr, _ = filter_same(tctx, host, ids, kps, tracks, thr, TIGHT, again=False)
    tail = tr[T - 8192:]
    assert st["eligible"] == T and np.all(tail["kind"] > ftw.KIND_UNTOUCHED) and np.all(tail["dropped_by_depth"] + tail["dropped_by_error"] > 0)
    assert st["removed_by_views"] + st["removed_by_angle"] + st["trimmed"] >= T // 3 and (tr["kind"] == ftw.KIND_UNTOUCHED).sum() > T // 2
    print("second pass: T %d, filter_ms %.3f of which prepare %.3f, trimmed %d, removed %d + %d, wall %.1f s" %
          (T, st["filter_ms"], st["prepare_ms"], st["trimmed"], st["removed_by_views"], st["removed_by_angle"], time.time() - t0))
    tctx.tracks_end()


# ---- where the dropped observation sits in its track ------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_dropped_observation_first_middle_last(tctx, host, where):
    """Tracks of 2, 3, 64, 65 and 129 elements, two of each: the first five carry one observation moved across the epipolar lines at
    their first, middle or last element (30 px; 4.5 px on the 3-view track, whose other errors stay below 2 px), the second five are
    clean.  Under a loose session at (2 px, 1.5 degrees): the long tracks are trimmed by exactly that element; the moved 2-view track
    is removed by views, the clean one by angle (1.2 degrees); the moved 3-view track loses its first or last view -- the other two are
    1.2 degrees apart: removed by angle after a drop -- or its middle one (2.4 degrees: trimmed)."""
    lengths = [2, 3, 64, 65, 129, 2, 3, 64, 65, 129]
    at = {t: {"first": 0, "middle": lengths[t] // 2, "last": lengths[t] - 1}[where] for t in range(5)}
    moved = {t: [(at[t], 0.0, 4.5 if lengths[t] == 3 else 30.0)] for t in range(5)}
    ids, kps, poses, lst = ring_job(lengths, moved=moved, noise_px=0.1)
    open_ring(tctx, ids, kps, lst, len(lengths))
    tracks = tctx.tracks()
    o = tracks[0]
    tctx.triangulate_tracks(CAM, poses, *LOOSE)
    st, pts, res, mask, tr, _ = filter_same(tctx, host, ids, kps, tracks, LOOSE, TIGHT)
    for t in (2, 3, 4):
        assert tr[t]["kind"] == ftw.KIND_TRIMMED and tr[t]["dropped_by_error"] == 1 and pts[t]["n_views"] == lengths[t] - 1
        assert mask[o[t] + at[t]] == 0 and mask[o[t]:o[t + 1]].sum() == lengths[t] - 1 and res[o[t] + at[t]] > 2.0
    assert tr[0]["kind"] == ftw.KIND_REMOVED_BY_VIEWS and tr[5]["kind"] == ftw.KIND_REMOVED_BY_ANGLE and tr[5]["dropped_by_error"] == 0
    assert tr[1]["dropped_by_error"] == 1 and tr[1]["kind"] == (ftw.KIND_TRIMMED if where == "middle" else ftw.KIND_REMOVED_BY_ANGLE)
    assert np.all(tr["kind"][6:] == ftw.KIND_UNTOUCHED)
    tctx.tracks_end()


def test_dropped_next_to_an_unposed_and_a_rejected_element(tctx, host):
    """USED != FIT != all: eight-view tracks on a robust (2 px) session in which image 3 has no pose and the observation in image 4
    of track 0 is 30 px off -- the triangulation's hypotheses reject it (byte 0, still USED).  Its observation in image 2 is 1.5 px off:
    a fitting observation that a call at (0.8 px, 1.5 degrees) drops, next to the unposed and the rejected element."""
    lengths = [8] * 4
    ids, kps, poses, lst = ring_job(lengths, moved={0: [(4, 0.0, 30.0), (2, 0.0, 1.5)]}, noise_px=0.05)
    open_ring(tctx, ids, kps, lst, 4)
    tracks = tctx.tracks()
    o = tracks[0]
    tctx.triangulate_tracks(CAM, some(poses, ids, (0, 1, 2, 4, 5, 6, 7)), *THR, robust=True, max_hypotheses=16)
    m0 = tctx.point_inliers()
    assert m0[o[0] + 4] == 0 and m0[o[0] + 3] == 0 and m0[o[0] + 2] == 1 and m0[o[0]:o[1]].sum() == 6
    st, pts, res, mask, tr, before = filter_same(tctx, host, ids, kps, tracks, THR, (0.8, 1.5))
    assert tr[0]["kind"] == ftw.KIND_TRIMMED and (tr[0]["dropped_by_error"], tr[0]["kept"]) == (1, 5) and mask[o[0] + 2] == 0
    assert res[o[0] + 3] == -1.0 and res[o[0] + 4] > 2.0 and res[o[0] + 2] > 0.8            # unposed: no slot; USED: an error
    assert (pts["status"][0] & _lib.TRI_ROBUST) and np.all(tr["kind"][1:] == ftw.KIND_UNTOUCHED)
    tctx.tracks_end()


# ---- every route of the rule ------------------------------------------------------------------------------------------------------------
def test_every_route(tctx, host):
    """A (4 px, 1 degree) plain session over six images of which image 5's camera is turned round (the scene lies behind it and projects
    onto its keypoints: small errors, negative depth).  Tracks 0 .. 3, 6, 7 have six views, 4 has two, 5 has three.
      call 1, LOOSER than the session (40 px, 0.5 degrees): image 5 is dropped by depth from every six-view track, nothing else: trimmed.
      then image 3's keypoint of track 2 becomes a NaN (the keypoints of an image may be replaced during a session).
      call 2, TIGHTER (2 px, 1.5 degrees): track 1 (8 px off in image 2: no ERROR_OK under the session) is trimmed and REGAINS; track 2
      drops its NaN; track 3 (two observations 30 px off) is removed by views; track 4 (1.2 degrees) is removed by angle without a
      drop; track 5 (4.5 px off in image 2) by angle after one; 6 and 7 are untouched by the second call."""
    lengths = [6, 6, 6, 6, 2, 3, 6, 6]
    moved = {1: [(2, 0.0, 8.0)], 3: [(1, 0.0, 30.0), (3, 0.0, 30.0)], 5: [(2, 0.0, 4.5)]}
    ids, kps, poses, lst = ring_job(lengths, moved=moved, noise_px=0.1, turned=(5,))
    open_ring(tctx, ids, kps, lst, len(lengths))
    tracks = tctx.tracks()
    o = tracks[0]
    thr = (4.0, 1.0, 2)
    tctx.triangulate_tracks(CAM, poses, *thr)
    p0 = tctx.points3d()[0]
    six = np.asarray(lengths) == 6
    assert not (p0["status"][six] & _lib.TRI_DEPTH_OK).any() and not (p0["status"][1] & _lib.TRI_ERROR_OK) and _lib.succeeded(p0)[[0, 2, 6, 7]].all()
    st, pts, res, mask, tr, _ = filter_same(tctx, host, ids, kps, tracks, thr, (40.0, 0.5))
    assert st["dropped_by_depth"] == 6 and st["dropped_by_error"] == 0 and st["trimmed"] == 6 and st["removed_by_views"] == st["removed_by_angle"] == 0
    assert np.all(pts["status"][six] & _lib.TRI_DEPTH_OK) and np.all(pts["n_views"][six] == 5) and not mask[o[:-1][six] + 5].any()
    bad = np.array(kps[3])
    bad[2, 0] = np.nan
    tctx.upload_keypoints(int(ids[3]), bad)
    kps = list(kps)
    kps[3] = bad
    st, pts, res, mask, tr, before = filter_same(tctx, host, ids, kps, tracks, thr, TIGHT)
    K = ftw
    assert tr["kind"].tolist() == [K.KIND_UNTOUCHED, K.KIND_TRIMMED, K.KIND_TRIMMED, K.KIND_REMOVED_BY_VIEWS, K.KIND_REMOVED_BY_ANGLE,
                                   K.KIND_REMOVED_BY_ANGLE, K.KIND_UNTOUCHED, K.KIND_UNTOUCHED], tr
    assert st["regained"] == 1 and not _lib.succeeded(before[0])[1] and _lib.succeeded(pts)[1] and mask[o[1] + 2] == 0
    assert np.isnan(res[o[2] + 3]) and mask[o[2] + 3] == 0 and pts[2]["n_views"] == 4 and tr[2]["dropped_by_error"] == 1
    assert tr[4]["dropped_by_error"] == 0 and tr[5]["dropped_by_error"] == 1 and st["dropped_by_depth"] == 0
    tctx.tracks_end()


def test_both_kinds_of_drop_in_one_track(tctx, host):
    """one call drops image 5 (turned round) by depth and an observation 8 px off by error from the same track"""
    ids, kps, poses, lst = ring_job([6] * 3, moved={1: [(2, 0.0, 8.0)]}, noise_px=0.1, turned=(5,))
    open_ring(tctx, ids, kps, lst, 3)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, poses, *LOOSE)
    st, pts, res, mask, tr, _ = filter_same(tctx, host, ids, kps, tracks, LOOSE, TIGHT)
    assert (tr[1]["dropped_by_depth"], tr[1]["dropped_by_error"], tr[1]["kept"]) == (1, 1, 4) and tr[1]["kind"] == ftw.KIND_TRIMMED
    assert st["dropped_by_depth"] == 3 and st["trimmed"] == 3
    tctx.tracks_end()


def test_regained_after_a_pose_refinement_that_lost_points(tctx, host):
    """refine_poses_fixtures' route "lost_and_gained": the pose refinement's re-verdict takes ERROR_OK from points; with NULL
    parameters the filter drops what crossed the session's max_error, the trimmed records regain it and keep REPOSED"""
    ids, kps, start, seen, fixed, thr, _ = pfx.route_case("lost_and_gained")
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), pfx.ROUTE_T)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(pfx.CAM, start, *thr)
    ok0 = _lib.succeeded(tctx.points3d()[0])
    rp = tctx.refine_poses(pfx.ROUTE_PARAMS[0], pfx.ROUTE_PARAMS[1], pfx.ROUTE_PARAMS[2], fixed=fixed)
    assert rp["points_lost"] > 0
    lost = ok0 & ~_lib.succeeded(tctx.points3d()[0])
    st, pts, res, mask, tr, before = filter_same(tctx, host, ids, kps, tracks, thr + (2,), None, cam=pfx.CAM)
    trim = tr["kind"] == ftw.KIND_TRIMMED
    assert st["regained"] > 0 and np.all(_lib.succeeded(pts)[trim]) and np.all(_lib.reposed(pts)[trim & _lib.reposed(before[0])])
    assert np.all((tr["kind"][lost] == ftw.KIND_TRIMMED) | (tr["kind"][lost] >= ftw.KIND_REMOVED_BY_VIEWS))
    tctx.tracks_end()


def test_history_bits_are_kept_on_a_trimmed_record(tctx, host):
    """test_gpu_extend_points' continue job: track 4 is retried at the robust triangulation (ROBUST), the session goes through
    refine_points (REFINED) and refine_poses (REPOSED), the images 0 and 4 arrive (EXTENDED).  The session admits 4 px; the track's
    observation in image 3 is 3.6 px off (its error at the point ~2.4 px, the others' ~1.2 px): a call at (1.8 px, 1.5 degrees) trims it,
    and the record keeps all four bits next to FILTERED."""
    thr = (4.0, 1.5, 2)
    ids, kps, poses, lst = ring_job([6] * 6, moved={4: [(2, 0.0, 30.0), (3, 0.0, 3.6)]}, noise_px=0.1)
    open_ring(tctx, ids, kps, lst, 6)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, ids, (1, 2, 3, 5)), *thr, robust=True, max_hypotheses=8)
    tctx.refine_points()
    tctx.refine_poses(min_observations=3, fixed=[int(ids[1]), int(ids[3])])       # (six observations: a free image 3 would absorb the offset)
    extend_same(tctx, host, ids, kps, tracks, some(poses, ids, (0, 4)), 0, thr=thr)
    p0 = tctx.points3d()[0]
    assert (p0["status"][4] & KEEP) == KEEP, p0["status"]
    st, pts, res, mask, tr, _ = filter_same(tctx, host, ids, kps, tracks, thr, (1.8, 1.5))
    assert tr[4]["kind"] == ftw.KIND_TRIMMED and (pts["status"][4] & (KEEP | _lib.TRI_FILTERED)) == (KEEP | _lib.TRI_FILTERED)
    assert mask[tracks[0][4] + 3] == 0 and mask[tracks[0][4] + 2] == 0 and pts[4]["n_views"] == 4
    tctx.tracks_end()


# ---- scope ------------------------------------------------------------------------------------------------------------------------------
def test_scope(tctx, host):
    """the extension's scene on a robust session, extended by the first of two increments: a listed image; a listed image without a
    pose, which selects nothing; an empty list against None; a permuted list gives the same bytes"""
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    prm = (1.0, 2.5)

    def fresh():
        tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR, robust=True, max_hypotheses=64)
        tctx.extend_points(some(poses, ids, efx.TWO[0]))

    fresh()
    s0 = state(tctx)
    unposed = [int(ids[p]) for p in efx.TWO[1][:2]]
    st, *_ = filter_same(tctx, host, ids, kps, tracks, THR, prm, unposed)
    assert st["eligible"] == 0 and same_state(s0, state(tctx))
    listed = [int(ids[p]) for p in efx.TWO[0]]
    st, pts, res, mask, tr, _ = filter_same(tctx, host, ids, kps, tracks, THR, prm, listed)
    assert 0 < st["eligible"] < efx.T and st["trimmed"] > 0 and (tr["kind"] == ftw.KIND_NOT_ELIGIBLE).any()
    fresh()
    st2 = tctx.filter_points(*prm, image_ids=listed[::-1] + [])
    assert same_state((pts, res, mask, s0[3]), state(tctx)) and {k: st2[k] for k in ftw.ALL_KEYS} == {k: st[k] for k in ftw.ALL_KEYS}
    fresh()
    st_all, p_all, r_all, m_all, _, _ = filter_same(tctx, host, ids, kps, tracks, THR, prm, None)
    assert st_all["eligible"] > st["eligible"]
    fresh()
    st_empty = tctx.filter_points(*prm, image_ids=[])
    assert same_state((p_all, r_all, m_all, s0[3]), state(tctx)) and {k: st_empty[k] for k in ftw.ALL_KEYS} == {k: st_all[k] for k in ftw.ALL_KEYS}
    tctx.tracks_end()


# ---- the calls that follow ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust_session", (False, True))
def test_following_calls_see_the_filtered_state(tctx, host, robust_session):
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    lst = pfx.match_list(seen, ids)
    kd = {int(i): k for i, k in zip(ids, kps)}
    mh = 16 if robust_session else 0
    bad = pfx.perturbed(poses, 5, rot=2e-4, trans=1e-3, keep=(int(ids[1]),))
    tctx.triangulate_tracks(CAM, some(bad, ids, efx.FIRST + efx.TWO[0]), *THR, robust=robust_session, max_hypotheses=16)
    tctx.refine_poses(min_observations=6)
    tctx.pose_refinements()
    tctx.register_images(CAM, [int(ids[6])], min_inliers=6)
    tctx.registrations()
    st, pts, res, mask, tr, _ = filter_same(tctx, host, ids, kps, tracks, THR, (0.6, 4.0))
    gone = tr["kind"] >= ftw.KIND_REMOVED_BY_VIEWS
    assert st["trimmed"] > 0 and gone.any()
    assert code(tctx.registrations) == _lib.E_STATE and code(tctx.pose_refinements) == _lib.E_STATE
    p0, r0, m0, lst0 = state(tctx)
    st = tctx.refine_points()
    wp, wr, wc = rtw.run(host, tracks, ids, kps, lst0, CAM, p0, r0, m0, THR[:2])
    pts, res = tctx.points3d()
    assert pts.tobytes() == wp.tobytes() and res.tobytes() == wr.tobytes() and st["refined"] == wc["refined"] > 0 and st["eligible"] == wc["eligible"]
    assert pts[gone].tobytes() == p0[gone].tobytes()                                          # removed records are skipped
    st = tctx.refine_poses(min_observations=6, fixed=[int(ids[1])])
    wp, wr, wl, wrec, wc = ptw.run(host, tracks, ids, kps, lst0, CAM, pts, res, m0, THR[:2], (10, 1e-6, 6), [int(ids[1])])
    pts, res = tctx.points3d()
    lst1 = tctx.pose_list()
    assert pts.tobytes() == wp.tobytes() and res.tobytes() == wr.tobytes() and lst1[1].tobytes() == wl[1].tobytes()
    assert tctx.pose_refinements().tobytes() == wrec.tobytes() and st["refined"] == wc["refined"]
    assert tctx.point_inliers().tobytes() == m0.tobytes()
    rest = [int(ids[p]) for p in efx.TWO[1]]
    tctx.register_images(CAM, rest, min_inliers=6)
    got = tctx.registrations()
    want = regtw.run(regtw.load_host(), tracks, pts, rest, kd, CAM, min_inliers=6)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    # the extension creates a removed track that sees a new image afresh: the full triangulation's record
    st, pts, res, mask, etr, _ = extend_same(tctx, host, ids, kps, tracks, some(bad, ids, efx.TWO[1]), mh)
    again = gone & (etr["kind"] == etw.KIND_CREATE)
    assert again.any() and not (gone & (etr["kind"] == etw.KIND_CONTINUE)).any()
    full_equals_created(host, ids, kps, tctx.pose_list(), efx.T, lst, pts, res, mask, etr, mh)
    # a later triangulation and tracks_finish invalidate as before
    tctx.triangulate_tracks(CAM, some(bad, ids, efx.FIRST), *THR)
    assert code(tctx.point_inliers) == _lib.E_STATE and len(tctx.pose_list()[0]) == 3
    tctx.filter_points()
    assert len(tctx.point_inliers()) == len(tracks[1])
    tctx.tracks_finish()
    assert code(tctx.filter_points) == _lib.E_STATE and code(tctx.point_inliers) == _lib.E_STATE
    tctx.tracks_end()


def test_errors_leave_the_session_alone(tctx, host):
    E = _lib
    ids, kps, poses, _, seen = efx.scene()
    assert code(tctx.filter_points) == E.E_STATE                                              # no session
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    assert code(tctx.filter_points) == E.E_STATE                                              # finished, not triangulated
    first = some(poses, ids, efx.FIRST)
    tctx.triangulate_tracks(CAM, first, *THR, robust=True)
    tctx.refine_poses(min_observations=6)
    tctx.register_images(CAM, [int(ids[4])], min_inliers=6)
    s0 = state(tctx)
    good = int(ids[1])
    for kw in (dict(max_error=np.nan, min_angle=1.5), dict(max_error=2.0, min_angle=np.inf), dict(max_error=-1.0, min_angle=1.5),
               dict(max_error=2.0, min_angle=-0.5), dict(image_ids=[good, 77]), dict(image_ids=[good, 20000]), dict(image_ids=[good, -1]),
               dict(image_ids=[good, int(ids[2]), good])):                                    # the bad id BEHIND a good one
        assert code(tctx.filter_points, **kw) == E.E_INVALID, kw
        assert same_state(s0, state(tctx))
        tctx.registrations()                                                                  # still valid: nothing was touched
        tctx.pose_refinements()
    assert tctx._L.msfm_filter_points(tctx._h, None, None, 1, None) == E.E_INVALID            # a NULL list with n_images > 0
    assert tctx._L.msfm_filter_points(tctx._h, None, None, -1, None) == E.E_INVALID
    assert same_state(s0, state(tctx))
    tctx.registrations()
    assert tctx._L.msfm_filter_points(tctx._h, None, None, 0, None) == E.OK                   # NULL params and stats, no list
    assert code(tctx.registrations) == E.E_STATE and code(tctx.pose_refinements) == E.E_STATE  # a successful call invalidates them
    tctx.tracks_end()
    assert code(tctx.filter_points) == E.E_STATE


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def test_reconstruct_filters_after_every_increment(tctx, host):
    """test_gpu_extend_points' grow scene (nine ring images, 120 points, 0.3 px of noise) with five observations in LATER images
    moved by 30 px: the extension admits none of them (a standing point rejects a new observation by error), but the alternation that
    follows meets the tracks they sit in.  Every increment's device state equals the twins run in the same order (registration,
    extension, point refinement, pose refinement, filter); at the end no fitting observation of a standing point exceeds max_error,
    and the RMS over the fitting observations is at or below the bound of that test, 2 x 0.3 x sqrt(2) px."""
    n_img, T = 9, 120
    ids, kps, poses, seen = pfx.chosen_scene(pfx.general_points(T, 53), [T] * n_img, noise_px=0.3, seed=3)
    for i in range(n_img):
        seen[:, i] = False
        seen[max(0, 12 * i - 30):12 * i + 54, i] = True
    for t, i in ((40, 4), (55, 5), (70, 6), (85, 7), (100, 8)):
        assert seen[t, i]
        kps[i][t, 1] += np.float32(30.0)
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), T)
    tracks = tctx.tracks()
    o = tracks[0]
    kd = {int(i): k for i, k in zip(ids, kps)}
    reg_host = regtw.load_host()
    tctx.triangulate_tracks(CAM, some(poses, ids, (0, 1, 2)), *THR)
    tctx.refine_points()
    fixed = [int(ids[0])]
    kw = dict(register_params=dict(min_inliers=15), fixed=fixed, pose_params=dict(min_observations=15))
    done, wl = [], None
    while True:
        p0, r0, m0, lst0 = state(tctx)
        todo = [int(i) for i in ids if int(i) not in tctx.poses()]
        out = tctx.reconstruct(CAM, rounds=2, max_increments=1, **kw)
        if not out:
            assert not todo or same_state((p0, r0, m0, lst0), state(tctx))
            break
        inc = out[0]
        assert sorted(inc) == ["alternate", "extend", "filter", "register", "registered"]
        done += inc["registered"]
        rec = regtw.run(reg_host, tracks, p0, todo, kd, CAM, min_inliers=15)[0]
        new = _lib.registered_poses(rec)
        assert sorted(new) == inc["registered"]
        wp, wr, wm, wc, wl = etw.run(host, tracks, ids, kps, lst0, new, CAM, p0, r0, m0, THR, 0)
        assert {k: inc["extend"][k] for k in etw.COUNT_KEYS} == {k: wc[k] for k in etw.COUNT_KEYS}
        for a, b in inc["alternate"]:
            wp, wr, c1 = rtw.run(host, tracks, ids, kps, wl, CAM, wp, wr, wm, THR[:2])
            wp, wr, wl, _, c2 = ptw.run(host, tracks, ids, kps, wl, CAM, wp, wr, wm, THR[:2], (10, 1e-6, 15), fixed)
            assert a["refined"] == c1["refined"] and b["refined"] == c2["refined"]
        wp, wr, wm, c3 = ftw.run(host, tracks, ids, kps, wl, CAM, wp, wr, wm, THR[:2])
        assert {k: inc["filter"][k] for k in ftw.ALL_KEYS} == c3
        pts, res, mask, lst = state(tctx)
        assert pts.tobytes() == wp.tobytes() and res.tobytes() == wr.tobytes() and mask.tobytes() == wm.tobytes()
        assert lst[0].tobytes() == wl[0].tobytes() and lst[1].tobytes() == wl[1].tobytes()
    assert sorted(done + [int(ids[p]) for p in (0, 1, 2)]) == [int(i) for i in ids] and len(tctx.reconstruct(CAM, **kw)) == 0
    pts, res, mask, _ = state(tctx)
    fit = (mask != 0) & np.repeat(_lib.succeeded(pts), np.diff(o))
    assert fit.sum() > 400 and np.all(res[fit] <= THR[0])
    rms = float(np.sqrt(np.mean(res[fit] ** 2)))
    print("reconstruct: %d images registered, final RMS %.3f px over %d fitting observations, %d records filtered" %
          (len(done), rms, int(fit.sum()), int(_lib.filtered(pts).sum())))
    assert rms <= 2 * 0.3 * np.sqrt(2.0)
    tctx.tracks_end()
