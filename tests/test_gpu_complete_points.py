"""Map completion on the device (msfm_complete_points, csrc/msfm_complete.hip.h) against the host twin (csrc/msfm_complete.h,
CompletePoints, through tests/complete_twin.py): records, residuals, inlier bytes, the pose list and all eight counters BYTE FOR BYTE.
The twin is fed the device's own state before the call (records, residuals, bytes where the session has them, the pose list), which
the earlier GPU tests hold equal to their twins.  Where a test is about a route, the twin's trace is asserted next to the byte
comparison.  Every call is repeated once: the second call changes not one byte and admits nothing.  The twin itself is checked against
the independent numpy reference in tests/test_complete_points_reference.py.

Device states come through API calls alone.  A candidate that fits is PLANTED (plant()): its keypoint is moved by 40 px with
upload_keypoints, filter_points drops it, the original keypoint is uploaded again."""
import time

import numpy as np
import pytest

import complete_twin as ctw
import extend_fixtures as efx
import extend_twin as etw
import filter_twin as ftw
import refine_points_twin as rtw
import refine_poses_fixtures as pfx
import refine_poses_twin as ptw
import registration_twin as regtw
from monocularsfm_amd import _lib
from test_gpu_extend_points import code, extend_same, same_state, some, state
from test_gpu_filter_points import filter_same
from test_gpu_robust_triangulation import open_ring, ring_job, second_pass_job

pytestmark = pytest.mark.gpu
CAM = efx.CAM
THR = efx.THRESHOLDS
KEEP = _lib.TRI_ROBUST | _lib.TRI_REFINED | _lib.TRI_REPOSED | _lib.TRI_EXTENDED | _lib.TRI_FILTERED
STANDS = _lib.TRI_POINT | _lib.TRI_ERROR_OK | _lib.TRI_ANGLE_OK


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return ctw.load_host()


def complete_same(ctx, host, ids, kps, tracks, thr, max_error=None, scope=None, cam=CAM, again=True):
    """one msfm_complete_points on the session's current state against the twin run from that state, and a second call that changes
    nothing -> (stats, points, residuals, bytes, the twin's trace, the state before)"""
    p0, r0, m0, lst0 = before = state(ctx)
    st = ctx.complete_points(max_error, image_ids=scope)
    pts, res, mask, lst = state(ctx)
    wp, wr, wm, wc, tr = ctw.run(host, tracks, ids, kps, lst0, cam, p0, r0, m0, thr, max_error, scope or (), trace=True)
    assert pts.tobytes() == wp.tobytes(), np.nonzero(pts != wp)[0][:8]
    assert res.tobytes() == wr.tobytes(), np.nonzero(res != wr)[0][:8]
    assert mask is not None and mask.tobytes() == wm.tobytes(), np.nonzero(mask != wm)[0][:8]
    assert lst[0].tobytes() == lst0[0].tobytes() and lst[1].tobytes() == lst0[1].tobytes()
    assert {k: st[k] for k in ctw.ALL_KEYS} == {k: wc[k] for k in ctw.ALL_KEYS}, (st, wc)
    assert st["complete_ms"] >= st["prepare_ms"] >= 0.0
    # the consequences: untouched and ineligible tracks bit for bit, completed ones keep X and the five history bits and still stand,
    # the bytes only rise, by exactly `admitted`
    o = tracks[0]
    per_obs = np.repeat(tr["kind"], np.diff(o))
    done = tr["kind"] == ctw.KIND_COMPLETED
    assert pts[~done].tobytes() == p0[~done].tobytes() and res[per_obs != 2].tobytes() == r0[per_obs != 2].tobytes()
    if m0 is not None:
        assert mask[per_obs != 2].tobytes() == m0[per_obs != 2].tobytes() and np.all(mask >= m0)
        assert int(mask.sum()) - int(m0.sum()) == st["admitted"]
    else:
        assert st["candidates"] == 0 and st["admitted"] == 0
    assert pts["X"].tobytes() == p0["X"].tobytes() and np.array_equal(pts["status"][done] & KEEP, p0["status"][done] & KEEP)
    assert np.all(_lib.completed(pts)[done]) and np.all((pts["status"][done] & STANDS) == STANDS)
    assert st["completed"] == int(done.sum()) and st["observations_used"] == int(p0["n_views"].sum()) + st["admitted"]
    assert st["candidates"] == st["admitted"] + st["rejected_by_depth"] + st["rejected_by_error"]
    if again:
        st2 = ctx.complete_points(max_error, image_ids=scope)
        assert same_state((pts, res, mask, lst), state(ctx)) and st2["admitted"] == 0 and st2["completed"] == 0, st2
        assert st2["succeeded"] == st["succeeded"] and st2["observations_used"] == st["observations_used"]
        assert st2["candidates"] == st["candidates"] - st["admitted"]
    return st, pts, res, mask, tr, before


def plant(ctx, ids, kps, where, after=None, **filter_kw):
    """where: [(track = keypoint row, image position)].  Each keypoint moves by 40 px, filter_points(**filter_kw) drops it, then the
    original keypoint -- or after[(track, position)] = (dx, dy) added to it -- is uploaded.  -> (the filter's stats, the keypoints)"""
    out = [np.array(k) for k in kps]
    for pos in sorted({p for _, p in where}):
        k = np.array(kps[pos])
        for j, p in where:
            if p == pos:
                k[j, 1] += np.float32(40.0)
        ctx.upload_keypoints(int(ids[pos]), k)
    st = ctx.filter_points(**filter_kw)
    assert st["dropped_by_error"] + st["dropped_by_depth"] >= len(where), st
    for (j, p), (dx, dy) in (after or {}).items():
        out[p][j, 0] += np.float32(dx)
        out[p][j, 1] += np.float32(dy)
    for pos in sorted({p for _, p in where}):
        ctx.upload_keypoints(int(ids[pos]), out[pos])
    return st, out


# ---- track counts: the wave and block edges of cmp_track_kernel ------------------------------------------------------------------------
@pytest.mark.parametrize("robust_session", (False, True))
def test_track_counts_at_the_wave_and_block_edges(tctx, host, robust_session):
    """T = 1, 63, 64, 65, 255, 256, 257 kept tracks under a (2 px, 1.5 degree) session; the tracks at the lanes 0, 63 | 64, 255 | 256
    have length 5 and a planted candidate in image 2, every other track has length 3 and no candidate.  On the plain session the bytes
    are created by the filter call in between; on the robust one they stand."""
    for T in (257, 256, 255, 65, 64, 63, 1):
        lengths = [5 if j in (0, 63, 64, 255, 256) else 3 for j in range(T)]
        ids, kps, poses, lst = ring_job(lengths, noise_px=0.1)
        assert open_ring(tctx, ids, kps, lst, T)["tracks_kept"] == T
        tracks = tctx.tracks()
        tctx.triangulate_tracks(CAM, poses, *THR, robust=robust_session, max_hypotheses=8)
        assert (code(tctx.point_inliers) == _lib.E_STATE) if not robust_session else tctx.point_inliers().all()
        touched = [j for j in (0, 63, 64, 255, 256) if j < T]
        fst, _ = plant(tctx, ids, kps, [(j, 2) for j in touched])
        assert fst["trimmed"] == len(touched) and fst["removed_by_views"] == fst["removed_by_angle"] == 0
        st, pts, res, mask, tr, before = complete_same(tctx, host, ids, kps, tracks, THR)
        assert np.array_equal(np.nonzero(tr["kind"] == ctw.KIND_COMPLETED)[0], touched) and st["eligible"] == T
        assert st["candidates"] == st["admitted"] == len(touched) and np.all(tr["kind"] >= ctw.KIND_UNTOUCHED)
        assert all(pts[j]["n_views"] == 5 and mask[tracks[0][j] + 2] == 1 and before[2][tracks[0][j] + 2] == 0 for j in touched)
        assert mask.all() and np.all((pts["status"][touched] & (_lib.TRI_FILTERED | _lib.TRI_COMPLETED)) == (_lib.TRI_FILTERED | _lib.TRI_COMPLETED))
        tctx.tracks_end()


def clean_second_pass_job(T, rows=8192):
    """second_pass_job's keypoints without its 40 px moves (it moves one observation of every third track and of every track of the last
    8192: the image t % 3 of track t) -> (ids, the job's keypoints, the clean ones, poses, lists)"""
    ids, kps, poses, lists = second_pass_job(T, rows)
    clean = []
    for q, kp in enumerate(kps):
        g, k = divmod(q, 3)
        t_abs = g * rows + np.arange(rows)
        hit = ((t_abs % 3 == 0) | (t_abs >= T - 8192)) & (t_abs < T) & (t_abs % 3 == k)
        c = np.array(kp)
        c[hit, 0] -= np.float32(40.0)
        clean.append(c)
    return ids, kps, clean, poses, lists


def test_second_grid_stride_pass(tctx, host):
    """cmp_track_kernel's grid holds 8 x CUs x 256 lanes: with 8192 tracks more its first 32 workgroups run a second pass of the
    wave-uniform t0 loop; ext_mask_kernel (in the filter call) and ref_obs_kernel run their second pass too.  Under a loose plain
    session over the clean keypoints, every third track and every track of the last 8192 gets one observation moved by 40 px, filtered
    out at (2 px, 1.5 degrees) and restored: a third of the tracks are completed, the second pass included."""
    t0 = time.time()
    cus = tctx.device_info()["cu_count"]
    T = 8 * 256 * cus + 8192
    ids, moved, clean, poses, lists = clean_second_pass_job(T)
    d = np.random.default_rng(1).integers(0, 256, (8192, 128), dtype=np.uint8)
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), d)
        tctx.upload_keypoints(int(i), clean[k])
    tctx.tracks_begin(ids, add_only=True)
    for l in lists:
        tctx.tracks_add(*l)
    assert tctx.tracks_finish()["tracks_kept"] == T
    tracks = tctx.tracks()
    thr = (60.0, 1.0, 2)
    tctx.triangulate_tracks(CAM, poses, *thr)
    for k, i in enumerate(ids):
        tctx.upload_keypoints(int(i), moved[k])
    fst = tctx.filter_points(2.0, 1.5)
    for k, i in enumerate(ids):
        tctx.upload_keypoints(int(i), clean[k])
    assert fst["trimmed"] >= T // 3 and fst["removed_by_views"] == 0
    st, pts, _, _, tr, _ = complete_same(tctx, host, ids, clean, tracks, thr, 2.0, again=False)
    tail = tr[T - 8192:]
    assert np.all(tail["kind"] == ctw.KIND_COMPLETED) and np.all(tail["admitted"] == 1)
    assert st["completed"] == st["admitted"] == fst["trimmed"] and st["eligible"] == T - fst["removed_by_angle"]
    assert (tr["kind"] == ctw.KIND_UNTOUCHED).sum() > T // 2
    print("second pass: T %d, complete_ms %.3f of which prepare %.3f, completed %d, filter before it trimmed %d, wall %.1f s" %
          (T, st["complete_ms"], st["prepare_ms"], st["completed"], fst["trimmed"], time.time() - t0))
    tctx.tracks_end()


# ---- where the admitted candidate sits in its track --------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_admitted_candidate_first_middle_last(tctx, host, where):
    """Tracks of 3, 4, 64, 65 and 129 elements, two of each, under a (2 px, 1 degree) session (two neighbouring views, 1.2 degrees,
    stand): the first five carry a planted candidate at their first, middle or last element, the second five are clean."""
    thr = (2.0, 1.0, 2)
    lengths = [3, 4, 64, 65, 129, 3, 4, 64, 65, 129]
    at = {t: {"first": 0, "middle": lengths[t] // 2, "last": lengths[t] - 1}[where] for t in range(5)}
    ids, kps, poses, lst = ring_job(lengths, noise_px=0.1)
    open_ring(tctx, ids, kps, lst, len(lengths))
    tracks = tctx.tracks()
    o = tracks[0]
    tctx.triangulate_tracks(CAM, poses, *thr)
    fst, _ = plant(tctx, ids, kps, [(t, at[t]) for t in range(5)])
    assert fst["trimmed"] == 5
    st, pts, res, mask, tr, before = complete_same(tctx, host, ids, kps, tracks, thr)
    for t in range(5):
        assert tr[t]["kind"] == ctw.KIND_COMPLETED and (tr[t]["candidates"], tr[t]["admitted"]) == (1, 1) and pts[t]["n_views"] == lengths[t]
        assert before[2][o[t] + at[t]] == 0 and mask[o[t]:o[t + 1]].all() and res[o[t] + at[t]] <= thr[0] < before[1][o[t] + at[t]]
    assert np.all(tr["kind"][5:] == ctw.KIND_UNTOUCHED) and not tr["candidates"][5:].any()
    tctx.tracks_end()


def test_candidate_next_to_an_unposed_and_a_rejected_element(tctx, host):
    """USED != FIT != all: eight-view tracks on a robust (2 px) session in which image 3 has no pose and the observation in image 4 of
    track 0 is 30 px off -- the triangulation's hypotheses reject it (byte 0, still USED) and it still does not fit.  The candidate
    planted in image 2 is admitted next to both."""
    ids, kps, poses, lst = ring_job([8] * 4, moved={0: [(4, 0.0, 30.0)]}, noise_px=0.05)
    open_ring(tctx, ids, kps, lst, 4)
    tracks = tctx.tracks()
    o = tracks[0]
    tctx.triangulate_tracks(CAM, some(poses, ids, (0, 1, 2, 4, 5, 6, 7)), *THR, robust=True, max_hypotheses=16)
    m0 = tctx.point_inliers()
    assert m0[o[0] + 4] == 0 and m0[o[0] + 3] == 0 and m0[o[0]:o[1]].sum() == 6
    plant(tctx, ids, kps, [(0, 2)])
    st, pts, res, mask, tr, before = complete_same(tctx, host, ids, kps, tracks, THR)
    assert tr[0]["kind"] == ctw.KIND_COMPLETED and (tr[0]["candidates"], tr[0]["admitted"], tr[0]["rejected_by_depth"]) == (2, 1, 0)
    assert mask[o[0]:o[1]].tolist() == [1, 1, 1, 0, 0, 1, 1, 1] and res[o[0] + 3] == -1.0 and res[o[0] + 4] > 20.0
    assert (pts["status"][0] & _lib.TRI_ROBUST) and np.all(tr["kind"][1:] == ctw.KIND_UNTOUCHED) and st["rejected_by_error"] == 1
    tctx.tracks_end()


# ---- every route of the rule ------------------------------------------------------------------------------------------------------------
def test_every_route(tctx, host):
    """A (2 px, 1.5 degree) plain session over six images of which image 5's camera is turned round (small errors, negative depth).
    The filter at (2 px, 1 degree) drops image 5 by depth from every six-view track and the planted candidates by error.  Then:
      track 0   the candidate in image 2 is the clean keypoint again: admitted.
      track 1   nothing planted: its only candidate is image 5: rejected by depth (as in every six-view track): untouched.
      track 2   the candidate in image 3 comes back 30 px off: rejected by error.
      track 3   the candidate in image 3 comes back as a NaN: rejected.
      track 4   the candidate in image 1 fits, the one in image 3 is 30 px off: both outcomes in one track.
      track 5   three views; without image 2 it has 1.2 degrees: the filter's 1 degree keeps it, the session's 1.5 take ANGLE_OK.  It
                does not stand: not eligible, although its candidate would fit."""
    lengths = [6, 6, 6, 6, 6, 3, 6, 6]
    ids, kps, poses, lst = ring_job(lengths, noise_px=0.1, turned=(5,))
    open_ring(tctx, ids, kps, lst, len(lengths))
    tracks = tctx.tracks()
    o = tracks[0]
    tctx.triangulate_tracks(CAM, poses, *THR)
    six = np.asarray(lengths) == 6
    fst, kps = plant(tctx, ids, kps, [(0, 2), (2, 3), (3, 3), (4, 1), (4, 3), (5, 2)],
                     after={(2, 3): (0.0, 30.0), (3, 3): (np.nan, 0.0), (4, 3): (0.0, 30.0)}, max_error=2.0, min_angle=1.0)
    assert fst["dropped_by_depth"] == 7 and fst["dropped_by_error"] == 6 and fst["trimmed"] == 8
    p0 = tctx.points3d()[0]
    assert (p0["status"][5] & STANDS) == (_lib.TRI_POINT | _lib.TRI_ERROR_OK) and np.all((p0["status"][six] & STANDS) == STANDS)
    st, pts, res, mask, tr, before = complete_same(tctx, host, ids, kps, tracks, THR)
    K = ctw
    assert tr["kind"].tolist() == [K.KIND_COMPLETED, K.KIND_UNTOUCHED, K.KIND_UNTOUCHED, K.KIND_UNTOUCHED, K.KIND_COMPLETED, K.KIND_NOT_ELIGIBLE,
                                   K.KIND_UNTOUCHED, K.KIND_UNTOUCHED], tr
    assert tr["rejected_by_depth"].tolist() == [1, 1, 1, 1, 1, 0, 1, 1] and tr["candidates"].tolist() == [2, 1, 2, 2, 3, 0, 1, 1]
    assert tr["admitted"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0] and st["rejected_by_error"] == 3 and st["eligible"] == 7
    assert mask[o[4]:o[5]].tolist() == [1, 1, 1, 0, 1, 0] and res[o[4] + 3] > 20.0 and mask[o[3] + 3] == 0 and mask[o[5] + 2] == 0
    assert (pts["status"][0] & _lib.TRI_DEPTH_OK) and mask[o[0] + 5] == 0 and res[o[0] + 5] >= 0.0   # (image 5 stays out; its slot is written)
    tctx.tracks_end()


def test_explicit_max_error_tighter_than_the_session(tctx, host):
    """a (4 px, 1.5 degree) session; the planted candidate comes back 2.5 px off: a call at 1 px rejects it, NULL parameters admit it"""
    thr = (4.0, 1.5, 2)
    ids, kps, poses, lst = ring_job([6] * 3, noise_px=0.05)
    open_ring(tctx, ids, kps, lst, 3)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, poses, *thr)
    _, kps = plant(tctx, ids, kps, [(1, 3)], after={(1, 3): (0.0, 2.5)})
    st, *_ = complete_same(tctx, host, ids, kps, tracks, thr, 1.0)
    assert (st["candidates"], st["admitted"], st["rejected_by_error"]) == (1, 0, 1)
    st, pts, res, mask, tr, _ = complete_same(tctx, host, ids, kps, tracks, thr)
    assert (st["candidates"], st["admitted"], st["completed"]) == (1, 1, 1) and 1.0 < res[tracks[0][1] + 3] <= 4.0 and mask.all()
    tctx.tracks_end()


def test_history_bits_are_kept_on_a_completed_record(tctx, host):
    """test_gpu_filter_points' history job: track 4 is retried at the robust triangulation (ROBUST), the session goes through
    refine_points (REFINED) and refine_poses (REPOSED), the images 0 and 4 arrive (EXTENDED), a filter at (1.8 px, 1.5 degrees) drops
    the observation in image 3 (FILTERED).  With NULL parameters (4 px) the completion admits it again, not the one 30 px off in image
    2, and the record keeps all five bits next to COMPLETED."""
    thr = (4.0, 1.5, 2)
    ids, kps, poses, lst = ring_job([6] * 6, moved={4: [(2, 0.0, 30.0), (3, 0.0, 3.6)]}, noise_px=0.1)
    open_ring(tctx, ids, kps, lst, 6)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, ids, (1, 2, 3, 5)), *thr, robust=True, max_hypotheses=8)
    tctx.refine_points()
    tctx.refine_poses(min_observations=3, fixed=[int(ids[1]), int(ids[3])])
    extend_same(tctx, host, ids, kps, tracks, some(poses, ids, (0, 4)), 0, thr=thr)
    filter_same(tctx, host, ids, kps, tracks, thr, (1.8, 1.5))
    p0 = tctx.points3d()[0]
    assert (p0["status"][4] & KEEP) == KEEP, p0["status"]
    st, pts, res, mask, tr, _ = complete_same(tctx, host, ids, kps, tracks, thr)
    b = tracks[0][4]
    assert tr[4]["kind"] == ctw.KIND_COMPLETED and (tr[4]["candidates"], tr[4]["admitted"]) == (2, 1)
    assert (pts["status"][4] & (KEEP | _lib.TRI_COMPLETED)) == (KEEP | _lib.TRI_COMPLETED)
    assert mask[b + 3] == 1 and mask[b + 2] == 0 and pts[4]["n_views"] == 5
    tctx.tracks_end()


# ---- the use case -----------------------------------------------------------------------------------------------------------------------
def test_extension_under_a_rough_pose_then_refinement_then_completion(tctx, host):
    """complete_fixtures' case 2 on the device: the increment arrives under poses 2 mrad and 5e-3 units off, extend_points rejects a
    large share of its observations, refine_poses repairs the poses, complete_points admits what had been rejected"""
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    first = [int(ids[p]) for p in efx.FIRST]
    tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR)
    bad = pfx.perturbed(poses, 7, rot=2e-3, trans=5e-3, keep=tuple(first))
    est, *_ = extend_same(tctx, host, ids, kps, tracks, some(bad, ids, efx.TWO[0]), 0)
    assert est["observations_rejected"] > 20 and est["observations_added"] > 20
    rp = tctx.refine_poses(min_observations=6, fixed=first)
    assert rp["refined"] == 2
    used0 = int(tctx.points3d()[0]["n_views"].sum())
    st, pts, res, mask, tr, before = complete_same(tctx, host, ids, kps, tracks, THR)
    assert st["admitted"] > 20 and st["observations_used"] == used0 + st["admitted"] == int(pts["n_views"].sum())
    rose = (mask != 0) & (before[2] == 0)
    assert np.isin(tracks[1][rose], [int(ids[p]) for p in efx.TWO[0]]).all() and np.all(res[rose] <= THR[0])
    done = tr["kind"] == ctw.KIND_COMPLETED
    assert np.all(_lib.reposed(pts)[done])
    tctx.tracks_end()


# ---- scope ------------------------------------------------------------------------------------------------------------------------------
def test_scope(tctx, host):
    """the extension's scene on a robust session, extended by the first of two increments and filtered at (1 px, 2.5 degrees): a listed
    image admits only its own candidates; a listed image without a pose selects nothing; an empty list against None; a permuted list
    gives the same bytes"""
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()

    def fresh():
        tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR, robust=True, max_hypotheses=64)
        tctx.extend_points(some(poses, ids, efx.TWO[0]))
        tctx.filter_points(1.0, 2.5)

    fresh()
    s0 = state(tctx)
    unposed = [int(ids[p]) for p in efx.TWO[1][:2]]
    st, *_ = complete_same(tctx, host, ids, kps, tracks, THR, None, unposed)
    assert st["candidates"] == 0 and st["eligible"] > 0 and same_state(s0, state(tctx))
    listed = [int(ids[p]) for p in efx.TWO[0]]
    st, pts, res, mask, tr, _ = complete_same(tctx, host, ids, kps, tracks, THR, None, listed)
    rose = (mask != 0) & (s0[2] == 0)
    assert st["admitted"] > 0 and np.isin(tracks[1][rose], listed).all()
    fresh()
    st2 = tctx.complete_points(image_ids=listed[::-1])
    assert same_state((pts, res, mask, s0[3]), state(tctx)) and {k: st2[k] for k in ctw.ALL_KEYS} == {k: st[k] for k in ctw.ALL_KEYS}
    fresh()
    st_all, p_all, r_all, m_all, _, _ = complete_same(tctx, host, ids, kps, tracks, THR, None, None)
    assert st_all["candidates"] > st["candidates"] and st_all["admitted"] >= st["admitted"]    # (the other images' candidates: the planted outliers)
    fresh()
    st_empty = tctx.complete_points(image_ids=[])
    assert same_state((p_all, r_all, m_all, s0[3]), state(tctx)) and {k: st_empty[k] for k in ctw.ALL_KEYS} == {k: st_all[k] for k in ctw.ALL_KEYS}
    tctx.tracks_end()


# ---- the calls that follow ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust_session", (False, True))
def test_following_calls_see_the_completed_state(tctx, host, robust_session):
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    kd = {int(i): k for i, k in zip(ids, kps)}
    mh = 16 if robust_session else 0
    bad = pfx.perturbed(poses, 5, rot=2e-4, trans=1e-3, keep=(int(ids[1]),))
    tctx.triangulate_tracks(CAM, some(bad, ids, efx.FIRST + efx.TWO[0]), *THR, robust=robust_session, max_hypotheses=16)
    filter_same(tctx, host, ids, kps, tracks, THR, (0.6, 4.0))
    tctx.refine_poses(min_observations=6)
    tctx.pose_refinements()
    tctx.register_images(CAM, [int(ids[6])], min_inliers=6)
    tctx.registrations()
    st, pts, res, mask, tr, _ = complete_same(tctx, host, ids, kps, tracks, THR)
    assert st["admitted"] > 0
    assert code(tctx.registrations) == _lib.E_STATE and code(tctx.pose_refinements) == _lib.E_STATE
    p0, r0, m0, lst0 = state(tctx)
    st = tctx.refine_points()
    wp, wr, wc = rtw.run(host, tracks, ids, kps, lst0, CAM, p0, r0, m0, THR[:2])
    pts, res = tctx.points3d()
    assert pts.tobytes() == wp.tobytes() and res.tobytes() == wr.tobytes() and st["refined"] == wc["refined"] > 0 and st["eligible"] == wc["eligible"]
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
    filter_same(tctx, host, ids, kps, tracks, THR, (1.0, 2.0))
    extend_same(tctx, host, ids, kps, tracks, some(bad, ids, efx.TWO[1]), mh)
    complete_same(tctx, host, ids, kps, tracks, THR)                                       # ... and once more behind the extension
    # a later triangulation and tracks_finish invalidate as before
    tctx.triangulate_tracks(CAM, some(bad, ids, efx.FIRST), *THR)
    assert code(tctx.point_inliers) == _lib.E_STATE and len(tctx.pose_list()[0]) == 3
    st = tctx.complete_points()                                                             # a session without bytes: they are created
    assert st["candidates"] == 0 and len(tctx.point_inliers()) == len(tracks[1])
    tctx.tracks_finish()
    assert code(tctx.complete_points) == _lib.E_STATE and code(tctx.point_inliers) == _lib.E_STATE
    tctx.tracks_end()


def test_filter_then_completion_at_the_same_threshold_and_back(tctx, host):
    """right after filter_points(e, a) a completion at max_error = e admits nothing the filter dropped; a filter at the completion's
    max_error, or looser, right after a completion drops nothing it admitted"""
    ids, kps, poses, _, seen = efx.scene()
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    tracks = tctx.tracks()
    tctx.triangulate_tracks(CAM, some(poses, ids, efx.FIRST), *THR, robust=True, max_hypotheses=64)
    tctx.extend_points(some(poses, ids, efx.TWO[0]))
    fst, *_ = filter_same(tctx, host, ids, kps, tracks, THR, (1.0, 2.5))
    assert fst["dropped_by_error"] > 0
    s0 = state(tctx)
    st, *_ = complete_same(tctx, host, ids, kps, tracks, THR, 1.0)
    assert st["candidates"] > 0 and st["admitted"] == 0 and same_state(s0, state(tctx))
    st, pts, res, mask, tr, _ = complete_same(tctx, host, ids, kps, tracks, THR, 1.6)
    assert st["admitted"] > 0
    rose = (mask != 0) & (s0[2] == 0)
    for e in (1.6, 2.0):
        filter_same(tctx, host, ids, kps, tracks, THR, (e, 0.0))
        assert tctx.point_inliers()[rose].all()
    tctx.tracks_end()


def test_errors_leave_the_session_alone(tctx, host):
    E = _lib
    ids, kps, poses, _, seen = efx.scene()
    assert code(tctx.complete_points) == E.E_STATE                                            # no session
    open_ring(tctx, ids, kps, pfx.match_list(seen, ids), efx.T)
    assert code(tctx.complete_points) == E.E_STATE                                            # finished, not triangulated
    first = some(poses, ids, efx.FIRST)
    tctx.triangulate_tracks(CAM, first, *THR, robust=True)
    tctx.refine_poses(min_observations=6)
    tctx.register_images(CAM, [int(ids[4])], min_inliers=6)
    s0 = state(tctx)
    good = int(ids[1])
    above = float(np.nextafter(THR[0], np.inf))                                               # just above the session's
    for kw in (dict(max_error=np.nan), dict(max_error=np.inf), dict(max_error=-1.0), dict(max_error=above), dict(image_ids=[good, 77]),
               dict(image_ids=[good, 20000]), dict(image_ids=[good, -1]), dict(image_ids=[good, int(ids[2]), good])):   # the bad id BEHIND a good one
        assert code(tctx.complete_points, **kw) == E.E_INVALID, kw
        assert same_state(s0, state(tctx))
        tctx.registrations()                                                                  # still valid: nothing was touched
        tctx.pose_refinements()
    assert tctx._L.msfm_complete_points(tctx._h, None, None, 1, None) == E.E_INVALID          # a NULL list with n_images > 0
    assert tctx._L.msfm_complete_points(tctx._h, None, None, -1, None) == E.E_INVALID
    assert same_state(s0, state(tctx))
    tctx.registrations()
    assert tctx.complete_points(max_error=THR[0])["admitted"] >= 0                            # the session's own value is allowed
    assert code(tctx.registrations) == E.E_STATE and code(tctx.pose_refinements) == E.E_STATE  # a successful call invalidates them
    assert tctx._L.msfm_complete_points(tctx._h, None, None, 0, None) == E.OK                 # NULL params and stats, no list
    tctx.tracks_end()
    assert code(tctx.complete_points) == E.E_STATE


# ---- the loop ---------------------------------------------------------------------------------------------------------------------------
def grow_scene():
    """test_gpu_filter_points.test_reconstruct_filters_after_every_increment's scene"""
    n_img, T = 9, 120
    ids, kps, poses, seen = pfx.chosen_scene(pfx.general_points(T, 53), [T] * n_img, noise_px=0.3, seed=3)
    for i in range(n_img):
        seen[:, i] = False
        seen[max(0, 12 * i - 30):12 * i + 54, i] = True
    for t, i in ((40, 4), (55, 5), (70, 6), (85, 7), (100, 8)):
        assert seen[t, i]
        kps[i][t, 1] += np.float32(30.0)
    return ids, kps, poses, seen, T


def test_reconstruct_completes_after_every_increment(tctx, host):
    """reconstruct(complete_params={}) on the filter test's grow scene: every increment's device state equals the twins run in the same
    order (registration, extension, point refinement, pose refinement, filter, completion); at the end no fitting observation of a
    standing point exceeds max_error, and the fitting observations are not fewer than in the same run without completion."""
    ids, kps, poses, seen, T = grow_scene()
    kd = {int(i): k for i, k in zip(ids, kps)}
    reg_host = regtw.load_host()
    fixed = [int(ids[0])]
    kw = dict(register_params=dict(min_inliers=15), fixed=fixed, pose_params=dict(min_observations=15))

    def start(ctx):
        open_ring(ctx, ids, kps, pfx.match_list(seen, ids), T)
        ctx.triangulate_tracks(CAM, some(poses, ids, (0, 1, 2)), *THR)
        ctx.refine_points()
        return ctx.tracks()

    tracks = start(tctx)
    o = tracks[0]
    done, admitted = [], 0
    while True:
        p0, r0, m0, lst0 = state(tctx)
        todo = [int(i) for i in ids if int(i) not in tctx.poses()]
        out = tctx.reconstruct(CAM, rounds=2, max_increments=1, complete_params={}, **kw)
        if not out:
            assert not todo or same_state((p0, r0, m0, lst0), state(tctx))
            break
        inc = out[0]
        assert sorted(inc) == ["alternate", "complete", "extend", "filter", "register", "registered"]
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
        wp, wr, wm, c4 = ctw.run(host, tracks, ids, kps, wl, CAM, wp, wr, wm, THR[:2])
        assert {k: inc["complete"][k] for k in ctw.ALL_KEYS} == c4
        admitted += c4["admitted"]
        pts, res, mask, lst = state(tctx)
        assert pts.tobytes() == wp.tobytes() and res.tobytes() == wr.tobytes() and mask.tobytes() == wm.tobytes()
        assert lst[0].tobytes() == wl[0].tobytes() and lst[1].tobytes() == wl[1].tobytes()
    assert sorted(done + [int(ids[p]) for p in (0, 1, 2)]) == [int(i) for i in ids]
    assert len(tctx.reconstruct(CAM, complete_params={}, **kw)) == 0
    pts, res, mask, _ = state(tctx)
    fit = (mask != 0) & np.repeat(_lib.succeeded(pts), np.diff(o))
    assert fit.sum() > 400 and np.all(res[fit] <= THR[0])
    tctx.tracks_end()
    # the same run without completion, on a context of its own
    ctx2 = _lib.Context(0)
    try:
        start(ctx2)
        plain = ctx2.reconstruct(CAM, rounds=2, **kw)
        assert all(sorted(inc) == ["alternate", "extend", "filter", "register", "registered"] for inc in plain)
        p2, _, m2, _ = state(ctx2)
        fit2 = (m2 != 0) & np.repeat(_lib.succeeded(p2), np.diff(o))
    finally:
        ctx2.close()
    print("reconstruct: %d fitting observations with completion (%d admitted over the increments), %d without" %
          (int(fit.sum()), admitted, int(fit2.sum())))
    assert fit.sum() >= fit2.sum()
