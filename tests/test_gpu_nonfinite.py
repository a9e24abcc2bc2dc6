"""Non-finite and huge keypoint coordinates through the reconstruction kernels and the verified matching call:
the device against the host twins BYTE FOR BYTE on the placements of tests/nonfinite_fixtures.py, every call of the chain compared with
its twin fed the device's own state before the call.  msfm_upload_keypoints validates nothing, so NaNs, infinities, 3e38 and denormals
reach every kernel that reads a keypoint; tests/test_nonfinite_reference.py proves on the CPU, for the identical fixtures and for every
value, that the twins end, that they treat the value as a gross outlier, and that the routes asserted there are reached.  Here each test
draws a few values from a fixed seed (always a signed NaN and an infinity: the values whose NaNs the two processors propagate or
generate with different bits -- msfm_pose.h, "THE NaN RULE").

The thin comparison helpers below are the existing *_same helpers with one change: a cost sum is compared to 1e-9 relative where
both sides are finite, and must otherwise be the same infinity or NaN on both sides.  (msfm_complete_points reports no cost sum: its
eight counters are integers and compared exactly, by test_gpu_complete_points.complete_same itself.)

THE COMPLETION runs on a SECOND PASS of the chain: the calls up to the last point refinement are made again (rebuilt(): the same calls
on the same inputs, so the same state -- asserted byte for byte against the first pass), then the filter under FILTER_TRIM and the
completion behind it; again, then FILTER_TRIM, FILTER_MIX and the completion; again, then the planted route and the cure
(planted_and_cured()).  So the inputs of every comparison of the first pass are what they were before the completion was added."""
import time

import numpy as np
import pytest

import complete_twin as ctw
import extend_twin as etw
import filter_twin as ftw
import nonfinite_fixtures as nf
import refine_points_twin as rtw
import refine_poses_twin as ptw
import registration_twin as regtw
import robust_triangulation_twin as robtw
import triangulation_twin as tw
from monocularsfm_amd import _lib
from test_gpu_complete_points import complete_same
from test_gpu_extend_points import same_state, state
from test_gpu_robust_triangulation import open_ring

pytestmark = pytest.mark.gpu
CAMS = {"cam": nf.CAM, "cam_d": nf.CAM_D}
PLACEMENTS = {"lanes": nf.lanes, "wave": nf.whole_wave, "images": nf.images}
CANONICAL = 0x7ff8000000000000
H = 8


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return nf.load_host()


def same_bytes(got, want, what):
    assert got.tobytes() == want.tobytes(), (what, np.nonzero(np.atleast_1d(got != want))[0][:8])


def same_cost(a, b, what):
    if np.isfinite(a) and np.isfinite(b):
        assert abs(a - b) <= 1e-9 * max(abs(b), 1e-300), (what, a, b)
    else:
        assert (a != a and b != b) or a == b, (what, a, b)


def only_the_nan(res, bad, what):
    """NaNs only in the bad observations' slots, and only THE NaN"""
    res = np.ascontiguousarray(res, np.float64)
    nan = np.isnan(res)
    assert not nan[~bad].any(), what
    assert set(int(v) for v in res.view(np.uint64)[nan]) <= {CANONICAL}, (what, [hex(int(v)) for v in set(res.view(np.uint64)[nan])])


def open_scene(ctx, sc):
    st = open_ring(ctx, sc.ids, sc.kps, sc.lst, sc.rows)
    tracks = ctx.tracks()
    assert st["tracks_kept"] == len(sc.lengths) and all(np.array_equal(a, b) for a, b in zip(tracks, sc.tracks))
    return tracks


def triangulated(ctx, host, sc, tracks, poses, cam, robust, what):
    st = ctx.triangulate_tracks(cam, poses, *nf.THR, robust=robust, max_hypotheses=H)
    pts, res = ctx.points3d()
    if robust:
        wp, wr, wm, wc = robtw.run(host, tracks, sc.ids, sc.kps, poses, cam, nf.THR + (H,))
        same_bytes(ctx.point_inliers(), wm, what)
        assert {k: st[k] for k in robtw.ROBUST_KEYS} == wc, (what, st, wc)
    else:
        wp, wr = tw.run(host, tracks, sc.ids, sc.kps, poses, cam, nf.THR)
    same_bytes(pts, wp, what)
    same_bytes(res, wr, what)
    assert {k: st[k] for k in tw.COUNT_KEYS} == tw.counts(wp) and st["tracks"] == len(pts), (what, st)
    only_the_nan(res, sc.bad, what)
    return st, pts, res


def points_refined(ctx, host, sc, tracks, cam, what, finite_costs=True):
    p0, r0, m0, l0 = state(ctx)
    st = ctx.refine_points()
    pts, res = ctx.points3d()
    wp, wr, wc = rtw.run(host, tracks, sc.ids, sc.kps, l0, cam, p0, r0, m0, nf.THR[:2])
    same_bytes(pts, wp, what)
    same_bytes(res, wr, what)
    assert {k: st[k] for k in rtw.COUNT_KEYS} == {k: wc[k] for k in rtw.COUNT_KEYS}, (what, st, wc)
    for k in rtw.COST_KEYS:
        same_cost(st[k], wc[k], (what, k))
        assert not finite_costs or np.isfinite(st[k]), (what, k, st[k])
    only_the_nan(res, sc.bad, what)
    return st, pts, res


def registered(ctx, host, sc, tracks, cam, what):
    pts = ctx.points3d()[0]
    image_id = int(sc.ids[nf.REG])
    st = ctx.register_images(cam, [image_id], **nf.REG_PARAMS)
    got = ctx.registrations()
    want = regtw.run(host, tracks, pts, [image_id], sc.kd(), cam, **nf.REG_PARAMS)
    for g, w, name in zip(got, want, ("records", "offsets", "track ids", "flags", "residuals")):
        same_bytes(g, w, (what, name))
    badc = nf.registration_bad(sc, got)
    assert not got[3][badc].any(), what                                            # a bad correspondence is never an inlier
    only_the_nan(got[4], badc, what)
    return st, got


def extended(ctx, host, sc, tracks, new, mh, cam, what):
    p0, r0, m0, l0 = state(ctx)
    st = ctx.extend_points(new, mh)
    pts, res, mask, lst = state(ctx)
    wp, wr, wm, wc, wl, tr = etw.run(host, tracks, sc.ids, sc.kps, l0, new, cam, p0, r0, m0, nf.THR, mh, trace=True)
    same_bytes(pts, wp, what)
    same_bytes(res, wr, what)
    same_bytes(mask, wm, what)
    same_bytes(lst[0], wl[0], what)
    same_bytes(lst[1], wl[1], what)
    keys = etw.COUNT_KEYS + ("images_added", "succeeded", "observations_used")
    assert {k: st[k] for k in keys} == {k: wc[k] for k in keys}, (what, st, wc)
    only_the_nan(res, sc.bad, what)
    return st, pts, res, mask, tr


def poses_refined(ctx, host, sc, tracks, cam, what):
    p0, r0, m0, l0 = state(ctx)
    fixed = [int(sc.ids[nf.OLD[0]])]
    st = ctx.refine_poses(*nf.POSE_PARAMS, fixed=fixed)
    pts, res, m1, l1 = state(ctx)
    rec = ctx.pose_refinements()
    wp, wr, wl, wrec, wc = ptw.run(host, tracks, sc.ids, sc.kps, l0, cam, p0, r0, m0, nf.THR[:2], nf.POSE_PARAMS, fixed)
    same_bytes(l1[0], wl[0], what)
    same_bytes(l1[1], wl[1], what)
    same_bytes(rec, wrec, what)
    same_bytes(pts, wp, what)
    same_bytes(res, wr, what)
    same_bytes(m1, m0, what)
    assert {k: st[k] for k in ptw.COUNT_KEYS} == {k: wc[k] for k in ptw.COUNT_KEYS}, (what, st, wc)
    for k in ptw.COST_KEYS:
        same_cost(st[k], wc[k], (what, k))
        assert np.isfinite(st[k]), (what, k, st[k])
    only_the_nan(res, sc.bad, what)
    return st, pts, res, rec


def filtered(ctx, host, sc, tracks, cam, what, params=None, creates_bytes=False):
    """one msfm_filter_points (params: the call's (max_error, min_angle), None: the session's) against FilterPoints run from the
    device's state before the call -- records, residuals, inlier bytes and the pose list by bytes, all nine counters -- THE NaN alone,
    and a second call that changes no byte and counts nothing.  creates_bytes: the session has no inlier bytes before the call.
    -> (stats, points, residuals, bytes, the twin's trace)"""
    t0 = time.perf_counter()
    p0, r0, m0, l0 = state(ctx)
    assert (m0 is None) == creates_bytes, what
    kw = {} if params is None else dict(max_error=params[0], min_angle=params[1])
    st = ctx.filter_points(**kw)
    pts, res, mask, lst = after = state(ctx)
    wp, wr, wm, wc, tr = ftw.run(host, tracks, sc.ids, sc.kps, l0, cam, p0, r0, m0, nf.THR[:2], params, trace=True)
    same_bytes(pts, wp, what)
    same_bytes(res, wr, what)
    assert mask is not None, what
    same_bytes(mask, wm, what)
    same_bytes(lst[0], l0[0], what)
    same_bytes(lst[1], l0[1], what)
    assert {k: st[k] for k in ftw.ALL_KEYS} == {k: wc[k] for k in ftw.ALL_KEYS}, (what, st, wc)
    only_the_nan(res, sc.bad, what)
    st2 = ctx.filter_points(**kw)
    assert same_state(after, state(ctx)), what
    assert all(st2[k] == (st[k] if k in ("succeeded", "observations_used") else 0) for k in ftw.ALL_KEYS if k != "eligible"), (what, st2)
    SECONDS["filter"].append(time.perf_counter() - t0)
    return st, pts, res, mask, tr


SECONDS = {"filter": [], "complete": []}     # wall time of every filtered() and completed() of a run, twins and second calls included


def completed(ctx, host, sc, tracks, cam, what, kps=None, max_error=None, scope=None, case=None):
    """one msfm_complete_points (max_error None: the session's; kps: the keypoints the session holds, None = the scene's) against
    CompletePoints run from the device's state before the call, with test_gpu_complete_points.complete_same's comparisons -- records,
    residuals, inlier bytes and the pose list by bytes, all eight counters, the consequences of the rule, and the second call that
    changes no byte and admits nothing -- and THE NaN alone.  With `case`, nonfinite_fixtures.completion_routes on the twin's trace of
    the device's own state: no byte on a bad observation, bad candidates rejected by error and never by depth, untouched tracks
    untouched, what a completed bad track's rewritten slots hold.
    -> (stats, points, residuals, bytes, the twin's trace, the state before, the completed bad tracks, the untouched ones with a
    rejected bad candidate)"""
    t0 = time.perf_counter()
    st, pts, res, mask, tr, before = complete_same(ctx, host, sc.ids, sc.kps if kps is None else kps, tracks, nf.THR, max_error, scope, cam=cam)
    SECONDS["complete"].append(time.perf_counter() - t0)
    only_the_nan(res, sc.bad, what)
    assert st["rejected_by_depth"] == 0, (what, st)
    done = untouched = None
    if case is not None:
        posed = np.isin(tracks[1], [int(i) for i, p in zip(*before[3]) if p["valid"]])
        # (a track created on the plain route over a bad observation carries the extension's byte 1 on it: second form, left out)
        tight = ~(np.add.reduceat(((before[2] != 0) & sc.bad).astype(np.int64), tracks[0][:-1]) > 0)
        done, untouched = nf.completion_routes(sc, case, cam, posed, before[:3], (pts, res, mask, st, tr), tight, what, scope)
    return st, pts, res, mask, tr, before, done, untouched


def robust_session(ctx, host, sc, tracks, cam, mh, what, finite=True):
    """robust triangulation under the OLD images' poses, point refinement, registration of REG, extension by NEW and REG's registered
    pose with max_hypotheses mh, pose refinement, point refinement: each against its twin -> dict step -> the device's outputs"""
    first = sc.some([p for p in nf.OLD if p < len(sc.ids)])
    out = {}
    out["robust"] = triangulated(ctx, host, sc, tracks, first, cam, True, what + ("robust",))
    out["refine1"] = points_refined(ctx, host, sc, tracks, cam, what + ("refine1",))
    new = sc.some([p for p in nf.NEW if p < len(sc.ids)])
    if nf.REG < len(sc.ids):
        out["register"] = registered(ctx, host, sc, tracks, cam, what + ("register",))
        new = _lib.registered_poses(out["register"][1][0], new)
    out["extend"] = extended(ctx, host, sc, tracks, new, mh, cam, what + ("extend",))
    out["poses"] = poses_refined(ctx, host, sc, tracks, cam, what + ("poses",))
    # (with max_hypotheses 0 a bad 3-view track is created on the plain route: after it the sums may be +inf as after the plain call)
    out["refine2"] = points_refined(ctx, host, sc, tracks, cam, what + ("refine2",), finite_costs=mh > 0 or finite)
    out["state"] = state(ctx)
    return out


def rebuilt(ctx, sc, cam, mh, session):
    """the calls of robust_session once more, without the comparisons: the same calls on the same inputs leave the same state --
    asserted against `session`, the first pass's outputs"""
    ctx.triangulate_tracks(cam, sc.some([p for p in nf.OLD if p < len(sc.ids)]), *nf.THR, robust=True, max_hypotheses=H)
    ctx.refine_points()
    new = sc.some([p for p in nf.NEW if p < len(sc.ids)])
    if nf.REG < len(sc.ids):
        ctx.register_images(cam, [int(sc.ids[nf.REG])], **nf.REG_PARAMS)
        new = _lib.registered_poses(ctx.registrations()[0], new)
    ctx.extend_points(new, mh)
    ctx.refine_poses(*nf.POSE_PARAMS, fixed=[int(sc.ids[nf.OLD[0]])])
    ctx.refine_points()
    assert same_state(session["state"], state(ctx)), "the second pass of the chain left another state than the first"


def planted_and_cured(ctx, host, sc, tracks, cam, what, case):
    """From the state behind the last point refinement, test_gpu_complete_points.plant()'s method on nonfinite_fixtures.planted_tracks:
    the keypoints of image PLANT_AT are uploaded with those tracks' observations moved by 40 px, filter_points under the session's
    thresholds drops them (against its twin, fed the moved keypoints), the original keypoints are uploaded again, and the completion
    finds them: EVERY bad 8-view track that stands is completed, its bad candidates rejected beside the admitted one.  Then one call
    with max_error = -0.0 (accepted; nothing fits exactly: no byte moves) and one scoped to REG.  THE CURE: the true keypoints are
    uploaded in place of the bad ones (the clean scene of the same seed) and the completion admits them: the twin's trace says so for
    every bad track that stands, no NaN is left in a completed track.  -> (the planted call's outputs, the cure's)"""
    moved = nf.Scene(sc.ids, nf.moved_keypoints(sc), sc.poses, sc.lst, sc.lengths, sc.bad)
    ctx.upload_keypoints(int(sc.ids[nf.PLANT_AT]), moved.kps[nf.PLANT_AT])
    fst, fp, _, fm, ftr = filtered(ctx, host, moved, tracks, cam, what + ("planted filter",))
    ctx.upload_keypoints(int(sc.ids[nf.PLANT_AT]), sc.kps[nf.PLANT_AT])
    o = tracks[0]
    where = np.zeros(len(sc.lengths), bool)
    where[nf.planted_tracks(sc)] = True
    badt = np.zeros(len(sc.lengths), bool)
    badt[sc.bad_tracks()] = True
    stands = _lib.succeeded(fp) & (tracks[3] != 0)
    read = where & (ftr["kind"] != ftw.KIND_NOT_ELIGIBLE)
    assert np.all(ftr["dropped_by_error"][read] >= 1) and not fm[o[:-1][read] + nf.PLANT_AT].any(), (what, fst)
    zero = completed(ctx, host, sc, tracks, cam, what + ("-0.0",), max_error=-0.0, case=case)
    assert zero[0]["admitted"] == 0 and zero[0]["candidates"] == zero[0]["rejected_by_error"] > 0 and same_state(zero[5], state(ctx)), (what, zero[0])
    if nf.REG < len(sc.ids) and int(sc.ids[nf.REG]) in ctx.poses():
        # (scoped to REG: image 7's candidates alone, the bad ones rejected; what it admits the full call would have admitted as well)
        reg = int(sc.ids[nf.REG])
        scoped = completed(ctx, host, sc, tracks, cam, what + ("scoped",), scope=[reg], case=case)
        rose = (scoped[3] != 0) & (scoped[5][2] == 0)
        assert np.all(tracks[1][rose] == reg) and scoped[0]["candidates"] == int(((tracks[1] == reg) & (scoped[5][2] == 0) & np.repeat(stands, np.diff(o))).sum())
    out = completed(ctx, host, sc, tracks, cam, what + ("planted",), case=case)
    long_bad = badt & where
    # (on this robust session every bad 8-view track stands, unless the plain route of max_hypotheses 0 created it: second form)
    assert np.array_equal(out[6][long_bad], stands[long_bad]) and (out[6].any() or not stands[long_bad].any()), (what, out[4][long_bad])
    assert np.all(out[4]["admitted"][where & stands] >= 1), (what, out[4][where & stands])
    for pos in sorted(set(nf.BAD_AT + nf.BAD_AT_SHORT)):
        if pos < len(sc.ids):
            ctx.upload_keypoints(int(sc.ids[pos]), sc.clean[pos])
    cure = completed(ctx, host, sc, tracks, cam, what + ("cure",), kps=sc.clean)
    st, pts, res, mask, tr, before = cure[:6]
    gained = (mask != 0) & (before[2] == 0)
    done = np.repeat(tr["kind"] == ctw.KIND_COMPLETED, np.diff(o))
    assert np.all(sc.bad[gained]) and np.all(np.isfinite(res[gained]) & (res[gained] <= nf.THR[0])), what
    assert not np.isnan(res[done]).any() and not np.isnan(res[~sc.bad]).any(), what
    assert not (before[1][gained] <= nf.THR[0]).any(), what
    if case[0].startswith("nan"):
        assert np.isnan(before[1][gained]).all(), what
    # every formerly bad observation of a standing 8-view track sits 0.3 px of noise from its point: admitted (the twin decides; that
    # it admits them all on these fixtures is tests/test_nonfinite_reference.py::test_the_cure's finding, from tests/complete_ref.py)
    tight = ~(np.add.reduceat(((before[2] != 0) & sc.bad).astype(np.int64), o[:-1]) > 0)
    assert st["admitted"] == int(gained.sum()) and st["admitted"] >= int((badt & stands & tight).sum()), (what, st)
    return out, cure


def chain(ctx, host, sc, cam, mh, case):
    """The calls of the stage in order on one session, each against its twin fed the device's state before it: plain triangulation and
    a point refinement on it, the filter on that plain session (it creates the inlier bytes) and the refinement that follows it;
    robust triangulation, point refinement, registration of REG, extension by NEW and REG's registered pose with max_hypotheses mh,
    pose refinement, point refinement; the filter under FILTER_TRIM, then under the tighter FILTER_MIX, and a point refinement; then,
    each behind a robust triangulation under the session's final poses (the state no filter has touched), the filter under
    FILTER_ANGLE and under FILTER_VIEWS; then the second pass with the completion (module docstring).
    -> dict step -> the device's outputs"""
    what = (case and case[0], mh)
    tracks = open_scene(ctx, sc)
    first = sc.some([p for p in nf.OLD if p < len(sc.ids)])
    out = {}
    out["plain"] = triangulated(ctx, host, sc, tracks, first, cam, False, what + ("plain",))
    # (after the plain call a bad track under 3e38 or 1e30 is eligible with an error that overflows: the cost sums are +inf there, on
    # both sides; under a NaN or an infinity the track has no point and the sums are finite -- tests/test_nonfinite_reference.py)
    finite = case is None or nf.non_finite(case) or case[0].startswith(("denormal", "minus_zero"))
    out["refine0"] = points_refined(ctx, host, sc, tracks, cam, what + ("refine0",), finite_costs=finite)
    # (the filter removes or trims every eligible bad track, the others have no point: every sum is finite behind it, whatever the value)
    out["filter0"] = filtered(ctx, host, sc, tracks, cam, what + ("filter0",), creates_bytes=True)
    out["refine0f"] = points_refined(ctx, host, sc, tracks, cam, what + ("refine0f",))
    out.update(robust_session(ctx, host, sc, tracks, cam, mh, what, finite))
    out["filter_trim"] = filtered(ctx, host, sc, tracks, cam, what + ("trim",), nf.FILTER_TRIM)
    out["filter_mix"] = filtered(ctx, host, sc, tracks, cam, what + ("mix",), nf.FILTER_MIX)
    out["refine3"] = points_refined(ctx, host, sc, tracks, cam, what + ("refine3",))
    last = ctx.poses()
    for name, pair in (("angle", nf.FILTER_ANGLE), ("views", nf.FILTER_VIEWS)):
        triangulated(ctx, host, sc, tracks, last, cam, True, what + ("robust before " + name,))
        out["filter_" + name] = filtered(ctx, host, sc, tracks, cam, what + (name,), pair)
    # the second pass (module docstring): the completion behind FILTER_TRIM, behind FILTER_TRIM then FILTER_MIX, and planted
    for name in ("trim", "mix"):
        rebuilt(ctx, sc, cam, mh, out)
        for pair in (nf.FILTER_TRIM, nf.FILTER_MIX)[:1 if name == "trim" else 2]:
            ctx.filter_points(max_error=pair[0], min_angle=pair[1])
        for got, want in zip(state(ctx)[:3], out["filter_" + name][1:4]):
            same_bytes(got, want, what + ("the second pass behind " + name,))
        out["complete_" + name] = completed(ctx, host, sc, tracks, cam, what + ("complete behind " + name,), case=case)
    if case is not None:
        rebuilt(ctx, sc, cam, mh, out)
        out["complete_planted"], out["cure"] = planted_and_cured(ctx, host, sc, tracks, cam, what, case)
    ctx.tracks_end()
    return out


@pytest.mark.parametrize("cam", sorted(CAMS))
@pytest.mark.parametrize("place", sorted(PLACEMENTS))
def test_the_chain_on_one_session(tctx, host, place, cam):
    """every call of the chain against its twin, with max_hypotheses 8 (the retry list runs) and 0 (ext_mask_kernel and the plain
    route); the routes the fixture is for, on the device's own outputs.  The filter runs five times per chain: on the plain session
    (ext_mask_kernel as the filter launches it) and under the four pairs of nonfinite_fixtures.FILTER_PAIRS.  The completion runs
    on the second pass of every chain: behind FILTER_TRIM, behind FILTER_TRIM and FILTER_MIX, planted, with max_error -0.0, scoped to
    REG, and on the cured keypoints.  The wall time of the filter steps and of the completion steps is printed."""
    for k in SECONDS:
        del SECONDS[k][:]
    for n, case in enumerate(nf.drawn(seed=sorted(PLACEMENTS).index(place) * 2 + sorted(CAMS).index(cam), k=3)):
        sc = PLACEMENTS[place](case)[0]
        for mh in (8, 0):
            out = chain(tctx, host, sc, CAMS[cam], mh, case)
            st = out["robust"][0]
            o = sc.tracks[0]
            old_bad = sum(1 for t, n_ in enumerate(sc.lengths) if n_ == 8 and sc.bad[o[t] + 4])
            assert st["retried"] == st["rescued"] == st["observations_rejected"] == old_bad > 0, (case[0], st)
            ext_st, _, _, mask, tr = out["extend"]
            created = np.repeat(tr["kind"] == etw.KIND_CREATE, np.diff(o))   # (on the plain route a created track's bytes are 1 on every view)
            assert ext_st["observations_rejected"] > 0 and not mask[sc.bad & ~(created & (mh == 0))].any()
            if place == "images":
                short_bad = [t for t in sc.bad_tracks() if sc.lengths[t] == 3]
                assert np.all(tr["kind"][short_bad] == etw.KIND_CREATE) and ext_st["retried"] == (len(short_bad) if mh else 0)
                assert _lib.registered(out["register"][1][0]).all()
            # the filter's routes, on the twin's traces of the device's own states
            badt = np.zeros(len(sc.lengths), bool)
            badt[sc.bad_tracks()] = True
            trims = [out[k][4]["kind"] == ftw.KIND_TRIMMED for k in ("filter_trim", "filter_mix")]
            assert (trims[0] & badt).any() or (trims[1] & badt).any(), (case[0], mh)      # a bad track's slots were rewritten
            assert (out["filter_trim"][4]["kind"][~badt] == ftw.KIND_UNTOUCHED).any() and out["filter_mix"][0]["trimmed"] > 0
            assert out["filter_angle"][0]["removed_by_angle"] > 0 and out["filter_views"][0]["removed_by_views"] > 0, (case[0], mh)
            # the completion's routes (tests/test_nonfinite_reference.py, compare_complete), on the twin's traces of the device's own
            # states: behind the filter a bad track is completed -- its bad slots rewritten -- under one of the two pairs at least,
            # and one with a rejected bad candidate is left untouched; on the planted route every standing bad 8-view track is
            # completed (asserted in planted_and_cured) and the cure admits the formerly bad observations
            behind = [out["complete_trim"], out["complete_mix"]]
            assert (behind[0][6] | behind[1][6]).any() and (behind[0][7] | behind[1][7]).any(), (case[0], mh, [b[0] for b in behind])
            reached = dict(behind_trim=int(behind[0][6].sum()), behind_mix=int(behind[1][6].sum()), planted=int(out["complete_planted"][6].sum()),
                           untouched=[int(b[7].sum()) for b in behind], cured=out["cure"][0]["admitted"])
            assert reached["planted"] > 0 and reached["cured"] > 0, (case[0], mh, reached)
            print(place, cam, case[0], mh, "bad tracks completed / left untouched with a rejected bad candidate / observations cured:", reached)
    print("wall time of this test's filter steps: %d calls, %.3f s; of its completion steps: %d calls, %.3f s" %
          (len(SECONDS["filter"]), sum(SECONDS["filter"]), len(SECONDS["complete"]), sum(SECONDS["complete"])))


@pytest.mark.parametrize("T", [257, 256, 255, 65, 64, 63, 1])
def test_track_count_prefixes_of_the_lane_placement(tctx, host, T):
    """the first T tracks of the lane placement: the last wave and the last block full, one short, one over; one track"""
    case = nf.drawn(seed=11, k=4)[[257, 256, 255, 65, 64, 63, 1].index(T) % 4]
    sc = nf.lanes(case)[0].prefix(T)
    assert len(sc.bad_tracks()) == sum(t < T for t in nf.LANES)
    out = chain(tctx, host, sc, nf.CAM, 8 if T % 2 else 0, case)
    # the completion step of every prefix: each bad track of it is planted and completed, at whatever lane the prefix ends
    planted = out["complete_planted"]
    assert np.all(planted[4]["kind"][sc.bad_tracks()] == ctw.KIND_COMPLETED) and planted[6].sum() == len(sc.bad_tracks()), (T, planted[4][sc.bad_tracks()])


@pytest.mark.parametrize("cam", sorted(CAMS))
@pytest.mark.parametrize("place", ["lanes", "wave"])
def test_completion_on_the_planted_route(tctx, host, place, cam):
    """planted_and_cured() behind the robust session (max_hypotheses 8) with values of its own draw (always a signed NaN and an
    infinity).  lanes: the bad tracks at the lanes 0, 63 | 64, 255 | 256 of cmp_track_kernel are completed, each with its three bad
    candidates rejected beside the admitted one, and their rewritten slots are THE NaN, +inf or finite as
    nonfinite_fixtures.bad_slot_class says.  wave: the 64 tracks of the middle wave are completed, each beside one rejected bad
    candidate: a whole wave of such tracks goes through wave_add_counters, and all eight counters equal the twin's.  Then the cure:
    the true keypoints uploaded, every formerly bad observation admitted, no NaN left in the session's residuals."""
    for case in nf.drawn(seed=21 + 2 * ["lanes", "wave"].index(place) + sorted(CAMS).index(cam), k=3):
        sc = PLACEMENTS[place](case)[0]
        what = (case[0], place, cam)
        tracks = open_scene(tctx, sc)
        robust_session(tctx, host, sc, tracks, CAMS[cam], 8, what)
        (st, pts, res, mask, tr, before, done, untouched), cure = planted_and_cured(tctx, host, sc, tracks, CAMS[cam], what, case)
        badt = sc.bad_tracks()
        n_bad = len(nf.BAD_AT) if place == "lanes" else 1
        assert np.array_equal(np.nonzero(done)[0], badt) and len(badt) == (len(nf.LANES) if place == "lanes" else 64), (what, tr[badt])
        assert np.all(tr["candidates"][badt] - tr["admitted"][badt] >= n_bad) and np.all(tr["admitted"][badt] >= 1), (what, tr[badt])
        assert st["rejected_by_error"] >= n_bad * len(badt) and st["completed"] >= len(nf.planted_tracks(sc)), (what, st)
        assert cure[0]["admitted"] == n_bad * len(badt) == int(sc.bad.sum()) and not np.isnan(cure[2]).any(), (what, cure[0])
        tctx.tracks_end()


def test_the_clean_neighbours(tctx, host):
    """In the lane placement every clean track's record, residuals and inlier bytes equal, byte for byte, those of the same job
    without any bad value: a poisoned lane leaks through no shuffle, ballot or shared list.  Through the triangulations, the point
    refinements, the extension by the NEW images under their true poses and the filter under FILTER_MIX, whose nine counters' wave
    reduction is the only exchange between lanes (the registration and the pose refinement fit over all tracks of an image: there a
    bad observation changes its clean neighbours by definition)."""
    def run(sc, case):
        tracks = open_scene(tctx, sc)
        first, new = sc.some(nf.OLD), sc.some(nf.NEW)
        out = [triangulated(tctx, host, sc, tracks, first, nf.CAM, False, "plain")[1:]]
        out.append(points_refined(tctx, host, sc, tracks, nf.CAM, "refine0", finite_costs=False)[1:])
        out.append(triangulated(tctx, host, sc, tracks, first, nf.CAM, True, "robust")[1:] + (tctx.point_inliers(),))
        out.append(points_refined(tctx, host, sc, tracks, nf.CAM, "refine1")[1:])
        out.append(extended(tctx, host, sc, tracks, new, 8, nf.CAM, "extend")[1:4])
        out.append(filtered(tctx, host, sc, tracks, nf.CAM, "filter", nf.FILTER_MIX)[1:4])
        tctx.tracks_end()
        return out
    clean_sc = nf.lanes(None)[0]
    clean = run(clean_sc, None)
    o = clean_sc.tracks[0]
    badt = np.zeros(len(clean_sc.lengths), bool)
    badt[clean_sc.bad_tracks()] = True
    per_slot = np.repeat(badt, np.diff(o))
    for case in nf.drawn(seed=5, k=3):
        got = run(nf.lanes(case)[0], case)
        for step, (g, c) in enumerate(zip(got, clean)):
            same_bytes(g[0][~badt], c[0][~badt], (case[0], step))
            for a, b in zip(g[1:], c[1:]):
                same_bytes(a[~per_slot], b[~per_slot], (case[0], step))


def test_tile_elements(tctx, host):
    """tracks of 2, 3, 64, 65 and 130 views with the bad observation at element 0, 63, 64 and last: the 64-observation LDS tiles of
    trr_retry_kernel, enumerated (H 64 covers the 3-view tracks' pairs) and sampled hypotheses; then the point refinement.  Before the
    robust calls the filter runs on the plain session: flt_track_kernel's element loops over the same tracks."""
    for case in nf.drawn(seed=7, k=3):
        sc = nf.elements(case)[0]
        tracks = open_scene(tctx, sc)
        triangulated(tctx, host, sc, tracks, sc.poses, nf.CAM, False, (case[0], "plain"))
        # the filter on the plain session, under its thresholds: the bad element at 0, 63, 64 and last of a fitting set of 2 .. 130
        st, _, _, mask, tr = filtered(tctx, host, sc, tracks, nf.CAM, (case[0], "filter"), creates_bytes=True)
        assert st["eligible"] >= 5 and (nf.non_finite(case) or not mask[sc.bad].all()), (case[0], st)
        for hyp in (8, 64):
            st = tctx.triangulate_tracks(nf.CAM, sc.poses, *nf.THR, robust=True, max_hypotheses=hyp)
            pts, res = tctx.points3d()
            wp, wr, wm, wc = robtw.run(host, tracks, sc.ids, sc.kps, sc.poses, nf.CAM, nf.THR + (hyp,))
            same_bytes(pts, wp, (case[0], hyp))
            same_bytes(res, wr, (case[0], hyp))
            same_bytes(tctx.point_inliers(), wm, (case[0], hyp))
            assert {k: st[k] for k in robtw.ROBUST_KEYS} == wc and st["retried"] >= 11
            only_the_nan(res, sc.bad, (case[0], hyp))
        # (the bad 2-view tracks keep their plain records: under 3e38 and 1e30 their cost is +inf)
        points_refined(tctx, host, sc, tracks, nf.CAM, (case[0], "refine"), finite_costs=False)
        tctx.tracks_end()


def test_replacing_keypoints_after_the_triangulation(tctx, host):
    """upload_keypoints with a bad value after the robust triangulation: the records were made from clean data, the next calls read
    poisoned data -- point refinement, registration, extension, the filter and a point refinement behind it against their twins fed
    the device's state and the NEW keypoints"""
    for case in nf.drawn(seed=9, k=3):
        clean, _, _ = nf.lanes(None)
        sc = nf.lanes(case)[0]
        tracks = open_scene(tctx, clean)
        first = sc.some(nf.OLD)
        triangulated(tctx, host, clean, tracks, first, nf.CAM, True, (case[0], "robust on clean data"))
        assert tctx.point_inliers().sum() == len(nf.OLD) * len(sc.lengths)    # every observation of a posed image supports its point
        for k, i in enumerate(sc.ids):
            tctx.upload_keypoints(int(i), sc.kps[k])
        st, pts, res = points_refined(tctx, host, sc, tracks, nf.CAM, (case[0], "refine"), finite_costs=False)
        _, got = registered(tctx, host, sc, tracks, nf.CAM, (case[0], "register"))
        new = _lib.registered_poses(got[0], sc.some(nf.NEW))
        extended(tctx, host, sc, tracks, new, 8, nf.CAM, (case[0], "extend"))
        # the filter drops the replaced observations that still sit in a fitting set (those of the OLD image: the extension admitted
        # none of the others); behind it every cost sum is finite
        st, _, _, mask, tr = filtered(tctx, host, sc, tracks, nf.CAM, (case[0], "filter"))
        assert not mask[sc.bad].any() and st["dropped_by_depth"] + st["dropped_by_error"] >= len(nf.LANES), (case[0], st)
        points_refined(tctx, host, sc, tracks, nf.CAM, (case[0], "refine after the filter"))
        tctx.tracks_end()


# ---- the verified matching call ----------------------------------------------------------------------------------------------------------
def test_the_verified_matching_call(tctx, host):
    """match_pairs_verified under the models 0, 1, 2, the model selection under both epipolar models, and with the two-view geometry
    on: one small pair list (a general and a planar scene, each pair both ways, and a cross pair) whose images carry the value in
    keypoint rows that the matcher does match -- the second image's descriptors are the first's with 0.4 % of noise, so the raw
    lists are certain and the same whatever the keypoints hold.  Lists, selection records, verification_stats() and the two-view
    records against verify_twin / pose_twin; no bad row in a kept list (but for the pixel 0 -- the denormal and -0.0 -- which an
    epipolar test may keep: tests/test_nonfinite_reference.py::test_verification_twins)."""
    import ctypes as C

    import pose_twin
    import verify_twin as vt
    from test_gpu_verify_homography import load, same, two_view
    vhost, phost = vt.load_host(), pose_twin.load_host()
    vhost.host_fundamental_ransac_ex.argtypes = [vt.FP, vt.FP, C.c_int, C.c_double, C.c_double, C.c_int, C.c_ulonglong, vt.UP]
    scenes = [two_view("general", 300, 40, 30, seed=51), two_view("planar", 300, 40, 30, seed=52)]
    pairs = np.array([(0, 1), (2, 3), (1, 0), (3, 2), (0, 3)], np.int32)
    clean, truth = load(tctx, scenes)
    raw = tctx.match_pairs(pairs)
    assert raw[0][1] - raw[0][0] >= 300 and raw[0][2] - raw[0][1] >= 300
    cam = nf.CAM
    for case in nf.drawn(seed=13, k=4):
        # the value in 10 matched rows of either image of both scenes: every fifteenth match of the scene's own pair
        kps = [k.copy() for k in clean]
        bad = [np.zeros(len(k), bool) for k in kps]
        for p in (0, 1):
            qt = raw[1][raw[0][p]:raw[0][p + 1]]
            for n, m in enumerate(range(3, len(qt), 15)[:20]):
                img = 2 * p + n % 2
                row = int(qt[m, n % 2])
                bad[img][row] = True
                for ax in case[2]:
                    kps[img][row, "xy".index(ax)] = nf.value(case[1])
        for i, k in enumerate(kps):
            tctx.upload_keypoints(i, k)
        assert same(tctx.match_pairs(pairs), raw)
        zero_like = case[0].startswith(("denormal", "minus_zero"))

        def no_bad_row(lists, what):
            if zero_like:
                return
            for p, (i, j) in enumerate(pairs):
                qt = lists[1][lists[0][p]:lists[0][p + 1]]
                assert not bad[i][qt[:, 0]].any() and not bad[j][qt[:, 1]].any(), (case[0], what, p)

        # model 0: the F RANSAC twin, pair by pair
        tctx.set_verification_model(_lib.VERIFY_FUNDAMENTAL)
        got = tctx.match_pairs_verified(pairs)
        keep = []
        for p, (i, j) in enumerate(pairs):
            qt = raw[1][raw[0][p]:raw[0][p + 1]]
            a = np.ascontiguousarray(kps[i][qt[:, 0], :2], np.float32)
            b = np.ascontiguousarray(kps[j][qt[:, 1], :2], np.float32)
            m = np.zeros(max(len(qt), 1), np.uint8)
            k = vhost.host_fundamental_ransac_ex(a.ctypes.data_as(vt.FP), b.ctypes.data_as(vt.FP), len(qt), 3.0, 0.99, 1000, 0x5eed5eed,
                                                 m.ctypes.data_as(vt.UP))
            keep.append(m[:k].astype(bool) if k else np.zeros(len(qt), bool))
        keep = np.concatenate(keep)
        want_off = np.concatenate([[0], np.cumsum([int(keep[raw[0][p]:raw[0][p + 1]].sum()) for p in range(len(pairs))])]).astype(np.int64)
        assert same(got, (want_off, raw[1][keep].reshape(-1, 2), raw[2][keep])), (case[0], "F")
        assert got[0][1] >= 250
        no_bad_row(got, "F")
        # models 1 and 2
        for model in (_lib.VERIFY_ESSENTIAL, _lib.VERIFY_HOMOGRAPHY):
            tctx.set_verification_model(model, cam if model == _lib.VERIFY_ESSENTIAL else None)
            got = tctx.match_pairs_verified(pairs)
            want = vt.run(vhost, raw, pairs, kps, model, cam=cam)
            assert same(got, want["lists"]) and tctx.verification_stats() == want["stats"], (case[0], model, tctx.verification_stats(), want["stats"])
            assert got[0][2] - got[0][1] >= 250 if model == _lib.VERIFY_HOMOGRAPHY else got[0][1] >= 250
            no_bad_row(got, model)
        # the selection under both epipolar models
        for model in (_lib.VERIFY_FUNDAMENTAL, _lib.VERIFY_ESSENTIAL):
            tctx.set_verification_model(model, cam if model == _lib.VERIFY_ESSENTIAL else None)
            tctx.set_model_selection(True)
            got = tctx.match_pairs_verified(pairs)
            rec = tctx.model_selection(len(pairs))
            want = vt.run(vhost, raw, pairs, kps, model, cam=cam, select=True)
            assert same(got, want["lists"]) and all(np.array_equal(x, y) for x, y in zip(rec, want["records"])), (case[0], model, rec)
            assert tctx.verification_stats() == want["stats"]
            assert rec[0][1] == _lib.VERIFY_HOMOGRAPHY and rec[0][0] == model
            no_bad_row(got, ("select", model))
            tctx.set_model_selection(False)
        # the two-view geometry (model 1 is set)
        tctx.set_two_view_geometry(True)
        got = tctx.match_pairs_verified(pairs)
        recs = tctx.two_view_geometry(len(pairs))
        want = pose_twin.run(phost, raw, pairs, kps, cam)
        assert recs.tobytes() == want.tobytes(), (case[0], recs, want)
        assert recs["valid"][0] == 1 and recs["n_kept"][0] == got[0][1]
        assert all(np.all(np.isfinite(recs[k])) for k in ("R", "t", "median_tri_angle", "mean_tri_angle", "mean_residual"))
        no_bad_row(got, "two-view geometry")
        tctx.set_two_view_geometry(False)
