"""Point refinement on the device (msfm_refine_points, csrc/msfm_refine.hip.h) against the host twin (csrc/msfm_refine.h, RefinePoints,
through tests/refine_points_twin.py): records, residuals and the integer counters BYTE FOR BYTE; the two cost sums (information only:
the device adds per wave, the twin in track order) to 1e-9 relative.  The twin is fed the device's own triangulation outputs, which
tests/test_gpu_triangulation.py and tests/test_gpu_robust_triangulation.py hold equal to the triangulation twins.  Where a test is
about a route of the LM loop or the verdict, the twin's trace is asserted next to the byte comparison: the routes are found on the CPU
by tests/refine_points_fixtures.routes and placed at the lanes named in the test.  The twin itself is checked against the independent
numpy reference in tests/test_refine_points_reference.py."""
import numpy as np
import pytest

import refine_points_fixtures as rfx
import refine_points_twin as rtw
import registration_twin as regtw
import tracks_fixtures as fx
from monocularsfm_amd import _lib, synth
from test_gpu_robust_triangulation import open_ring, ring_job, second_pass_job

pytestmark = pytest.mark.gpu
CAM = rfx.CAM
CAM_D = CAM + (-0.1, 0.02, 1e-3, -5e-4)


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return rtw.load_host()


def refine_same(ctx, host, ids, kps, poses, tracks, cam=CAM, thresholds=(2.0, 1.5), params=rtw.DEFAULTS, robust=False, trace=False):
    """one msfm_refine_points on the session's current records against the twin run from those records -> (stats, points, residuals[,
    the twin's trace])"""
    p0, r0 = ctx.points3d()
    m0 = ctx.point_inliers() if robust else None
    st = ctx.refine_points(*params)
    pts, res = ctx.points3d()
    want = rtw.run(host, tracks, ids, kps, poses, cam, p0, r0, m0, thresholds, params, trace=trace)
    wp, wr, wc = want[:3]
    assert pts.tobytes() == wp.tobytes(), np.nonzero(pts != wp)[0][:8]
    assert res.tobytes() == wr.tobytes(), np.nonzero(res != wr)[0][:8]
    assert {k: st[k] for k in rtw.COUNT_KEYS} == {k: wc[k] for k in rtw.COUNT_KEYS}, (st, wc)
    for k in rtw.COST_KEYS:
        assert abs(st[k] - wc[k]) <= 1e-9 * max(abs(wc[k]), 1e-300), (k, st[k], wc[k])
    assert st["refine_ms"] >= st["prepare_ms"] >= 0.0
    assert np.array_equal(pts["n_views"], p0["n_views"])
    assert np.all(_lib.succeeded(pts) | ~_lib.succeeded(p0))                                   # the succeeded set only grows
    same = ~_lib.refined(pts) | (_lib.refined(p0) & (pts["X"] == p0["X"]).all(1))              # records that were not rewritten ...
    assert pts[same].tobytes() == p0[same].tobytes()                                           # ... are bit for bit what they were
    if robust:
        assert ctx.point_inliers().tobytes() == m0.tobytes()
    return (st, pts, res) + tuple(want[3:])


def test_routes_at_the_wave_and_block_edges(tctx, host):
    """T = 257 with one CPU-found route each at lanes 0, 63 | 64 and 255 | 256 (a rejected step followed by an accepted one; a stop at
    the lambda ceiling by depth-rejected steps; dropped for ERROR_OK; gained ERROR_OK; dropped for ANGLE_OK), then the prefixes T = 256,
    255 and 1; max_iters 0 (nothing changes), 1, 2 and 10; a repeated call."""
    ids, kps, poses, lengths = rfx.routes_job()
    found = rfx.routes(host, ids, kps, poses, lengths)[6]
    place = {0: "rejected_then_accepted", 63: "ceiling", 64: "dropped_error_ok", 255: "gained_error_ok", 256: "dropped_angle_ok"}
    found["ceiling"] = np.intersect1d(found["ceiling"], found["depth_rejected"])
    special = {}
    for lane, r in place.items():
        special[lane] = next(int(t) for t in found[r] if int(t) not in special.values())
    rest = [t for t in range(len(lengths)) if t not in special.values()]
    order = [special[j] if j in special else rest.pop(0) for j in range(257)]
    kps, lengths = rfx.reordered(kps, lengths, order)
    for T in (257, 256, 255, 1):
        n = lengths[:T]
        open_ring(tctx, ids[:max(n)], kps[:max(n)], rfx.ring_list(n, ids), 2000)
        tracks = tctx.tracks()
        assert np.array_equal(tracks[0], rfx.tracks_of(n, ids)[0])
        some = {int(i): poses[int(i)] for i in ids[:max(n)]}
        for mi in (0, 1, 2, 10):
            tctx.triangulate_tracks(CAM, some, *rfx.ROUTE_THRESHOLDS)
            before = [a.tobytes() for a in tctx.points3d()]
            st, pts, res, tr = refine_same(tctx, host, ids[:max(n)], kps[:max(n)], some, tracks, thresholds=rfx.ROUTE_THRESHOLDS,
                                           params=(mi, 1e-4), trace=True)
            if mi == 0:
                assert [pts.tobytes(), res.tobytes()] == before and st["refined"] == 0 and st["iterations"] == 0 and st["eligible"] == T
                assert st["cost_before"] == st["cost_after"]
            if mi in (1, 2):
                assert np.all(tr["steps"] <= mi) and (T == 1 or (tr["stop"] == rtw.STOP_MAX_ITERS).any())
        if T >= 257:   # (max_iters 10 ran last) the routes, where they were placed
            assert tr[0]["accepted_after_rejected"] > 0 and tr[0]["verdict"] == 0
            assert tr[63]["stop"] == rtw.STOP_CEILING and tr[63]["depth_rejected"] > 0
            assert tr[64]["verdict"] == rfx.ERROR_OK and tr[256]["verdict"] == rfx.ANGLE_OK
            assert (pts[255]["status"] & 4) and st["gained_error_ok"] > 0 and st["rejected_by_verdict"] >= 2
        st2, pts2, _, tr2 = refine_same(tctx, host, ids[:max(n)], kps[:max(n)], some, tracks, thresholds=rfx.ROUTE_THRESHOLDS,
                                        params=(10, 1e-4), trace=True)                       # a second call: from the refined records
        assert st2["cost_after"] <= st2["cost_before"] == pytest.approx(st["cost_after"], rel=1e-9)
        tctx.tracks_end()


def test_unposed_inconsistent_unattempted_and_a_long_track(tctx, host):
    """One track of 130 views among short ones; every seventh image unposed (unposed elements interleaved among the used
    observations); min_views 3 leaves the 2-view tracks unattempted; a second keypoint of image 0 joins two tracks into an
    inconsistent one.  The bytes of everything that is not eligible are untouched and the per-observation array stays aligned."""
    lengths = [2, 3, 5, 130, 7, 2, 12, 3, 64, 65] * 3
    ids, kps, poses, lst = ring_job(lengths, noise_px=1.0)
    lst = (np.r_[lst[0], [[ids[0], ids[1]]]].astype(np.int32), np.r_[lst[1], lst[1][-1] + 1], np.r_[lst[2], [[4, 6]]].astype(np.int32))
    open_ring(tctx, ids, kps, lst, len(lengths))
    ts = tctx.tracks_finish(keep_inconsistent=True)
    tracks = tctx.tracks()
    assert ts["longest_track"] == 130 and ts["tracks_kept"] == len(lengths) - 1 and int((tracks[3] == 0).sum()) == 1
    some = {i: (None if k % 7 == 3 else p) for k, (i, p) in enumerate(sorted(poses.items()))}
    for cam, thr in ((CAM, (2.0, 1.5)), (CAM_D, (1.0, 4.0))):
        tctx.triangulate_tracks(cam, some, *thr, 3)
        p0, r0 = tctx.points3d()
        st, pts, res = refine_same(tctx, host, ids, kps, some, tracks, cam=cam, thresholds=thr)
        idle = (p0["status"] & 3) != 3
        assert idle.sum() >= 7 and st["eligible"] == len(pts) - idle.sum() and st["refined"] > 0
        assert pts[idle].tobytes() == p0[idle].tobytes()
        skipped = np.repeat(idle, np.diff(tracks[0])) | (r0 < 0)
        assert res[skipped].tobytes() == r0[skipped].tobytes()
    tctx.tracks_end()


def test_after_the_robust_call_on_the_corrupted_scene_job(tctx, host):
    """Rejected observations get new errors, stay out of the sums, and the inlier bytes are what they were; tracks, track ids and
    match lists are byte-equal before and after; register_images after the refine call equals the registration twin fed the refined
    points; fetch_registrations between the two returns MSFM_E_STATE."""
    ids, imgs, kps, pairs = fx.scene_job()
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), imgs[k])
        tctx.upload_keypoints(int(i), kps[k])
    poses = {int(i): (c[0], c[1]) for i, c in zip(ids, synth.scene_cameras(len(ids), seed=77))}
    tctx.set_verification_model(_lib.VERIFY_ESSENTIAL, CAM)
    tctx.tracks_begin(ids)
    offs, qt, dist = tctx.match_pairs_verified(pairs)
    tctx.tracks_finish()
    tracks = tctx.tracks()
    o = tracks[0]
    chosen = [(t, (0, int(o[t + 1] - o[t]) // 2, int(o[t + 1] - o[t]) - 1)[n % 3]) for n, t in enumerate(range(0, len(o) - 1, 5))]
    bad, _ = synth.corrupt_observations(ids, kps, tracks, chosen)
    for k, i in enumerate(ids):
        tctx.upload_keypoints(int(i), bad[k])
    tid = {int(i): tctx.track_ids(int(i)).tobytes() for i in ids}
    known = {i: p for i, p in poses.items() if i != int(ids[5])}
    tctx.triangulate_tracks(CAM, known, robust=True)
    p0, r0 = tctx.points3d()
    mask = tctx.point_inliers()
    tctx.register_images(CAM, [int(ids[5])])
    tctx.registrations()
    st, pts, res = refine_same(tctx, host, ids, bad, known, tracks, robust=True)
    with pytest.raises(_lib.MsfmError) as e:
        tctx.registrations()
    assert e.value.code == _lib.E_STATE
    rejected = (mask == 0) & (r0 >= 0)
    moved = np.repeat(_lib.refined(pts), np.diff(o))
    assert st["refined"] > 100 and (rejected & moved).sum() > 10 and np.all(res[rejected & moved] != r0[rejected & moved])
    assert np.all(pts["status"] & _lib.TRI_ROBUST == p0["status"] & _lib.TRI_ROBUST)
    for t in np.nonzero(_lib.refined(pts) & ((p0["status"] & _lib.TRI_ROBUST) != 0))[0][:50]:   # mean_residual: the inliers alone
        e_ = res[o[t]:o[t + 1]][mask[o[t]:o[t + 1]] == 1]
        assert abs(pts[t]["mean_residual"] - e_.mean()) < 1e-9
    assert [a.tobytes() for a in tctx.tracks()] == [a.tobytes() for a in tracks]
    assert {int(i): tctx.track_ids(int(i)).tobytes() for i in ids} == tid
    vq, vd = tctx._view()
    assert vq.tobytes() == qt.tobytes() and vd.tobytes() == dist.tobytes()
    rst = tctx.register_images(CAM, [int(ids[5])])
    got = tctx.registrations()
    want = regtw.run(host_reg(), tracks, pts, [int(ids[5])], {int(i): b for i, b in zip(ids, bad)}, CAM)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and rst["succeeded"] == 1
    tctx.tracks_end()


_REG = []


def host_reg():
    if not _REG:
        _REG.append(regtw.load_host())
    return _REG[0]


def test_second_grid_stride_pass(tctx, host):
    """ref_track_kernel's grid holds 8 x CUs x 256 lanes: with 8192 tracks more its first 32 workgroups run a second pass; the
    per-observation kernel runs its second pass too (three observations per track).  After the robust call, default parameters."""
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
    tctx.triangulate_tracks(CAM, poses, robust=True)
    st, pts, _ = refine_same(tctx, host, ids, kps, poses, tracks, robust=True)
    assert st["eligible"] > T // 2 and _lib.refined(pts)[T - 8192:].any()
    print("second pass: T %d, refine_ms %.3f of which prepare %.3f" % (T, st["refine_ms"], st["prepare_ms"]))
    tctx.tracks_end()


def test_errors_and_state(tctx):
    def code(fn, *a, **k):
        with pytest.raises(_lib.MsfmError) as e:
            fn(*a, **k)
        return e.value.code

    E = _lib
    ids, kps, poses, lst = ring_job([4] * 6)
    assert code(tctx.refine_points) == E.E_STATE                                             # no session
    open_ring(tctx, ids, kps, lst, 6)
    assert code(tctx.refine_points) == E.E_STATE                                             # finished, not triangulated
    tctx.triangulate_tracks(CAM, poses)
    for kw in (dict(max_iters=-1), dict(max_iters=101), dict(step_tol=-1e-3), dict(step_tol=float("nan")), dict(step_tol=float("inf"))):
        assert code(tctx.refine_points, **kw) == E.E_INVALID
    assert tctx._L.msfm_refine_points(tctx._h, None, None) == E.OK                           # NULL params and stats
    st = tctx.refine_points(max_iters=100, step_tol=0.0)
    assert st["eligible"] == 6
    tctx.register_images(CAM, [int(ids[0])], min_inliers=3)
    tctx.registrations()
    tctx.refine_points()
    assert code(tctx.registrations) == E.E_STATE and len(tctx.points3d()[0]) == 6            # registrations gone, points stay
    tctx.tracks_finish()
    assert code(tctx.refine_points) == E.E_STATE                                             # after tracks_finish
    tctx.triangulate_tracks(CAM, poses, robust=True)
    tctx.refine_points()
    assert len(tctx.point_inliers()) == 24                                                   # the inlier bytes stay valid
    tctx.set_limits(max_pairs_per_batch=1)
    gen = tctx.match_pairs_stream([(int(ids[0]), int(ids[1])), (int(ids[1]), int(ids[2]))], max_distance=1e9)
    next(gen)
    assert code(tctx.refine_points) == E.E_STATE                                             # while a series is open
    gen.close()
    tctx.tracks_end()
    assert code(tctx.refine_points) == E.E_STATE
