"""Map alignment on the device (msfm_estimate_alignment, msfm_transform_map) against the host twins fed the device's
own state before the call, BYTE FOR BYTE: the msfm_alignment record but estimate_ms, every per-prior record; after transform_map every
integer of the stats, pose_list(), points3d() with records and residuals, point_inliers() and camera() (both unchanged).  Smallest
shapes: ring sessions with 3, 4, 255, 256, 257 priors (one prior, the LDS tile of 256 and its partial), outlier shares 0, one prior and
a quarter, the least-squares route, a failed estimate, 1, 64, 65 and 257 tracks (one lane, one wave, one lane of the second, and more
than one pass of a workgroup), a robust and a refined session, points whose X' overflows, every refused estimate, the registrations around both calls, and the whole
chain."""
import numpy as np
import pytest

import align_ref as ar
import align_twin as atw
import reconstruction_fixtures as rfx
from monocularsfm_amd import _lib
from test_gpu_robust_triangulation import CAM, open_ring, ring_job

pytestmark = pytest.mark.gpu
THRESHOLDS = (2.0, 1.0)   # max_error, min_angle: the ring's neighbours stand 1.2 degrees apart
KEYS = ("status", "n_listed", "n_used", "n_inliers", "hypotheses", "refits")


@pytest.fixture(scope="module")
def actx():
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return atw.load_host()


def similarity(seed, s=40.0, far=1e3):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=3)
    return s, ar.random_rotation(rng), d * far / np.linalg.norm(d)


def priors_of(poses, ids, sim, outliers=(), noise=0.005, seed=5, off=50.0):
    """the centres of `poses` under the similarity, Gaussian noise on every one (sigma = a tenth of the tests' max_error 0.05), the
    `outliers` (positions in ids) moved by `off` along every axis (1700 x max_error)"""
    rng = np.random.default_rng(seed)
    s, Q, d = sim
    pos = {}
    for k, i in enumerate(ids):
        R, t = poses[int(i)]
        pos[int(i)] = s * Q @ (-np.asarray(R).T @ np.asarray(t)) + d + rng.normal(0, noise, 3) + (off if k in outliers else 0.0)
    return pos


def same_estimate(ctx, host, ids, positions, **kw):
    before = rfx.snapshot(ctx)
    lst = ctx.pose_list()
    a, rec = ctx.estimate_alignment(positions, **kw)
    wa, wrec = atw.estimate(host, ids, lst, positions, **kw)
    assert {k: a[k] for k in KEYS} == {k: wa[k] for k in KEYS}, (a, wa)
    for k in ("s", "Q", "d", "rms"):
        assert np.asarray(a[k]).tobytes() == np.asarray(wa[k]).tobytes(), (k, a[k], wa[k])
    assert rec.tobytes() == wrec.tobytes(), np.nonzero(rec != wrec)[0][:8]
    assert a["estimate_ms"] >= 0.0 and rfx.snapshot(ctx) == before, "the estimate is read-only"
    return a, rec


def same_transform(ctx, host, ids, kps, sim, thresholds=THRESHOLDS, cam=CAM):
    tracks, lst, (pts, res) = ctx.tracks(), ctx.pose_list(), ctx.points3d()
    try:
        mask = ctx.point_inliers()
    except _lib.MsfmError:
        mask = None
    camera = ctx.camera()
    st = ctx.transform_map(*sim)
    wl, wp, wr, wc = atw.transform(host, tracks, ids, kps, lst, cam, pts, res, mask, thresholds, *sim)
    assert {k: st[k] for k in atw.COUNT_KEYS} == wc, (st, wc)
    gl, (gp, gr) = ctx.pose_list(), ctx.points3d()
    assert gl[0].tobytes() == wl[0].tobytes() and gl[1].tobytes() == wl[1].tobytes()
    assert gp.tobytes() == wp.tobytes(), np.nonzero(gp != wp)[0][:8]
    assert gr.tobytes() == wr.tobytes(), np.nonzero(gr != wr)[0][:8]
    assert ctx.camera() == camera and st["transform_ms"] >= 0.0
    if mask is not None:
        assert ctx.point_inliers().tobytes() == mask.tobytes()
    return st, gp, (pts, res, lst)


def test_estimate_at_the_tile_edges_and_outlier_shares(actx, host):
    """one session of 257 posed ring cameras; the priors listed: the first m of them"""
    ids, kps, poses, lst = ring_job([257, 257])
    open_ring(actx, ids, kps, lst, 2)
    some = {i: (None if k in (1, 200) else p) for k, (i, p) in enumerate(sorted(poses.items()))}   # two listed images without a pose
    sim = similarity(3)
    for given in (poses, some):
        actx.triangulate_tracks(CAM, given, *THRESHOLDS)
        for m in (3, 4, 255, 256, 257):
            for out in ((), (m - 1,), tuple(range(2, m, 4))):
                if sum(given[int(i)] is not None and k not in out for k, i in enumerate(ids[:m])) < 3:
                    continue
                pos = priors_of(poses, ids[:m], sim, out)
                a, rec = same_estimate(actx, host, ids, pos, max_error=0.05)
                want = np.asarray([(given[int(i)] is not None) and k not in out for k, i in enumerate(ids[:m])])
                assert a["status"] & _lib.ALN_SUCCEEDED and np.array_equal((rec["flags"] & _lib.ALN_INLIER) != 0, want), (m, out, a)
                assert np.array_equal((rec["flags"] & _lib.ALN_USED) != 0, [given[int(i)] is not None for i in ids[:m]])
            a, rec = same_estimate(actx, host, ids, priors_of(poses, ids[:m], sim))                       # least squares
            usable = sum(given[int(i)] is not None for i in ids[:m])
            fitted = _lib.ALN_ATTEMPTED | _lib.ALN_MODEL | _lib.ALN_SUCCEEDED | _lib.ALN_LEAST_SQUARES
            assert a["status"] == (fitted if usable >= 3 else 0) and a["hypotheses"] == 0 and a["n_used"] == usable
        same_estimate(actx, host, ids, priors_of(poses, ids, sim, tuple(range(0, 257, 2))), max_error=0.05, max_hypotheses=4096,
                      confidence=0.999999, min_inliers=10)                                            # more than one round
        a, _ = same_estimate(actx, host, ids, priors_of(poses, ids[:2], sim), max_error=0.05)             # two priors: not attempted
        assert a["status"] == 0 and a["n_used"] == sum(given[int(i)] is not None for i in ids[:2])
    with pytest.raises(_lib.MsfmError) as e:
        actx.estimate_alignment({5: (0, 0, 0)})                                                       # 5 is not declared
    assert e.value.code == _lib.E_INVALID
    actx.tracks_end()


def test_a_failed_estimate_leaves_the_session_as_it_was(actx, host):
    """collinear centres: every sample and the fit of all are invalid"""
    ids, kps, poses, lst = ring_job([6, 6, 6])
    open_ring(actx, ids, kps, lst, 3)
    line = {int(i): (np.eye(3), np.asarray([-0.3 * k, 0.0, 6.5])) for k, i in enumerate(ids)}
    actx.triangulate_tracks(CAM, line, *THRESHOLDS)
    pos = priors_of(line, ids, similarity(4))
    for kw in (dict(max_error=0.05), {}):
        a, rec = same_estimate(actx, host, ids, pos, **kw)
        assert a["status"] & ~_lib.ALN_LEAST_SQUARES == _lib.ALN_ATTEMPTED and a["s"] == 0.0 and not a["Q"].any() and np.all(rec["error"] == -1.0)
        before = rfx.snapshot(actx)
        assert actx.align(pos, **kw)[2] is None and rfx.snapshot(actx) == before
    actx.tracks_end()


@pytest.mark.parametrize("T", [1, 64, 65, 257])
def test_transform_over_track_counts(actx, host, T):
    ids, kps, poses, lst = ring_job([5] * T, rows=max(T, 2))
    open_ring(actx, ids, kps, lst, max(T, 2))
    actx.triangulate_tracks(CAM, poses, *THRESHOLDS)
    st, gp, (pts, res, old) = same_transform(actx, host, ids, kps, (1.0, np.eye(3), np.zeros(3)))          # the identity
    now = actx.pose_list()[1]
    assert gp["X"].tobytes() == pts["X"].tobytes() and all(np.array_equal(now[k], old[1][k]) for k in ("valid", "R", "t"))   # (-0.0 == 0.0)
    assert np.array_equal(gp["status"], pts["status"] | _lib.TRI_ALIGNED) and st["points_transformed"] == T
    sim = similarity(T)
    st, gp, _ = same_transform(actx, host, ids, kps, sim)
    assert st["points_lost"] == st["points_gained"] == 0 and st["succeeded"] == T and st["poses_transformed"] == 5 and _lib.aligned(gp).all()
    a, rec = same_estimate(actx, host, ids, priors_of(poses, ids, similarity(9)), max_error=0.05)       # a transformed session aligns
    assert a["status"] & _lib.ALN_SUCCEEDED and abs(a["s"] - 1.0) < 1e-3
    same_transform(actx, host, ids, kps, (1e300, sim[1], np.zeros(3)))                                 # huge: finite arithmetic all the way
    for bad in ((0.0, np.eye(3), np.zeros(3)), (1.0, np.diag([1.0, 1.0, -1.0]), np.zeros(3)), (1.0, 1.001 * np.eye(3), np.zeros(3)),
                (1.0, np.eye(3), (np.inf, 0, 0))):
        before = rfx.snapshot(actx)
        with pytest.raises(_lib.MsfmError) as e:
            actx.transform_map(*bad)
        assert e.value.code == _lib.E_INVALID and rfx.snapshot(actx) == before
    actx.tracks_end()


def near_origin(poses, ids):
    """the same cameras with the world's origin moved to the first camera's centre: X - C0 for every point, t + R C0 for every pose.
    No keypoint changes.  The translations become small (the cameras stand 0.14 apart) and the points stay 6.5 away, so that s t is
    finite where s X is not."""
    R0, t0 = poses[int(ids[0])]
    C0 = -np.asarray(R0).T @ np.asarray(t0)
    return {i: (R, np.asarray(t) + np.asarray(R) @ C0) for i, (R, t) in poses.items()}


def test_points_that_overflow_become_the_removed_record(actx, host):
    """s = 1e308 on a session whose translations are below 1 and whose points lie 6.5 away: every new pose is finite, every X' is not"""
    T = 65
    ids, kps, poses, lst = ring_job([5] * T)
    open_ring(actx, ids, kps, lst, T)
    near = near_origin(poses, ids)
    assert max(np.abs(t).max() for _, t in near.values()) < 1.0
    st = actx.triangulate_tracks(CAM, near, *THRESHOLDS)
    assert st["succeeded"] == T and np.abs(actx.points3d()[0]["X"]).max(1).min() > 2.0
    tracks = actx.tracks()
    st, gp, (pts, res, old) = same_transform(actx, host, ids, kps, (1e308, np.eye(3), np.zeros(3)))
    assert st["points_transformed"] == st["points_lost"] == T and st["succeeded"] == 0 and st["poses_transformed"] == 5
    assert np.all(gp["status"] == _lib.TRI_ATTEMPTED | _lib.TRI_ALIGNED) and not gp["X"].any() and not gp["n_views"].any()
    assert not gp["mean_residual"].any() and not gp["tri_angle"].any() and np.all(actx.points3d()[1] == -1.0)
    assert np.isfinite(actx.pose_list()[1]["t"]).all()
    actx.tracks_end()


def test_every_refused_estimate_leaves_the_session_as_it_was(actx):
    """the library's own list of MSFM_E_INVALID (the twin's return codes are separate code)"""
    import ctypes as C
    ids, kps, poses, lst = ring_job([5, 5])
    open_ring(actx, ids, kps, lst, 2)
    actx.triangulate_tracks(CAM, poses, *THRESHOLDS)
    pos = priors_of(poses, ids, similarity(6))
    before = rfx.snapshot(actx)
    for kw, args in ((dict(max_error=0.05, max_hypotheses=4097), pos), (dict(max_error=0.05, max_hypotheses=-1), pos),
                     (dict(max_error=0.0), pos), (dict(max_error=-1.0), pos), (dict(max_error=np.inf), pos), (dict(max_error=np.nan), pos),
                     (dict(max_error=0.05, confidence=1.0), pos), (dict(max_error=0.05, confidence=0.0), pos), (dict(confidence=np.nan), pos),
                     ({}, {**pos, int(ids[3]): (np.nan, 0.0, 0.0)}), (dict(max_error=0.05), {**pos, int(ids[1]): (0.0, np.inf, 0.0)}),
                     ({}, {**pos, 2: (0.0, 0.0, 0.0)}), ({}, {**pos, 10001: (0.0, 0.0, 0.0)})):
        with pytest.raises(_lib.MsfmError) as e:
            actx.estimate_alignment(args, **kw)
        assert e.value.code == _lib.E_INVALID and rfx.snapshot(actx) == before, (kw, sorted(args))
    # the raw call: an id given twice, a negative count, a list without positions, no record to fill
    twice = np.asarray([ids[0], ids[1], ids[0]], np.int32)
    xyz = np.zeros((3, 3))
    out = _lib.Alignment()
    dp = xyz.ctypes.data_as(C.POINTER(C.c_double))
    call = actx._L.msfm_estimate_alignment
    assert call(actx._h, _lib._ip(twice), dp, 3, None, C.byref(out), None) == _lib.E_INVALID
    assert call(actx._h, _lib._ip(twice), dp, -1, None, C.byref(out), None) == _lib.E_INVALID
    assert call(actx._h, _lib._ip(twice), None, 2, None, C.byref(out), None) == _lib.E_INVALID
    assert call(actx._h, _lib._ip(twice), dp, 2, None, None, None) == _lib.E_INVALID
    assert actx._L.msfm_transform_map(actx._h, None, None) == _lib.E_INVALID and rfx.snapshot(actx) == before
    assert call(actx._h, _lib._ip(twice), dp, 2, None, C.byref(out), None) == 0 and out.n_used == 2 and out.status == 0   # (and a good one)
    actx.tracks_end()
    with pytest.raises(_lib.MsfmError) as e:                             # no session: MSFM_E_STATE, for both calls
        actx.estimate_alignment(pos)
    assert e.value.code == _lib.E_STATE
    with pytest.raises(_lib.MsfmError) as e:
        actx.transform_map(1.0, np.eye(3), np.zeros(3))
    assert e.value.code == _lib.E_STATE


def test_transform_keeps_the_bits_and_the_mask_of_a_robust_and_a_refined_session(actx, host):
    lengths = [2, 3, 5, 7, 7, 12] * 11
    ids, kps, poses, lst = ring_job(lengths, outlier={4: 3, 9: 0, 17: 11})
    open_ring(actx, ids, kps, lst, len(lengths))
    some = {i: (None if k == 5 else p) for k, (i, p) in enumerate(sorted(poses.items()))}
    actx.triangulate_tracks(CAM, some, *THRESHOLDS, robust=True)
    sim = similarity(21)
    st, gp, (pts, _, _) = same_transform(actx, host, ids, kps, sim)
    assert np.array_equal(gp["status"] & _lib.TRI_ROBUST, pts["status"] & _lib.TRI_ROBUST) and (gp["status"] & _lib.TRI_ROBUST).any()
    assert st["poses_transformed"] == len(ids) - 1
    actx.refine_points()
    actx.refine_poses(min_observations=6)
    st, gp, (pts, _, _) = same_transform(actx, host, ids, kps, similarity(22, s=0.025))
    kept = _lib.TRI_ROBUST | _lib.TRI_REFINED | _lib.TRI_REPOSED
    assert np.array_equal(gp["status"] & kept, pts["status"] & kept) and (gp["status"] & _lib.TRI_REPOSED).any()
    assert not (pts["status"] & _lib.TRI_ALIGNED).all(), "refine_points / refine_poses cleared ALIGNED on what they rewrote"
    actx.tracks_end()


def test_registrations_around_the_two_calls(actx, host):
    lengths = [8] * 40
    ids, kps, poses, lst = ring_job(lengths)
    open_ring(actx, ids, kps, lst, len(lengths))
    first = {i: p for k, (i, p) in enumerate(sorted(poses.items())) if k < 6}
    actx.triangulate_tracks(CAM, first, *THRESHOLDS)
    actx.register_images(CAM, [int(ids[6]), int(ids[7])])
    same_estimate(actx, host, ids, priors_of(poses, ids[:6], similarity(2)), max_error=0.05)
    rec = actx.registrations()[0]
    assert _lib.registered(rec).all()                                   # the estimate left them fetchable
    same_transform(actx, host, ids, kps, similarity(2))
    with pytest.raises(_lib.MsfmError) as e:
        actx.registrations()
    assert e.value.code == _lib.E_STATE
    actx.tracks_end()


def test_the_chain_on_the_device_equals_the_twin_chain(actx):
    """section 26's chain for seed 77 on both sides: ten increments, align to priors with three gross outliers, the rest of the loop"""
    cap = rfx.variant("s77")
    sim = similarity(77)
    order = sorted(cap["poses"])
    pos = priors_of(cap["poses"], order, sim, outliers=(2, 9, 17), noise=0.0, off=200.0)
    got = []
    for ctx in (actx, atw.AlignTwinContext()):
        _, records, _ = rfx.open_session(ctx, cap)
        ctx.initialize(cap["cam"], rfx.two_view_dict(cap, records), min_points=rfx.MIN_POINTS)
        steps = rfx.increments(ctx, cap["cam"])
        for _ in range(10):
            next(steps)
        a, rec, st = ctx.align(pos, max_error=5.0)
        assert a["status"] & _lib.ALN_SUCCEEDED and st is not None
        mid = (rfx.snapshot(ctx), {k: a[k] for k in KEYS}, a["Q"].tobytes(), a["d"].tobytes(), a["s"], a["rms"], rec.tobytes(),
               {k: st[k] for k in atw.COUNT_KEYS})
        for _ in steps:
            pass
        got.append((mid, rfx.snapshot(ctx), sorted(ctx.poses())))
        ctx.tracks_end()
    assert got[0][0] == got[1][0], "after align"
    assert got[0][1] == got[1][1] and got[0][2] == got[1][2] == order, "at the end"
