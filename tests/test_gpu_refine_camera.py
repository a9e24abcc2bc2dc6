"""Camera refinement on the device (msfm_refine_camera, csrc/msfm_refine_camera.hip.h) against the host twin
(csrc/msfm_refine_camera.h, RefineCamera, through tests/refine_camera_twin.py) BYTE FOR BYTE: the camera (msfm_fetch_camera and the
stats' two copies), every integer of the stats, both costs (bit-equal: the summation order is fixed by the data), every point record,
every residual and every inlier byte after the call.  The twin is fed the device's own triangulation outputs, the session's own pose
list and camera.  The twin itself is checked against the independent numpy reference in tests/test_refine_camera_reference.py.

The sessions are hand-built rings (tests/test_gpu_robust_triangulation.ring_job: track j runs through the images 0 .. lengths[j] - 1)
so that O, the number of kept observations, sits where the two levels of the summation change shape, and the eight scenes of
tests/test_refine_camera_reference.py (tests/tracks_fixtures.scene_job's captures, 24 x 600, seeds 77 and 5).  Every session is
triangulated under a camera that is OFF (bad() below: fx, fy 2 %, cx, cy 8 px, k1 0.02, k2 0.005) with max_error 60 px, which keeps every
track of a clean job standing under such a camera."""
import numpy as np
import pytest

import complete_twin as cmtw
import filter_twin as ftw
import refine_camera_twin as ctw
import refine_points_twin as rtw
import refine_poses_fixtures as pfx
import refine_poses_twin as ptw
from monocularsfm_amd import _lib
from test_gpu_robust_triangulation import open_ring, ring_job

pytestmark = pytest.mark.gpu
CAM = pfx.CAM
THR = (60.0, 0.5)   # min_angle: below the 1.0 .. 1.4 degrees two neighbouring ring cameras subtend at a point of the scene
ALL = ctw.FX_FY | ctw.CX_CY | ctw.K1_K2
KEYS = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")


def bad(cam, sign=1.0):
    c = ctw.camera8(cam)
    return (c[0] * (1 + 0.02 * sign), c[1] * (1 - 0.02 * sign), c[2] + 8.0 * sign, c[3] - 8.0 * sign, c[4] + 0.02 * sign, c[5] - 0.005 * sign,
            c[6], c[7])


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return ctw.load_host()


def cam_tuple(d):
    return tuple(d[k] for k in KEYS)


def cam_bytes(c):
    return np.asarray(c, np.float64).tobytes()


def state(ctx, robust):
    pts, res = ctx.points3d()
    return pts, res, (ctx.point_inliers() if robust else None), ctx.pose_list(), cam_tuple(ctx.camera())


def camera_same(ctx, host, ids, kps, tracks, mask=ctw.FX_FY, params=ctw.DEFAULTS, thresholds=THR, robust=False):
    """one msfm_refine_camera on the session's current state against the twin run from that state -> (stats, points, residuals, the
    twin's trace)"""
    p0, r0, m0, l0, c0 = state(ctx, robust)
    st = ctx.refine_camera(mask, *params)
    pts, res, m1, l1, c1 = state(ctx, robust)
    wp, wr, wc, wn, tr = ctw.run(host, tracks, ids, kps, l0, c0, p0, r0, m0, thresholds, params, mask, trace=True)
    assert cam_bytes(c1) == cam_bytes(wc), (c1, wc)
    assert cam_bytes(cam_tuple(st["camera_before"])) == cam_bytes(c0) and cam_bytes(cam_tuple(st["camera_after"])) == cam_bytes(c1)
    assert {k: st[k] for k in ctw.COUNT_KEYS} == {k: wn[k] for k in ctw.COUNT_KEYS}, (st, wn)
    assert all(np.float64(st[k]).tobytes() == np.float64(wn[k]).tobytes() for k in ctw.COST_KEYS), (st, wn)
    assert pts.tobytes() == wp.tobytes(), np.nonzero(pts != wp)[0][:8]
    assert res.tobytes() == wr.tobytes(), np.nonzero(res != wr)[0][:8]
    assert st["refine_ms"] >= 0.0 and l1[1].tobytes() == l0[1].tobytes()                      # no pose moves
    if robust:
        assert m1.tobytes() == m0.tobytes()                                                  # the inlier bytes never change
    assert np.array_equal(pts["X"], p0["X"]) and np.array_equal(pts["n_views"], p0["n_views"])
    keep = 32 | 64 | 128 | 256 | 512 | 1024
    assert np.array_equal(pts["status"] & keep, p0["status"] & keep)
    eligible = (p0["status"] & 3) == 3
    if st["refined"]:
        assert st["accepted_steps"] > 0 and st["inliers_after"] >= st["inliers_before"] and st["cost_after"] < st["cost_before"]
        assert np.array_equal(_lib.recalibrated(pts), eligible | _lib.recalibrated(p0)) and st["points_recalibrated"] == eligible.sum()
        assert c1[6:] == c0[6:] and c1 != c0                                                  # p1, p2 never move
    else:
        assert cam_bytes(c1) == cam_bytes(c0) and pts.tobytes() == p0.tobytes() and res.tobytes() == r0.tobytes()
        assert st["points_recalibrated"] == 0 and st["cost_after"] == st["cost_before"]
    ok0, ok1 = _lib.succeeded(p0), _lib.succeeded(pts)
    assert st["points_lost"] == (ok0 & ~ok1).sum() and st["points_gained"] == (~ok0 & ok1).sum()
    return st, pts, res, tr


def opened(ctx, lengths, **kw):
    ids, kps, poses, lst = ring_job(lengths, **kw)
    open_ring(ctx, ids, kps, lst, len(lengths))
    tracks = ctx.tracks()
    assert tracks[0][-1] == sum(lengths)
    return ids, kps, poses, tracks


def lengths_for(O, longest):
    """track lengths out of 2 .. longest that add up to O"""
    n, rem = divmod(O, longest)
    out = [longest] * n
    if rem == 1:
        out[-1] = longest - 1
        rem = 2
    return out + ([rem] if rem else [])


# ---- the CPU cases at scene_job size ---------------------------------------------------------------------------------------------------
CAM_D = CAM + (-0.1, 0.02, 1e-3, -5e-4)
CAM_A = (2500.0, 2380.0, 1536.0, 1152.0)   # fx != fy
SCENES = [("plain", 77, CAM), ("plain", 5, CAM), ("robust", 77, CAM), ("robust", 5, CAM), ("plain", 77, CAM_D), ("plain", 5, CAM_D),
          ("plain", 77, CAM_A), ("plain", 5, CAM_A)]
MASKS = [ctw.FX_FY, ctw.F, ctw.CX_CY, ctw.K1_K2, ALL, ctw.F | ctw.K1_K2]


def open_capture(ctx, kind, seed, cam):
    """tests/test_refine_camera_reference.py's scene (tests/tracks_fixtures.scene_job's capture of `seed`, 0.3 px of noise, under `cam`;
    "robust": with corrupted observations) folded through tracks_add -> the capture dict"""
    import tracks_fixtures as fx
    from test_robust_triangulation_reference import corrupted
    from test_triangulation_reference import capture
    c = capture(seed, noise_px=0.3, cam=cam) if kind == "plain" else corrupted(seed, cam)
    rng = np.random.default_rng(2)
    for i in c["ids"]:
        ctx.upload_image(int(i), rng.integers(0, 256, (len(c["kps"][int(i)]), 128), dtype=np.uint8))
        ctx.upload_keypoints(int(i), c["kps"][int(i)])
    offs, img, idx = c["tracks"][0], c["tracks"][1], c["tracks"][2]
    edges = {}
    for t in range(len(offs) - 1):                      # a chain through every track's elements
        for e in range(offs[t], offs[t + 1] - 1):
            edges.setdefault((int(img[e]), int(img[e + 1])), []).append((int(idx[e]), int(idx[e + 1])))
    ctx.tracks_begin(c["ids"], min_pair_matches=1)
    ctx.tracks_add(*fx.csr(sorted(edges.items())))
    ctx.tracks_finish()
    assert all(a.tobytes() == np.asarray(b).astype(a.dtype).tobytes() for a, b in zip(ctx.tracks()[:3], c["tracks"][:3]))
    return c


@pytest.mark.parametrize("kind,seed,cam", SCENES)
def test_capture_every_mask_and_iteration_limit(tctx, host, kind, seed, cam):
    """The eight scenes of tests/test_refine_camera_reference.py -- the captures of seeds 77 and 5, plain, robust (corrupted
    observations), under the distorted CAM_D and under CAM_A with fx != fy -- each with every one of the six masks at max_iters 10, 1
    and 2, and a repeated call from the camera that stands.  (The session's camera is the one its triangulation was given, so here
    the records are made under the camera that is off.)"""
    robust = kind == "robust"
    c = open_capture(tctx, kind, seed, cam)
    tracks = tctx.tracks()
    stood = 0
    for mask in MASKS:
        for mi in (10, 1, 2):
            tctx.triangulate_tracks(bad(cam), c["poses"], *THR, robust=robust)
            st, pts, res, tr = camera_same(tctx, host, c["ids"], c["kps"], tracks, mask, (mi, 1e-6, 100), robust=robust)
            assert st["observations"] > 5000 and st["iterations"] <= mi and tr["steps"] == st["iterations"]
            assert st["accepted_steps"] > 0 and st["stop"] in (ctw.STOP_STEP, ctw.STOP_MAX_ITERS) and (mi > 1 or st["stop"] == ctw.STOP_MAX_ITERS)
            stood += st["refined"]
            if mask == ALL and mi == 10:
                assert st["refined"] == 1
                st2, *_ = camera_same(tctx, host, c["ids"], c["kps"], tracks, mask, (mi, 1e-6, 100), robust=robust)  # a repeated call
                assert np.float64(st2["cost_before"]).tobytes() == np.float64(st["cost_after"]).tobytes()
    assert stood == 18                                       # (found on the CPU twin: every one of the calls stands)
    tctx.tracks_end()


def test_start_without_distortion_takes_undistorts_shortcut_once(tctx, host):
    """k1 = k2 = p1 = p2 = 0 at the start with K1_K2 in the mask: the first evaluation takes undistort's all-zero shortcut, every later
    one the 40 steps."""
    ids, kps, poses, tracks = opened(tctx, [12] * 300)
    start = (2550.0, 2450.0, 1544.0, 1144.0)
    tctx.triangulate_tracks(start, poses, *THR)
    st, *_ = camera_same(tctx, host, ids, kps, tracks, ALL, (10, 1e-6, 100))
    assert st["refined"] == 1 and st["camera_before"]["k1"] == 0.0 == st["camera_before"]["k2"] and st["camera_after"]["k1"] != 0.0
    tctx.tracks_end()


# ---- the edges of the two summation levels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O", [255, 256, 257, 511, 512, 513, 769])
def test_level_one_edges(tctx, host, O):
    """O kept observations one short of a chunk, exact and one over (one and two chunks); 257, 513 and 769: the last chunk holds a
    single slot."""
    ids, kps, poses, tracks = opened(tctx, lengths_for(O, 3))
    for mi in (10, 1):
        tctx.triangulate_tracks(bad(CAM), poses, *THR)
        st, *_ = camera_same(tctx, host, ids, kps, tracks, ALL, (mi, 1e-6, 6))
        assert st["observations"] == O and st["accepted_steps"] > 0
    tctx.tracks_end()


@pytest.mark.parametrize("O", [255 * 256, 255 * 256 + 1, 256 * 256, 256 * 256 + 1])
def test_level_two_edges(tctx, host, O):
    """255, 256 and 257 chunks: the strided partials of level 2 with an empty last partial, exactly one chunk each, and a second round
    for partial 0 alone."""
    ids, kps, poses, tracks = opened(tctx, lengths_for(O, 16))
    tctx.triangulate_tracks(bad(CAM), poses, *THR)
    st, *_ = camera_same(tctx, host, ids, kps, tracks, ALL, (3, 1e-6, 100))
    assert st["observations"] == O and st["accepted_steps"] > 0
    tctx.tracks_end()


def test_chunks_that_contribute_nothing(tctx, host):
    """Runs of 600 consecutive slots of tracks that do not stand (one observation 300 px off: no ERROR_OK) at the head, in the middle
    and at the tail: whole chunks of zeros in level 1, zeros among the partials of level 2."""
    T, run = 1200, 200
    dead = list(range(run)) + list(range(500, 500 + run)) + list(range(T - run, T))
    ids, kps, poses, tracks = opened(tctx, [3] * T, moved={j: [(0, 300.0, 0.0)] for j in dead})
    tctx.triangulate_tracks(bad(CAM), poses, *THR)
    p0 = tctx.points3d()[0]
    contributes = np.repeat(_lib.succeeded(p0), np.diff(tracks[0]))
    chunks = np.add.reduceat(contributes.astype(np.int64), np.arange(0, len(contributes), 256))
    assert chunks[0] == 0 and chunks[-1] == 0 and (chunks[4:10] == 0).any() and (chunks > 0).sum() >= 6
    st, *_ = camera_same(tctx, host, ids, kps, tracks, ALL, (10, 1e-6, 100))
    assert st["observations"] == contributes.sum() == 3 * (T - len(dead)) and st["refined"] == 1
    tctx.tracks_end()


def test_more_chunks_than_workgroups(tctx, host):
    """The chunk kernels' grid holds at most 8 x CUs workgroups: with 8 x CUs + 3 chunks the first three workgroups walk to a second
    chunk.  The sums are stored at the chunks' own places: the twin's bits."""
    cus = tctx.device_info()["cu_count"]
    O = 256 * (8 * cus + 2) + 7
    ids, kps, poses, tracks = opened(tctx, lengths_for(O, 32))
    tctx.triangulate_tracks(bad(CAM), poses, *THR)
    st, *_ = camera_same(tctx, host, ids, kps, tracks, ALL, (2, 1e-6, 100))
    assert st["observations"] == O and st["accepted_steps"] == 2
    tctx.tracks_end()
    print("second stride pass: %d CUs, %d observations, %d chunks, refine_ms %.3f" % (cus, O, (O + 255) // 256, st["refine_ms"]))


# ---- what does not stand, and what is not attempted ---------------------------------------------------------------------------------
def test_calls_that_change_nothing(tctx, host):
    """max_iters = 0; fewer than min_observations contributing; a refined camera that does NOT stand (8 px of noise next to a tight
    max_error: the L2 optimum costs a max-norm inlier); one NaN keypoint uploaded after the triangulation (a non-finite starting
    cost): every fetched byte stays."""
    ids, kps, poses, tracks = opened(tctx, [8] * 150, noise_px=8.0, seed=13)
    tctx.triangulate_tracks(bad(CAM), poses, 200.0, 1.0)
    st, *_ = camera_same(tctx, host, ids, kps, tracks, ALL, (0, 1e-6, 100), thresholds=(200.0, 1.0))
    assert (st["stop"], st["iterations"], st["refined"]) == (ctw.STOP_MAX_ITERS, 0, 0) and st["cost_before"] > 0.0
    st, *_ = camera_same(tctx, host, ids, kps, tracks, ALL, (10, 1e-6, 1201), thresholds=(200.0, 1.0))
    assert (st["stop"], st["observations"], st["cost_before"]) == (ctw.STOP_FEW, 1200, 0.0)
    tctx.triangulate_tracks(bad(CAM), poses, 16.0, 1.0)      # (found on the CPU twin: 616 contribute, the refined camera keeps 612)
    st, _, _, tr = camera_same(tctx, host, ids, kps, tracks, ALL, (10, 1e-6, 100), thresholds=(16.0, 1.0))
    assert tr["verdict"] == ctw.LOST_INLIERS and (st["refined"], st["rejected_by_inliers"]) == (0, 1)
    assert st["accepted_steps"] > 0 and st["inliers_after"] < st["inliers_before"] == st["observations"]
    tctx.triangulate_tracks(CAM, poses, 200.0, 1.0)          # the records are made from clean data ...
    kps = [k.copy() for k in kps]
    kps[2][5, 0] = np.float32(np.nan)
    tctx.upload_keypoints(int(ids[2]), kps[2])               # ... and the call reads a NaN in a standing track's fitting set
    st, *_ = camera_same(tctx, host, ids, kps, tracks, ALL, (10, 1e-6, 100), thresholds=(200.0, 1.0))
    assert (st["stop"], st["refined"], st["observations"], st["cost_before"]) == (ctw.STOP_NONFINITE, 0, 1200, 0.0)
    tctx.tracks_end()


def test_errors(tctx):
    ids, kps, poses, lst = ring_job([4] * 40)
    with pytest.raises(_lib.MsfmError) as e:
        tctx.refine_camera()
    assert e.value.code == _lib.E_STATE
    with pytest.raises(_lib.MsfmError) as e:
        tctx.camera()
    assert e.value.code == _lib.E_STATE
    open_ring(tctx, ids, kps, lst, 40)
    for call in (tctx.refine_camera, tctx.camera):
        with pytest.raises(_lib.MsfmError) as e:
            call()
        assert e.value.code == _lib.E_STATE                                                  # no triangulation yet
    tctx.triangulate_tracks(CAM, poses)
    assert cam_tuple(tctx.camera()) == ctw.camera8(CAM)
    for kw in (dict(mask=0), dict(mask=16), dict(mask=("fx_fy", "f")), dict(max_iters=-1), dict(max_iters=101), dict(step_tol=-1.0),
               dict(step_tol=float("nan")), dict(min_observations=5)):
        with pytest.raises(_lib.MsfmError) as e:
            tctx.refine_camera(**kw)
        assert e.value.code == _lib.E_INVALID, kw
    assert tctx.refine_camera(min_observations=6)["refined"] in (0, 1)
    tctx.tracks_end()


# ---- state rules and the calls that follow ------------------------------------------------------------------------------------------
def test_invalidation_and_follow_on_calls_under_the_new_camera(tctx, host):
    """registrations() and pose_refinements() raise E_STATE after the call, points3d(), point_inliers() and poses() work; a following
    refine_points, refine_poses, filter_points and complete_points equal their twins run under the NEW camera."""
    ids, kps, poses, lst = ring_job([10] * 300, outlier={j: 9 for j in range(0, 300, 7)})
    open_ring(tctx, ids, kps, lst, 300)
    tracks = tctx.tracks()
    start = pfx.perturbed(poses, 21, rot=5e-4, trans=3e-3, keep=(int(ids[0]),))
    tctx.triangulate_tracks(bad(CAM), start, *THR, robust=True)
    tctx.register_images(bad(CAM), [int(ids[2])])
    tctx.registrations()
    tctx.refine_poses()
    tctx.pose_refinements()
    st, *_ = camera_same(tctx, host, ids, kps, tracks, ALL, (10, 1e-6, 100), robust=True)
    assert st["refined"] == 1
    for fetch in (tctx.registrations, tctx.pose_refinements):
        with pytest.raises(_lib.MsfmError) as e:
            fetch()
        assert e.value.code == _lib.E_STATE
    cam = cam_tuple(tctx.camera())
    assert cam != bad(CAM) and len(tctx.poses()) == len(ids)
    fhost, chost = ftw.load_host(), cmtw.load_host()
    # refine_points
    p0, r0, m0, l0, _ = state(tctx, True)
    s = tctx.refine_points()
    wp, wr, wc = rtw.run(host, tracks, ids, kps, ptw.poses_dict(*l0), cam, p0, r0, m0, THR)
    p1, r1, m1, l1, _ = state(tctx, True)
    assert p1.tobytes() == wp.tobytes() and r1.tobytes() == wr.tobytes() and s["refined"] == wc["refined"] > 0
    # refine_poses
    s = tctx.refine_poses(fixed=[int(ids[0])])
    wp, wr, wl, wrec, wc = ptw.run(host, tracks, ids, kps, l1, cam, p1, r1, m1, THR, ptw.DEFAULTS, [int(ids[0])])
    p2, r2, m2, l2, _ = state(tctx, True)
    assert p2.tobytes() == wp.tobytes() and r2.tobytes() == wr.tobytes() and l2[1].tobytes() == wl[1].tobytes() and s["refined"] == wc["refined"] > 0
    # filter_points
    s = tctx.filter_points(3.0, 1.0)
    wp, wr, wm, wc = ftw.run(fhost, tracks, ids, kps, l2, cam, p2, r2, m2, THR, (3.0, 1.0))
    p3, r3, m3, l3, _ = state(tctx, True)
    assert p3.tobytes() == wp.tobytes() and r3.tobytes() == wr.tobytes() and m3.tobytes() == wm.tobytes()
    assert {k: s[k] for k in ftw.ALL_KEYS} == wc
    # complete_points
    s = tctx.complete_points(20.0)
    wp, wr, wm, wc = cmtw.run(chost, tracks, ids, kps, l3, cam, p3, r3, m3, THR, 20.0)
    p4, r4, m4, _, c4 = state(tctx, True)
    assert p4.tobytes() == wp.tobytes() and r4.tobytes() == wr.tobytes() and m4.tobytes() == wm.tobytes()
    assert {k: s[k] for k in cmtw.ALL_KEYS} == wc and c4 == cam
    tctx.tracks_end()


def test_alternate_with_the_camera_equals_the_three_twins_chained(tctx, host):
    ids, kps, poses, lst = ring_job([10] * 300)
    open_ring(tctx, ids, kps, lst, 300)
    tracks = tctx.tracks()
    first = int(ids[0])
    tctx.triangulate_tracks(bad(CAM, 1.5), pfx.perturbed(poses, 5, keep=(first,)), *THR)
    p, r, _, l, cam = state(tctx, False)
    out = tctx.alternate(3, fixed=[first], camera_params={})
    assert len(out) == 3 and all(len(o) == 3 for o in out)
    for a, b, c in out:
        p, r, wa = rtw.run(host, tracks, ids, kps, ptw.poses_dict(*l), cam, p, r, None, THR)
        p, r, l, _, wb = ptw.run(host, tracks, ids, kps, l, cam, p, r, None, THR, ptw.DEFAULTS, [first])
        p, r, cam, wc = ctw.run(host, tracks, ids, kps, l, cam, p, r, None, THR)
        for s, w in ((b, wb), (c, wc)):                                                       # (the point call adds its costs per wave)
            assert all(np.float64(s[k]).tobytes() == np.float64(w[k]).tobytes() for k in ("cost_before", "cost_after"))
        assert a["refined"] == wa["refined"] and b["refined"] == wb["refined"] and c["refined"] == wc["refined"]
    p1, r1, _, l1, c1 = state(tctx, False)
    assert p1.tobytes() == p.tobytes() and r1.tobytes() == r.tobytes() and l1[1].tobytes() == l[1].tobytes() and cam_bytes(c1) == cam_bytes(cam)
    assert out[0][2]["refined"] == 1 and c1 != bad(CAM, 1.5)
    two = tctx.alternate(1, fixed=[first])
    assert len(two[0]) == 2                                                                   # without camera_params: as before
    tctx.tracks_end()
