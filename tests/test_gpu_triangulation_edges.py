"""tri_track_kernel (csrc/msfm_triangulate.hip.h) at its kernel, verdict and scan edges, everything through test_gpu_triangulation.same():
records and residuals BYTE FOR BYTE with the host twin, the counters with the twin's counts.  The jobs and the checks are
tests/triangulation_fixtures.py's, which tests/test_triangulation_fixtures.py runs on the twin: every exit of triangulate_track at the
lanes 0, 63, 64, 255 and 256 and under track counts 257, 256, 255, 65, 64, 63 and 1 (a partly filled last wave calls
wave_add_counters with lanes beyond T), err <= max_error and angle >= min_angle met with equality by the device's own numbers, the
parameters at their limits, the scan's first pair, the shifted and scaled scenes and the small-parallax tracks of
tests/test_triangulation_reference.py (the same bits from hipcc as from g++, where a contraction or another sqrt or division would
show first), a small second grid-stride pass, and the plain call behind a robust one."""
import numpy as np
import pytest

import test_triangulation_reference as tb
import triangulation_fixtures as tf
import triangulation_ref as ref
import triangulation_twin as tw
from monocularsfm_amd import _lib
from test_gpu_robust_triangulation import second_pass_job
from test_gpu_triangulation import CAM, CAM_D, same

pytestmark = pytest.mark.gpu


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return tw.load_host()


def device_run(ctx, host, job, tracks):
    """the callable the shared checks take: one device call, compared with the twin by same()"""
    def run(params=tw.DEFAULTS, poses=None, cam=CAM):
        return same(ctx, host, job["ids"], job["kps"], job["poses"] if poses is None else poses, cam, params, tracks)[1:]
    return run


ROUTE_CASES = [(tf.N_TRACKS, layout) for layout in range(len(tf.LAYOUTS))] + [(T, 0) for T in tf.PREFIXES]


@pytest.mark.parametrize("T,layout", ROUTE_CASES)
def test_routes_at_the_wave_and_block_edges(tctx, host, T, layout):
    """T = 257 under every layout (each route at each of the lanes 0, 63, 64, 255, 256), and the prefixes of layout 0: a session over
    the first T tracks' images, whose records are the first T of the full job's.  The planted status words by position; no -1 in a
    posed slot next to a track without residuals."""
    job = tf.routes_job(T, layout)
    tracks = tf.open_job(tctx, job)
    full = tf.twin_run(host, tf.routes_job(layout=layout))
    for cam in (CAM, CAM_D):
        st, pts, res = same(tctx, host, job["ids"], job["kps"], job["poses"], cam, tracks=tracks)
        seen = {p: (r, int(pts[p]["status"])) for p, r in sorted(job["planted"].items())}
        print("T %d, layout %d, %d camera parameters: {lane: (route, status)} %s" % (T, layout, len(cam), seen))
        assert all(s == tf.ROUTE_STATUS[r] for r, s in seen.values()), seen
        n_depth = sum(r == "depth" for r in job["planted"].values())   # (the verdict has no depth test: 15 counts as succeeded)
        assert int((pts["status"] == tf.SUCCEEDED).sum()) == T - len(seen) == st["succeeded"] - n_depth and st["tracks"] == T
        bare = tf.neighbours_hold_residuals(job, pts, res)
        assert sorted(bare) == sorted(p for p, r in job["planted"].items() if r in tf.NO_RESIDUALS)
        tf.verdicts_follow(job, pts, res, tw.DEFAULTS)
        fp, fr = full(cam=cam)
        assert pts.tobytes() == fp[:T].tobytes() and res.tobytes() == fr[:len(res)].tobytes()
    tctx.tracks_end()


def test_thresholds_met_with_equality(tctx, host):
    job = tf.routes_job()
    seen = tf.equality_checks(device_run(tctx, host, job, tf.open_job(tctx, job)), job)
    print("equality on the device: {track: (threshold, status at it, status one place off)} %s" % seen)
    assert len(seen) == 6 and {63, 64} <= set(seen)
    tctx.tracks_end()


def test_parameters_at_their_limits(tctx, host):
    job = tf.routes_job()
    worst = tf.parameter_checks(device_run(tctx, host, job, tf.open_job(tctx, job)), job, tb.TOL_ANGLE)
    print("parameters on the device: worst |tri_angle - reference angle| %.3g degrees" % worst)
    tctx.tracks_end()


def test_scan_stops_at_the_first_pair(tctx, host):
    job = tf.scan_order_job()
    run = device_run(tctx, host, job, tf.open_job(tctx, job))
    ang = tf.scan_order_check(run, job, tb.TOL_ANGLE)
    pts, _ = run((2.0, 91.0, 2))                                # no pair reaches it: the largest of all pairs, (5, 3)
    assert not int(pts[0]["status"]) & ref.ANGLE_OK and abs(float(pts[0]["tri_angle"]) - max(ang.values())) <= tb.TOL_ANGLE
    tctx.tracks_end()


@pytest.fixture(scope="module")
def capture_session(built_lib):
    """ONE session on the seed-5 capture's tracks for every case of MP_CASES -> (context, capture, its tracks on the device)"""
    c, _ = tf.conditioning_jobs()
    ctx = _lib.Context(0)
    d = np.random.default_rng(1).integers(0, 256, (len(c["kps"][int(c["ids"][0])]), 128), dtype=np.uint8)
    for i in c["ids"]:
        ctx.upload_image(int(i), d)
        ctx.upload_keypoints(int(i), c["kps"][int(i)])
    ctx.tracks_begin(c["ids"], add_only=True)
    ctx.tracks_add(*c["lst"])
    assert ctx.tracks_finish()["tracks_kept"] == len(c["tracks"][0]) - 1
    tracks = ctx.tracks()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(tracks, c["tracks"]))
    yield ctx, c, tracks
    ctx.tracks_end()
    ctx.close()


@pytest.mark.parametrize("case", range(len(tb.MP_CASES)), ids=[m[0] for m in tb.MP_CASES])
def test_ill_conditioned_scenes_equal_the_twin(capture_session, host, case):
    """One call per entry of MP_CASES in the one session of capture_session: the twin's bytes, so the mpmath bounds of
    tests/test_triangulation_reference.py hold for the device; MP_BOUNDS is asserted directly on the 20 tracks that lie farthest
    from the 50-digit solution in the case."""
    ctx, c, tracks = capture_session
    name, poses = c["cases"][case]
    st, pts, _ = same(ctx, host, c["ids"], c["kps"], poses, c["cam"], tracks=tracks)
    assert st["with_point"] == st["tracks"] == len(pts)
    far = max(tf.mp_distance(c, poses, pts, t) for t in tf.MP_WORST[name])
    print("%s: worst |X_device - X_mp| over the recorded tracks %.3g (bound %.3g)" % (name, far, tb.MP_BOUNDS[name]))
    assert far <= tb.MP_BOUNDS[name], (name, far)


def test_small_parallax_tracks_equal_the_twin(tctx, host):
    """a second session: depth 1e1 .. 1e5 over unit baselines under min_angle = 0, parallax from 5.7 down to 5.7e-4 degrees"""
    small = tf.conditioning_jobs()[1]
    tracks = tf.open_job(tctx, small)
    st, pts, _ = same(tctx, host, small["ids"], small["kps"], small["poses"], CAM, (2.0, 0.0, 2), tracks)
    assert st["succeeded"] == st["tracks"] == 10 and pts["tri_angle"].min() < 1e-3 < 5.0 < pts["tri_angle"].max()
    tctx.tracks_end()


SECOND_PASS_PARAMS = (0.5, 4.5, 2)   # 0.3 px of noise; the cameras left to the last tracks stand 4.8 degrees apart (1586 or more of the last
#                                      8192 succeed in the twin at 256 CUs, 2684 or fewer have ERROR_OK)


def test_second_grid_stride_pass(tctx, host):
    """tri_track_kernel's grid holds 8 x CUs x 256 lanes: with 8192 tracks more its first 32 workgroups run the grid-stride loop a
    second time.  The middle image of the last three is unposed, so the last tracks have two views; under thresholds at the noise
    and at the cameras' angle both verdicts occur among them."""
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
    some = {i: (None if i == int(ids[-2]) else p) for i, p in poses.items()}
    st, pts, res = same(tctx, host, ids, kps, some, CAM, SECOND_PASS_PARAMS)
    last = _lib.succeeded(pts[T - 8192:])
    print("second pass: T %d, triangulate_ms %.3f, %d of the last 8192 succeeded" % (T, st["triangulate_ms"], int(last.sum())))
    n_last = T - (len(ids) // 3 - 1) * 8192                     # the tracks through the last three images
    assert 500 < last.sum() < 7692 and np.all(pts["n_views"][T - n_last:] == 2) and np.all(pts["n_views"][:T - n_last] == 3)
    assert (res[-3 * n_last:] == -1.0).sum() == n_last and not (res[:-3 * n_last] == -1.0).any()
    tctx.tracks_end()


def test_plain_call_after_a_robust_one(tctx, host):
    """The robust call retries the tracks without ERROR_OK and rewrites their records; the plain call behind it leaves what a fresh
    session's plain call leaves, and no inlier bytes."""
    job = tf.routes_job()
    tracks = tf.open_job(tctx, job)
    st = tctx.triangulate_tracks(CAM, job["poses"], robust=True)
    assert st["retried"] > 0 and (tctx.points3d()[0]["status"] & _lib.TRI_ROBUST).any() and len(tctx.point_inliers()) == len(tracks[1])
    _, pts, res = same(tctx, host, job["ids"], job["kps"], job["poses"], tracks=tracks)
    with pytest.raises(_lib.MsfmError) as e:
        tctx.point_inliers()
    assert e.value.code == _lib.E_STATE and not (pts["status"] & _lib.TRI_ROBUST).any()
    tctx.tracks_end()
    tf.open_job(tctx, job)                                      # a fresh session
    tctx.triangulate_tracks(CAM, job["poses"])
    fp, fr = tctx.points3d()
    assert pts.tobytes() == fp.tobytes() and res.tobytes() == fr.tobytes()
    tctx.tracks_end()
