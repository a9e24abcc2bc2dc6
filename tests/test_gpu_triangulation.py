"""Track triangulation on the device (msfm_triangulate_tracks / msfm_fetch_points3d, csrc/msfm_triangulate.hip.h) against the host twin
(csrc/msfm_triangulate.h through tests/triangulation_twin.py): the records and the residuals BYTE FOR BYTE -- on the tracks of real
verified calls, on hand-made tracks with unposed images, inconsistent and length-2 tracks, under min_views = 3 and a distorted camera,
and at the production shape (1329 images x 8192 keypoints).  The twin itself is checked against the independent numpy reference in
tests/test_triangulation_reference.py."""
import numpy as np
import pytest

import tracks_fixtures as fx
import triangulation_twin as tw
from monocularsfm_amd import _lib, synth

pytestmark = pytest.mark.gpu
CAM = (2500.0, 2500.0, 1536.0, 1152.0)
CAM_D = CAM + (-0.1, 0.02, 1e-3, -5e-4)


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return tw.load_host()


def same(ctx, host, ids, kps, poses, cam=CAM, params=tw.DEFAULTS, tracks=None):
    """triangulate on the device and on the twin: records and residuals byte for byte, the stats' counts from the records"""
    tracks = ctx.tracks() if tracks is None else tracks
    st = ctx.triangulate_tracks(cam, poses, *params)
    pts, res = ctx.points3d()
    wp, wr = tw.run(host, tracks, ids, kps, poses, cam, params)
    assert pts.dtype == tw.POINT3D and len(pts) == len(tracks[0]) - 1 and len(res) == len(tracks[1])
    assert pts.tobytes() == wp.tobytes(), np.nonzero(pts != wp)[0][:8]
    assert res.tobytes() == wr.tobytes()
    want = tw.counts(wp)
    assert {k: st[k] for k in tw.COUNT_KEYS} == want and st["tracks"] == len(pts)
    assert st["device_bytes"] >= 48 * len(pts) + 8 * len(res) and st["triangulate_ms"] >= 0.0
    assert np.array_equal(_lib.succeeded(pts), (wp["status"] & 14) == 14)
    return st, pts, res


def scene_poses(ids, seed=77):
    return {int(i): (c[0], c[1]) for i, c in zip(ids, synth.scene_cameras(len(ids), seed=seed))}


def test_real_verified_tracks_and_nothing_else_changes(tctx, host):
    ids, imgs, kps, pairs = fx.scene_job()
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), imgs[k])
        tctx.upload_keypoints(int(i), kps[k])
    kp = {int(i): k for i, k in zip(ids, kps)}
    poses = scene_poses(ids)
    tctx.set_verification_model(_lib.VERIFY_ESSENTIAL, CAM)
    tctx.tracks_begin(ids)
    offs, qt, dist = tctx.match_pairs_verified(pairs)
    tctx.tracks_finish()
    before = tctx.tracks()
    st, pts, res = same(tctx, host, ids, kp, poses)
    assert st["tracks"] > 1000 and st["succeeded"] > 0.8 * st["tracks"] and st["error_ok"] < st["with_point"] == st["attempted"] == st["tracks"]
    # existing results unchanged: the track result and the match lists, byte for byte
    after = tctx.tracks()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    vq, vd = tctx._view()
    assert vq.tobytes() == qt.tobytes() and vd.tobytes() == dist.tobytes()
    # repeat under other parameters, with images unposed, under a distorted camera
    same(tctx, host, ids, kp, poses, params=(1.0, 4.0, 3))
    some = {i: (None if k % 5 == 0 else p) for k, (i, p) in enumerate(sorted(poses.items())) if k % 7}
    s2, p2, r2 = same(tctx, host, ids, kp, some, params=(2.0, 1.5, 3))
    assert 0 < s2["attempted"] < s2["tracks"] and (r2 < 0).sum() > (res < 0).sum()
    same(tctx, host, ids, kp, poses, cam=CAM_D)
    # re-filter: the points are gone until triangulation runs again, then they belong to the new tracks
    st3 = tctx.tracks_finish(min_length=3)
    with pytest.raises(_lib.MsfmError) as e:
        tctx.points3d()
    assert e.value.code == _lib.E_STATE
    assert st3["tracks_kept"] < st["tracks"]
    s4, p4, _ = same(tctx, host, ids, kp, poses)
    assert s4["tracks"] == st3["tracks_kept"] and p4["n_views"].min() >= 3
    tctx.tracks_end()
    with pytest.raises(_lib.MsfmError) as e:
        tctx.points3d()
    assert e.value.code == _lib.E_STATE


def test_hand_made_tracks(tctx, host):
    """fx.HAND through tracks_add, inconsistent tracks kept: unposed images, an inconsistent track, tracks of length 2; min_views 3;
    a distorted camera.  (The geometry is arbitrary: keypoints at random places -- the device must still give the twin's bytes.)"""
    rng = np.random.default_rng(5)
    kp = {}
    for i, n in zip(fx.IDS, fx.ROWS):
        tctx.upload_image(int(i), rng.integers(0, 256, (int(n), 128), dtype=np.uint8))
        kp[int(i)] = synth.keypoints(int(n), seed=int(i))
        if int(i) != 9:
            tctx.upload_keypoints(int(i), kp[int(i)])
    poses = scene_poses(np.sort(fx.IDS), seed=3)
    poses[9] = None                                              # listed, not valid -- and it has no keypoints
    tctx.tracks_begin(fx.IDS, min_pair_matches=fx.MIN_PAIR)
    tctx.tracks_add(*fx.csr(fx.HAND))
    tctx.tracks_finish(keep_inconsistent=True)
    tracks = tctx.tracks()
    assert (np.diff(tracks[0]) == 2).any() and (tracks[3] == 0).any() and (tracks[1] == 9).any()
    for cam, params in ((CAM, tw.DEFAULTS), (CAM, (50.0, 0.5, 3)), (CAM_D, (1e4, 0.0, 2))):
        st, pts, res = same(tctx, host, fx.IDS, kp, poses, cam, params)
        assert np.all(pts["status"][tracks[3] == 0] == 0) and np.all(res[tracks[1] == 9] == -1.0)
        assert 0 < st["attempted"] < st["tracks"]
    del poses[9]                                                 # not listed: the same records
    a = tctx.points3d()[0].tobytes()
    tctx.triangulate_tracks(CAM_D, poses, 1e4, 0.0, 2)
    assert tctx.points3d()[0].tobytes() == a
    # NULL params are the reference's defaults; NULL outputs are allowed
    ids_, tab = _lib.pose_table(poses)
    cam = _lib.camera_struct(CAM)
    assert tctx._L.msfm_triangulate_tracks(tctx._h, _lib.C.byref(cam), _lib._ip(ids_), tab.ctypes.data, len(ids_), None, None) == _lib.OK
    assert tctx._L.msfm_fetch_points3d(tctx._h, None, None) == _lib.OK
    d = tctx.points3d()[0].tobytes()
    tctx.triangulate_tracks(CAM, poses)
    assert tctx.points3d()[0].tobytes() == d
    tctx.tracks_end()


def test_errors(tctx):
    E = _lib

    def code(fn, *a, **k):
        with pytest.raises(_lib.MsfmError) as e:
            fn(*a, **k)
        return e.value.code

    rng = np.random.default_rng(5)
    for i, n in zip(fx.IDS, fx.ROWS):
        tctx.upload_image(int(i), rng.integers(0, 256, (int(n), 128), dtype=np.uint8))
        if int(i) != 9:
            tctx.upload_keypoints(int(i), synth.keypoints(int(n), seed=int(i)))
    tctx.upload_image(40, rng.integers(0, 256, (4, 128), dtype=np.uint8))
    poses = scene_poses(np.sort(fx.IDS), seed=3)
    ok = {i: p for i, p in poses.items() if i != 9}
    # state: no session, before finish, while a series is open
    assert code(tctx.triangulate_tracks, CAM, ok) == E.E_STATE and code(tctx.points3d) == E.E_STATE
    tctx.tracks_begin(fx.IDS)
    tctx.tracks_add(*fx.csr(fx.HAND))
    assert code(tctx.triangulate_tracks, CAM, ok) == E.E_STATE and code(tctx.points3d) == E.E_STATE
    tctx.tracks_finish()
    assert code(tctx.points3d) == E.E_STATE                      # finished, not triangulated
    tctx.set_limits(max_pairs_per_batch=1)
    gen = tctx.match_pairs_stream([(3, 5), (5, 7)], max_distance=1e9)
    next(gen)
    assert code(tctx.triangulate_tracks, CAM, ok) == E.E_STATE
    gen.close()
    # invalid: camera, parameters, poses, ids
    assert code(tctx.triangulate_tracks, None, ok) == E.E_INVALID
    for cam in ((0.0, 2500.0, 1.0, 1.0), (2500.0, -1.0, 1.0, 1.0), (2500.0, 2500.0, float("nan"), 1.0), CAM + (float("inf"),)):
        assert code(tctx.triangulate_tracks, cam, ok) == E.E_INVALID
    for kw in (dict(max_error=-1.0), dict(min_angle=-0.5), dict(max_error=float("nan")), dict(min_angle=float("inf"))):
        assert code(tctx.triangulate_tracks, CAM, ok, **kw) == E.E_INVALID
    bad_r = dict(ok)
    bad_r[3] = (np.full((3, 3), np.nan), np.zeros(3))
    bad_t = dict(ok)
    bad_t[5] = (np.eye(3), np.asarray([0.0, np.inf, 0.0]))
    assert code(tctx.triangulate_tracks, CAM, bad_r) == E.E_INVALID and code(tctx.triangulate_tracks, CAM, bad_t) == E.E_INVALID
    assert code(tctx.triangulate_tracks, CAM, {**ok, 40: ok[3]}) == E.E_INVALID   # resident, not declared
    assert code(tctx.triangulate_tracks, CAM, {**ok, 10007: ok[3]}) == E.E_INVALID and code(tctx.triangulate_tracks, CAM, {**ok, -1: ok[3]}) == E.E_INVALID
    ids2, tab2 = _lib.pose_table(ok)
    ids2 = np.r_[ids2, ids2[:1]].astype(np.int32)                # an id given twice
    tab2 = np.r_[tab2, tab2[:1]]
    cam = _lib.camera_struct(CAM)
    L, h = tctx._L, tctx._h
    assert L.msfm_triangulate_tracks(h, _lib.C.byref(cam), _lib._ip(ids2), tab2.ctypes.data, len(ids2), None, None) == E.E_INVALID
    assert L.msfm_triangulate_tracks(h, _lib.C.byref(cam), None, None, 2, None, None) == E.E_INVALID
    assert L.msfm_triangulate_tracks(h, _lib.C.byref(cam), None, None, -1, None, None) == E.E_INVALID
    # a posed image without keypoints
    assert code(tctx.triangulate_tracks, CAM, poses) == E.E_NOIMAGE
    # the context is usable after every one of them; no poses at all is a valid call (nothing is attempted)
    st = tctx.triangulate_tracks(CAM, {})
    assert st["attempted"] == 0 and st["tracks"] > 0 and np.all(tctx.points3d()[0]["status"] == 0) and np.all(tctx.points3d()[1] == -1.0)
    assert tctx.triangulate_tracks(CAM, ok)["attempted"] > 0
    assert code(tctx.triangulate_tracks, None, ok) == E.E_INVALID and code(tctx.points3d) == E.E_STATE   # a failed call leaves no points
    tctx.tracks_end()


# ---- the production shape -------------------------------------------------------------------------------------------------------------
N_IMG, N_KP, LONG_LEN, N_LONG = 1329, 8192, 300, 8


def test_production_shape(tctx, host):
    """1329 x 8192: ~1.78 M tracks, ~10.6 M observations folded from synthetic lists (no matching time).  The device equals the twin on
    EVERY track (a superset of a sample plus the long ones), and the stats' counts equal the twin's over all tracks."""
    ids, kps, poses, lists = synth.triangulation_job(N_IMG, N_KP, CAM, long_len=LONG_LEN, n_long=N_LONG)
    d = np.random.default_rng(1).integers(0, 256, (N_KP, 128), dtype=np.uint8)
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), d)
        tctx.upload_keypoints(int(i), kps[k])
    tctx.tracks_begin(ids, add_only=True)
    for l in lists:
        tctx.tracks_add(*l)
    ts = tctx.tracks_finish()
    assert ts["tracks_inconsistent"] == 0 and ts["longest_track"] == LONG_LEN and ts["tracks_kept"] > 1_700_000 and ts["observations_kept"] > 10_000_000
    tracks = tctx.tracks()
    kp = {int(i): k for i, k in zip(ids, kps)}
    st, pts, res = same(tctx, host, ids, kp, poses, tracks=tracks)
    long_ones = np.nonzero(np.diff(tracks[0]) == LONG_LEN)[0]
    assert len(long_ones) == N_LONG and np.all(pts["n_views"][long_ones] == LONG_LEN - 6)   # (six of every 300 are unposed)
    assert np.all(_lib.succeeded(pts[long_ones]))
    assert st["succeeded"] > 0.8 * st["tracks"] and 0 < st["tracks"] - st["angle_ok"] and st["error_ok"] < st["with_point"]
    print("production shape: %d tracks, %d observations used, triangulate_ms %.3f, stats %s" % (st["tracks"], st["observations_used"], st["triangulate_ms"], st))
    tctx.tracks_end()
