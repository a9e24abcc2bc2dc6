"""Robust track triangulation on the device (msfm_triangulate_tracks_robust / msfm_fetch_point_inliers,
csrc/msfm_triangulate_robust.hip.h) against the host twin (csrc/msfm_triangulate.h, TriangulateTracksRobust, through
tests/robust_triangulation_twin.py): records, residuals, inlier bytes and the counters of both stats BYTE FOR BYTE -- on a clean job
(where it must equal the plain call), without tracks, on the corrupted tracks of real verified calls, on hand-built tracks around the
LDS tile boundaries and the enumerated | sampled threshold, with more retried tracks than the retry launch has waves and with exactly
one.  The twin itself is checked against the independent numpy reference in tests/test_robust_triangulation_reference.py."""
import numpy as np
import pytest

import registration_twin as regtw
import robust_triangulation_twin as rtw
import tracks_fixtures as fx
import triangulation_twin as tw
from monocularsfm_amd import _lib, synth

pytestmark = pytest.mark.gpu
CAM = (2500.0, 2500.0, 1536.0, 1152.0)
CAM_D = CAM + (-0.1, 0.02, 1e-3, -5e-4)
CAM_A = (2500.0, 2380.0, 1536.0, 1152.0)   # fx != fy


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return rtw.load_host()


def same(ctx, host, ids, kps, poses, cam=CAM, params=rtw.DEFAULTS, tracks=None):
    """the robust call on the device and on the twin: everything byte for byte"""
    tracks = ctx.tracks() if tracks is None else tracks
    st = ctx.triangulate_tracks(cam, poses, *params[:3], robust=True, max_hypotheses=params[3])
    pts, res = ctx.points3d()
    mask = ctx.point_inliers()
    wp, wr, wm, wc = rtw.run(host, tracks, ids, kps, poses, cam, params)
    assert pts.tobytes() == wp.tobytes(), np.nonzero(pts != wp)[0][:8]
    assert res.tobytes() == wr.tobytes(), np.nonzero(res != wr)[0][:8]
    assert mask.dtype == np.uint8 and mask.tobytes() == wm.tobytes(), np.nonzero(mask != wm)[0][:8]
    assert {k: st[k] for k in tw.COUNT_KEYS} == tw.counts(wp) and st["tracks"] == len(pts)
    assert {k: st[k] for k in rtw.ROBUST_KEYS} == wc, (st, wc)
    assert st["device_bytes"] >= 48 * len(pts) + 9 * len(res) and st["robust_ms"] >= st["triangulate_ms"] >= 0.0
    return st, pts, res, mask


def ring_job(lengths, outlier=None, rows=None, noise_px=0.3, seed=3):
    """Hand-built tracks: track j runs through the images 0 .. lengths[j] - 1 at keypoint row j; cameras 1.2 degrees apart on a circle
    around the scene; outlier: {track: position} moved by 40 px.  -> (ids, kps, poses, the list for tracks_add)"""
    rng = np.random.default_rng(seed)
    n_img, n_tr = int(max(lengths)), len(lengths)
    rows = rows or n_tr
    ids = np.arange(n_img, dtype=np.int32) * 3 + 1
    X = np.stack([rng.uniform(-1.0, 1.0, n_tr), rng.uniform(-1.0, 1.0, n_tr), rng.uniform(-1.0, 1.0, n_tr)], 1)
    kps, poses = [], {}
    for i in range(n_img):
        th = 2 * np.pi * i / 300.0
        z = np.asarray([-np.sin(th), 0.0, np.cos(th)])
        x = np.cross([0.0, 1.0, 0.0], z)
        R, t = np.stack([x, np.cross(z, x), z]), np.asarray([0.0, 0.02 * np.sin(5 * th), 6.5])
        k = synth.keypoints(rows, seed=seed + i)
        Y = X @ R.T + t
        k[:n_tr, 0] = (CAM[0] * Y[:, 0] / Y[:, 2] + CAM[2] + rng.normal(0, noise_px, n_tr)).astype(np.float32)
        k[:n_tr, 1] = (CAM[1] * Y[:, 1] / Y[:, 2] + CAM[3] + rng.normal(0, noise_px, n_tr)).astype(np.float32)
        kps.append(k)
        poses[int(ids[i])] = (R, t)
    for j, pos in (outlier or {}).items():
        kps[pos][j, 0] += np.float32(40.0)
    lengths = np.asarray(lengths)
    pairs, offs, qt = [], [0], []
    for i in range(n_img - 1):
        rows_i = np.nonzero(lengths > i + 1)[0].astype(np.int32)
        pairs.append((ids[i], ids[i + 1]))
        qt.append(np.stack([rows_i, rows_i], 1))
        offs.append(offs[-1] + len(rows_i))
    lst = (np.asarray(pairs, np.int32).reshape(-1, 2), np.asarray(offs, np.int64), np.concatenate(qt).astype(np.int32).reshape(-1, 2))
    return ids, kps, poses, lst


def open_ring(ctx, ids, kps, lst, rows):
    d = np.random.default_rng(1).integers(0, 256, (rows, 128), dtype=np.uint8)
    for k, i in enumerate(ids):
        ctx.upload_image(int(i), d)
        ctx.upload_keypoints(int(i), kps[k])
    ctx.tracks_begin(ids, add_only=True)
    if len(lst[0]):
        ctx.tracks_add(*lst)
    return ctx.tracks_finish()


def test_clean_job_equals_the_plain_call_and_no_tracks(tctx, host):
    lengths = [2, 3, 5, 7, 7, 12, 64, 65, 130] * 3
    ids, kps, poses, lst = ring_job(lengths)
    open_ring(tctx, ids, kps, lst, len(lengths))
    tctx.triangulate_tracks(CAM, poses)
    pp, pr = (a.tobytes() for a in tctx.points3d())
    with pytest.raises(_lib.MsfmError) as e:
        tctx.point_inliers()                                   # the last triangulation was the plain one
    assert e.value.code == _lib.E_STATE
    st, pts, res, mask = same(tctx, host, ids, kps, poses)
    assert st["retried"] == 0 and st["hypotheses"] == 0 and st["error_ok"] == st["tracks"] == len(lengths)   # (no retry launch)
    assert pts.tobytes() == pp and res.tobytes() == pr and np.all(mask == 1) and not (pts["status"] & _lib.TRI_ROBUST).any()
    tctx.triangulate_tracks(CAM, poses)
    assert tctx.points3d()[0].tobytes() == pp
    with pytest.raises(_lib.MsfmError) as e:
        tctx.point_inliers()
    assert e.value.code == _lib.E_STATE
    tctx.tracks_end()
    # T = 0: a session without any match
    tctx.tracks_begin(ids, add_only=True)
    tctx.tracks_finish()
    st = tctx.triangulate_tracks(CAM, poses, robust=True)
    assert st["tracks"] == 0 and st["retried"] == 0 and len(tctx.point_inliers()) == 0 and len(tctx.points3d()[0]) == 0
    tctx.tracks_end()
    with pytest.raises(_lib.MsfmError) as e:
        tctx.point_inliers()
    assert e.value.code == _lib.E_STATE


def test_hand_built_tracks_at_the_tile_and_sampling_edges(tctx, host):
    """m = 2, 3, 11, 12 (55 | 66 pairs across max_hypotheses 64: enumerated | sampled), 63, 64, 65, 128, 129, 300 (the LDS tiles of
    64), the outlier at positions 0, 63, 64 and last; max_hypotheses 1, 63, 64, 65, 128, 1024; unposed images interleaved."""
    lengths, outlier = [], {}
    for m in (2, 3, 11, 12, 63, 64, 65, 128, 129, 300):
        for pos in sorted({0, 63, 64, m - 1}):
            if pos < m:
                outlier[len(lengths)] = pos
                lengths.append(m)
    ids, kps, poses, lst = ring_job(lengths, outlier)
    ts = open_ring(tctx, ids, kps, lst, len(lengths))
    assert ts["tracks_kept"] == len(lengths) and ts["longest_track"] == 300
    tracks = tctx.tracks()
    for H in (1, 63, 64, 65, 128, 1024):
        st, pts, res, mask = same(tctx, host, ids, kps, poses, params=(2.0, 1.5, 2, H), tracks=tracks)
        assert st["retried"] == sum(m >= 3 for m in lengths)
        assert H < 64 or (st["rescued"] > 0 and st["observations_rejected"] >= st["rescued"])
    some = {i: (None if k % 7 == 3 else p) for k, (i, p) in enumerate(sorted(poses.items()))}
    same(tctx, host, ids, kps, some, params=(2.0, 1.5, 3, 64), tracks=tracks)
    same(tctx, host, ids, kps, some, cam=CAM_D, params=(1.0, 4.0, 2, 65), tracks=tracks)
    tctx.tracks_end()


def test_more_retried_tracks_than_waves_and_exactly_one(tctx, host):
    n = 5000                                                   # (the retry launch has at most 2 x 256 x 4 = 2048 waves)
    ids, kps, poses, lst = ring_job([3] * n, {j: j % 3 for j in range(n)})
    open_ring(tctx, ids, kps, lst, n)
    st, pts, _, _ = same(tctx, host, ids, kps, poses)
    assert st["retried"] == n and st["hypotheses"] == 3 * n and np.all(pts["status"] & _lib.TRI_ROBUST)
    tctx.tracks_end()
    ids, kps, poses, lst = ring_job([7] * 70, {33: 4})
    open_ring(tctx, ids, kps, lst, 70)
    st, pts, _, mask = same(tctx, host, ids, kps, poses)
    assert st["retried"] == st["rescued"] == st["observations_rejected"] == 1 and st["succeeded"] == 70
    assert np.nonzero(mask == 0)[0].tolist() == [33 * 7 + 4] and np.nonzero(pts["status"] & _lib.TRI_ROBUST)[0].tolist() == [33]
    tctx.tracks_end()


def test_corrupted_scene_job_and_nothing_else_changes(tctx, host):
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
    tctx.triangulate_tracks(CAM, poses)
    before = [a.tobytes() for a in tctx.points3d()]
    st, pts, res, mask = same(tctx, host, ids, bad, poses, tracks=tracks)
    assert st["retried"] >= len(chosen) // 2 and st["rescued"] > 0.8 * st["retried"] and st["observations_rejected"] >= st["rescued"]
    plain_ok = int(_lib.succeeded(np.frombuffer(before[0], _lib.POINT3D)).sum())
    assert st["succeeded"] >= plain_ok + st["rescued"] - 5
    # the registration after the robust call: the twin fed the robust points
    kp = {int(i): k for i, k in zip(ids, bad)}
    rs = tctx.register_images(CAM, ids[:6])
    got = tctx.registrations()
    want = regtw.run(regtw.load_host(), tracks, pts, ids[:6], kp, CAM)
    assert rs["succeeded"] > 0 and all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    # tracks and match lists unchanged; a plain call after the robust one gives the plain call's bytes again
    assert all(a.tobytes() == b.tobytes() for a, b in zip(tracks, tctx.tracks()))
    vq, vd = tctx._view()
    assert vq.tobytes() == qt.tobytes() and vd.tobytes() == dist.tobytes()
    tctx.triangulate_tracks(CAM, poses)
    assert [a.tobytes() for a in tctx.points3d()] == before
    with pytest.raises(_lib.MsfmError) as e:
        tctx.registrations()                                   # a triangulation invalidates the registrations
    assert e.value.code == _lib.E_STATE
    for cam in (CAM_D, CAM_A):
        same(tctx, host, ids, bad, poses, cam=cam, tracks=tracks)
    # a re-filter invalidates the inlier bytes
    tctx.tracks_finish(min_length=3)
    with pytest.raises(_lib.MsfmError) as e:
        tctx.point_inliers()
    assert e.value.code == _lib.E_STATE
    tctx.tracks_end()


def test_errors(tctx):
    E = _lib

    def code(fn, *a, **k):
        with pytest.raises(_lib.MsfmError) as e:
            fn(*a, **k)
        return e.value.code

    ids, kps, poses, lst = ring_job([4] * 6)
    rob = dict(robust=True)
    assert code(tctx.triangulate_tracks, CAM, poses, **rob) == E.E_STATE and code(tctx.point_inliers) == E.E_STATE   # no session
    d = np.random.default_rng(1).integers(0, 256, (6, 128), dtype=np.uint8)
    for k, i in enumerate(ids):
        tctx.upload_image(int(i), d)
        if k:
            tctx.upload_keypoints(int(i), kps[k])
    tctx.upload_image(400, d)
    tctx.tracks_begin(ids, add_only=True)
    tctx.tracks_add(*lst)
    assert code(tctx.triangulate_tracks, CAM, poses, **rob) == E.E_STATE                      # before finish
    tctx.tracks_finish()
    assert code(tctx.point_inliers) == E.E_STATE                                             # finished, not triangulated
    ok = {i: p for i, p in poses.items() if i != int(ids[0])}
    assert code(tctx.triangulate_tracks, CAM, poses, **rob) == E.E_NOIMAGE                   # a posed image without keypoints
    assert code(tctx.triangulate_tracks, None, ok, **rob) == E.E_INVALID
    for cam in ((0.0, 2500.0, 1.0, 1.0), (2500.0, -1.0, 1.0, 1.0), (2500.0, 2500.0, float("nan"), 1.0), CAM + (float("inf"),)):
        assert code(tctx.triangulate_tracks, cam, ok, **rob) == E.E_INVALID
    for kw in (dict(max_error=-1.0), dict(min_angle=-0.5), dict(max_error=float("nan")), dict(min_angle=float("inf")),
               dict(max_hypotheses=0), dict(max_hypotheses=1025), dict(max_hypotheses=-3)):
        assert code(tctx.triangulate_tracks, CAM, ok, **rob, **kw) == E.E_INVALID
    bad_r = dict(ok)
    bad_r[int(ids[1])] = (np.full((3, 3), np.nan), np.zeros(3))
    assert code(tctx.triangulate_tracks, CAM, bad_r, **rob) == E.E_INVALID
    assert code(tctx.triangulate_tracks, CAM, {**ok, 400: ok[int(ids[1])]}, **rob) == E.E_INVALID   # resident, not declared
    ids2, tab2 = _lib.pose_table(ok)
    ids2, tab2 = np.r_[ids2, ids2[:1]].astype(np.int32), np.r_[tab2, tab2[:1]]                      # an id given twice
    cam = _lib.camera_struct(CAM)
    L, h = tctx._L, tctx._h
    assert L.msfm_triangulate_tracks_robust(h, _lib.C.byref(cam), _lib._ip(ids2), tab2.ctypes.data, len(ids2), None, None, None) == E.E_INVALID
    assert L.msfm_triangulate_tracks_robust(h, _lib.C.byref(cam), None, None, 2, None, None, None) == E.E_INVALID
    assert L.msfm_triangulate_tracks_robust(h, _lib.C.byref(cam), None, None, -1, None, None, None) == E.E_INVALID
    # usable after every one of them; NULL params are the defaults, NULL outputs allowed; a failed call leaves neither points nor bytes
    ids3, tab3 = _lib.pose_table(ok)
    assert L.msfm_triangulate_tracks_robust(h, _lib.C.byref(cam), _lib._ip(ids3), tab3.ctypes.data, len(ids3), None, None, None) == E.OK
    assert L.msfm_fetch_point_inliers(h, None) == E.OK
    a = tctx.point_inliers().tobytes()
    tctx.triangulate_tracks(CAM, ok, robust=True)
    assert tctx.point_inliers().tobytes() == a
    assert code(tctx.triangulate_tracks, None, ok, **rob) == E.E_INVALID and code(tctx.point_inliers) == E.E_STATE and code(tctx.points3d) == E.E_STATE
    tctx.set_limits(max_pairs_per_batch=1)
    gen = tctx.match_pairs_stream([(int(ids[0]), int(ids[1])), (int(ids[1]), int(ids[2]))], max_distance=1e9)
    next(gen)
    assert code(tctx.triangulate_tracks, CAM, ok, **rob) == E.E_STATE                        # while a series is open
    gen.close()
    tctx.tracks_end()
