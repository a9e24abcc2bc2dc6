"""Image registration on the device (msfm_register_images / msfm_fetch_registrations, csrc/msfm_register.hip.h) against the host twin
(csrc/msfm_register.h through tests/registration_twin.py): records, offsets, track ids, flags and residuals BYTE FOR BYTE -- on the
tracks of real verified calls, on small hand-made sessions (0, 2, 3, a few and exactly min_inliers correspondences, collinear points,
more images than the round kernel's grid has workgroups), with outliers, without refinement, and through every error.  The twin itself
is checked against the independent numpy reference in tests/test_registration_reference.py."""
import numpy as np
import pytest

import registration_twin as tw
import tracks_fixtures as fx
from monocularsfm_amd import _lib, synth

pytestmark = pytest.mark.gpu
CAM = (2500.0, 2500.0, 1536.0, 1152.0)
TILE = 256   # kRegTile of csrc/msfm_register.hip.h


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def host():
    return tw.load_host()


def same(ctx, host, image_ids, kp, cam=CAM, **params):
    """register on the device and on the twin: everything byte for byte, the stats from the twin's records"""
    tracks, points = ctx.tracks(), ctx.points3d()[0]
    st = ctx.register_images(cam, image_ids, **params)
    got = ctx.registrations()
    want = tw.run(host, tracks, points, image_ids, kp, cam, **params)
    names = ("records", "offsets", "track ids", "flags", "residuals")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, np.nonzero(g != w)[0][:8])
    rec = want[0]
    rounds, solved = tw.schedule(rec, params.get("max_iters", tw.DEFAULTS["max_iters"]))
    assert st["images"] == len(image_ids) and st["correspondences"] == len(want[2])
    assert st["attempted"] == int(((rec["status"] & _lib.REG_ATTEMPTED) != 0).sum())
    assert st["succeeded"] == int(_lib.registered(rec).sum())
    assert (st["rounds"], st["hypotheses"]) == (rounds, solved), (st, rounds, solved)
    assert st["device_bytes"] >= 128 * len(rec) + 13 * len(want[2]) and st["register_ms"] >= 0.0
    return st, got


def scene_poses(ids, seed=77):
    return {int(i): (c[0], c[1]) for i, c in zip(ids, synth.scene_cameras(len(ids), seed=seed))}


def scene_session(ctx, n_images=24, n_desc=600):
    ids, imgs, kps, pairs = fx.scene_job(n_images=n_images, n_desc=n_desc)
    for k, i in enumerate(ids):
        ctx.upload_image(int(i), imgs[k])
        ctx.upload_keypoints(int(i), kps[k])
    ctx.set_verification_model(_lib.VERIFY_ESSENTIAL, CAM)
    ctx.tracks_begin(ids)
    lists = ctx.match_pairs_verified(pairs)
    ctx.tracks_finish()
    return ids, {int(i): k for i, k in zip(ids, kps)}, scene_poses(ids), lists


def test_scene_job_all_images_and_nothing_else_changes(tctx, host):
    ids, kp, poses, (offs, qt, dist) = scene_session(tctx)
    with pytest.raises(_lib.MsfmError) as e:        # before triangulation
        tctx.register_images(CAM, ids)
    assert e.value.code == _lib.E_STATE
    tctx.triangulate_tracks(CAM, poses)
    before = [a.tobytes() for a in tctx.tracks()] + [a.tobytes() for a in tctx.points3d()]
    st, (rec, roffs, tid, flags, res) = same(tctx, host, ids, kp)
    n = np.diff(roffs)
    assert len(set(n.tolist())) > 5 and np.all(n % TILE != 0) and n.max() > TILE and n.min() > 15   # ragged, more than one tile
    assert st["succeeded"] == 24 and np.all(rec["status"] == 15) and st["rounds"] == 1 and st["hypotheses"] == 24 * 64
    for r in rec:                                                            # ground truth: the poses the points were made with
        R, t = poses[int(r["image_id"])]
        assert np.abs(r["R"].reshape(3, 3) - R).max() < 5e-3 and np.abs(r["t"] - t).max() < 2e-2
    after = [a.tobytes() for a in tctx.tracks()] + [a.tobytes() for a in tctx.points3d()]
    vq, vd = tctx._view()
    assert before == after and vq.tobytes() == qt.tobytes() and vd.tobytes() == dist.tobytes()
    # refinement off against on; another order of the list and a subset
    s0, (rec0, *_rest) = same(tctx, host, ids, kp, refine_iters=0)
    assert np.all((rec0["status"] & _lib.REG_REFINED) == 0) and np.all(rec0["n_inliers"] <= rec["n_inliers"] + 5)
    same(tctx, host, ids[::-1][:7], kp, max_error=1.0, min_inliers=30)
    s3, _ = same(tctx, host, ids, kp, max_error=0.5)          # below the capture's noise: several rounds per image
    assert s3["rounds"] >= 2
    # 30 % of one image's keypoints moved by tens of pixels; all keypoints of another shuffled: it runs every round and fails
    rng = np.random.default_rng(3)
    a, b, c = int(ids[4]), int(ids[9]), int(ids[2])
    moved = {i: k.copy() for i, k in kp.items()}
    sel = rng.random(len(moved[a])) < 0.3
    moved[a][sel, :2] += (rng.uniform(20, 60, (int(sel.sum()), 2)) * rng.choice([-1, 1], (int(sel.sum()), 2))).astype(np.float32)
    moved[b][:, :2] = moved[b][rng.permutation(len(moved[b])), :2]
    for i in (a, b):
        tctx.upload_keypoints(i, moved[i])
    s1, (rec1, *_rest) = same(tctx, host, [a, b, c], moved, max_iters=192)
    assert int(rec1[0]["status"]) == 15 and 0.55 * rec1[0]["n_correspondences"] < rec1[0]["n_inliers"] < 0.85 * rec1[0]["n_correspondences"]
    assert not _lib.registered(rec1)[1] and int(rec1[1]["hypotheses"]) == 192 and int(rec1[2]["hypotheses"]) == 64
    assert s1["rounds"] == 3 and s1["hypotheses"] == 192 + 64 + int(rec1[0]["hypotheses"])
    # a new finish invalidates the registrations and the points
    tctx.tracks_finish(min_length=3)
    for call in (tctx.registrations, lambda: tctx.register_images(CAM, ids)):
        with pytest.raises(_lib.MsfmError) as e:
            call()
        assert e.value.code == _lib.E_STATE


def test_the_loop_register_then_triangulate_again(tctx, host):
    ids, kp, poses, _ = scene_session(tctx)
    half = {i: p for k, (i, p) in enumerate(sorted(poses.items())) if k % 2 == 0}
    rest = [i for i in poses if i not in half]
    s1 = tctx.triangulate_tracks(CAM, half)
    st, (rec, *_rest) = same(tctx, host, rest, kp)
    assert st["succeeded"] == len(rest)
    more = _lib.registered_poses(rec, half)
    assert set(more) == set(poses) and set(half) < set(more)
    s2 = tctx.triangulate_tracks(CAM, more)
    assert s2["succeeded"] > s1["succeeded"] and s2["attempted"] > s1["attempted"]
    with pytest.raises(_lib.MsfmError) as e:        # the new points do not carry the old registrations
        tctx.registrations()
    assert e.value.code == _lib.E_STATE


def test_refined_pose_that_loses_inliers_is_dropped(tctx, host):
    """refine_iters = 10 against 0 where the refined pose has FEWER inliers than the winner: the capture of
    tests/test_registration_reference.py (its ground-truth tracks through tracks_add, 0.3 px of noise) at max_error = 0.3 px.  The
    unrefined pose and its mask stand -- POSE without REFINED -- and the device gives the twin's bytes."""
    import test_triangulation_reference as tri
    c = tri.capture(77, noise_px=0.3, cam=CAM)
    rng = np.random.default_rng(2)
    for i in c["ids"]:
        tctx.upload_image(int(i), rng.integers(0, 256, (len(c["kps"][int(i)]), 128), dtype=np.uint8))
        tctx.upload_keypoints(int(i), c["kps"][int(i)])
    offs, img, idx = c["tracks"][0], c["tracks"][1], c["tracks"][2]
    edges = {}
    for t in range(len(offs) - 1):                      # a chain through every track's elements
        for e in range(offs[t], offs[t + 1] - 1):
            edges.setdefault((int(img[e]), int(img[e + 1])), []).append((int(idx[e]), int(idx[e + 1])))
    tctx.tracks_begin(c["ids"], min_pair_matches=1)
    tctx.tracks_add(*fx.csr(sorted(edges.items())))
    tctx.tracks_finish()
    assert all(a.tobytes() == np.asarray(b).astype(a.dtype).tobytes() for a, b in zip(tctx.tracks()[:3], c["tracks"][:3]))
    tctx.triangulate_tracks(CAM, c["poses"])
    st, (rec, roffs, tid, flags, res) = same(tctx, host, c["ids"], c["kps"], max_error=0.3)
    dropped = (rec["status"] & (_lib.REG_POSE | _lib.REG_REFINED)) == _lib.REG_POSE
    assert dropped.sum() >= 1 and np.all(_lib.registered(rec[dropped])) and (rec["status"] == 15).sum() >= 20 and st["rounds"] == 3
    s0, (rec0, _o, _t, flags0, res0) = same(tctx, host, c["ids"], c["kps"], max_error=0.3, refine_iters=0)
    assert np.all((rec0["status"] & _lib.REG_REFINED) == 0)
    for k in np.nonzero(dropped)[0]:                    # the dropped image's record and mask ARE the unrefined run's
        a, b = roffs[k], roffs[k + 1]
        assert rec[k].tobytes() == rec0[k].tobytes() and flags[a:b].tobytes() == flags0[a:b].tobytes() and res[a:b].tobytes() == res0[a:b].tobytes()
    kept = np.nonzero(~dropped)[0]                      # ... and where the refined pose stands it has at least the winner's inliers
    assert np.all(rec["n_inliers"][kept] >= rec0["n_inliers"][kept]) and (rec["n_inliers"][kept] > rec0["n_inliers"][kept]).any()


def small_session(ctx, counts, n_points=40, seed=9, line=()):
    """Three posed images that see all n_points scene points and one target image per entry of `counts` that sees that many of them
    (targets listed in `line` see points on one straight line).  Exact projections, tracks by tracks_add.  -> (ids, kp, poses, targets)"""
    rng = np.random.default_rng(seed)
    n = 3 + len(counts)
    cams = synth.scene_cameras(n, seed=seed)
    X = np.stack([rng.uniform(-1.6, 1.6, n_points), rng.uniform(-1.1, 1.1, n_points), rng.uniform(-1.0, 1.0, n_points)], 1)
    X[:8] = X[0] + np.outer(np.arange(8), [0.11, 0.07, -0.05])           # the first eight points lie on a line
    ids = np.arange(n, dtype=np.int32) * 2 + 1
    seen = [np.arange(n_points)] * 3
    for j, m in enumerate(counts):
        seen.append(np.arange(m) if j in line else 8 + rng.permutation(n_points - 8)[:m])
    kp, items = {}, []
    for i in range(n):
        R, t, f, cx, cy = cams[i]
        Y = X[seen[i]] @ R.T + t
        k = np.zeros((max(len(seen[i]), 1), 4), np.float32)
        k[:len(seen[i]), 0] = f * Y[:, 0] / Y[:, 2] + cx
        k[:len(seen[i]), 1] = f * Y[:, 1] / Y[:, 2] + cy
        kp[int(ids[i])] = k
        ctx.upload_image(int(ids[i]), rng.integers(0, 256, (len(k), 128), dtype=np.uint8))
        ctx.upload_keypoints(int(ids[i]), k)
        if i in (1, 2) or (i >= 3 and len(seen[i])):
            items.append(((int(ids[0]), int(ids[i])), [(int(p), q) for q, p in enumerate(seen[i])]))
    ctx.tracks_begin(ids, min_pair_matches=1)
    ctx.tracks_add(*fx.csr(items))
    ctx.tracks_finish()
    poses = {int(ids[i]): (cams[i][0], cams[i][1]) for i in range(3)}
    truth = {int(ids[i]): (cams[i][0], cams[i][1]) for i in range(n)}
    return ids, kp, poses, [int(i) for i in ids[3:]], truth


def test_small_images_and_degenerate_samples(tctx, host):
    counts = [0, 2, 3, 7, 15, 4, 3]
    ids, kp, poses, targets, truth = small_session(tctx, counts, line=(5, 6))
    st3 = tctx.triangulate_tracks(CAM, poses)
    assert st3["succeeded"] == 40
    st, (rec, roffs, tid, flags, res) = same(tctx, host, targets, kp)     # min_inliers = 15
    assert np.diff(roffs).tolist() == counts
    assert rec["status"].tolist() == [0, 0, 0, 0, 15, 0, 0] and np.all(res[:roffs[4]] == -1.0)
    st, (rec, *_rest) = same(tctx, host, targets, kp, min_inliers=3)
    assert rec["status"][:2].tolist() == [0, 0] and np.all(rec["status"][2:5] == 15)
    for k in (3, 4):                        # exact data: the true pose (three points alone leave up to four poses: not image 2)
        R, t = truth[targets[k]]
        assert np.abs(rec[k]["R"].reshape(3, 3) - R).max() < 1e-5 and np.abs(rec[k]["t"] - t).max() < 1e-4
    # correspondences on one line: every sample is collinear, no hypothesis has a pose, the record has none
    assert rec["status"][5:].tolist() == [1, 1] and np.all(rec["R"][5:] == 0) and np.all(rec["n_inliers"][5:] == 0)
    assert rec["hypotheses"][5:].tolist() == [1024, 1024]
    same(tctx, host, targets, kp, min_inliers=0, max_iters=70, refine_iters=1)
    same(tctx, host, [], kp)
    # errors
    L, h, cam = tctx._L, tctx._h, _lib.camera_struct(CAM)
    ip = _lib._ip

    def rc(ids_, prm=None, camera=cam):
        a = np.asarray(ids_, np.int32)
        return L.msfm_register_images(h, _lib.C.byref(camera) if camera is not None else None, ip(a), len(a), _lib.C.byref(prm) if prm else None, None)

    assert rc(targets) == _lib.OK and L.msfm_fetch_registrations(h, None, None, None, None, None) == _lib.OK   # NULL params / outputs
    assert rc([targets[0], 4]) == _lib.E_NOIMAGE                                   # not declared
    assert rc([targets[0], targets[0]]) == _lib.E_INVALID                          # twice
    assert rc(targets, camera=None) == _lib.E_INVALID
    for bad in ((-1.0, 0.9999, 1024, 15, 10), (4.0, 1.0, 1024, 15, 10), (4.0, 0.9999, 0, 15, 10), (4.0, 0.9999, 1024, -1, 10),
                (4.0, 0.9999, 1024, 15, 101), (float("nan"), 0.9999, 1024, 15, 10)):
        assert rc(targets, _lib.RegisterParams(*bad, 0)) == _lib.E_INVALID, bad
    with pytest.raises(_lib.MsfmError) as e:                                       # a failed call leaves no registrations
        tctx.registrations()
    assert e.value.code == _lib.E_STATE
    tctx.tracks_end()
    assert rc(targets) == _lib.E_STATE


def test_image_without_keypoints(tctx):
    rng = np.random.default_rng(1)
    ids = np.asarray([2, 5, 8], np.int32)
    for i in ids:
        tctx.upload_image(int(i), rng.integers(0, 256, (6, 128), dtype=np.uint8))
        if i != 8:
            tctx.upload_keypoints(int(i), synth.keypoints(6, seed=int(i)))
    tctx.tracks_begin(ids, min_pair_matches=1)
    tctx.tracks_add(*fx.csr([((2, 5), [(0, 0), (1, 1)]), ((5, 8), [(0, 0)])]))
    tctx.tracks_finish()
    tctx.triangulate_tracks(CAM, scene_poses([2, 5]))
    with pytest.raises(_lib.MsfmError) as e:
        tctx.register_images(CAM, [8])
    assert e.value.code == _lib.E_NOIMAGE
    assert tctx.register_images(CAM, [2, 5])["attempted"] == 0


def test_more_images_than_the_round_kernel_has_workgroups(tctx, host):
    """1100 target images of 20 correspondences each in one call: the persistent grid (four workgroups per CU) wraps over the list."""
    n = 1100
    ids, kp, poses, targets, truth = small_session(tctx, [20] * n, seed=4)
    tctx.triangulate_tracks(CAM, poses)
    st, (rec, *_rest) = same(tctx, host, targets, kp)
    assert st["succeeded"] == n and st["images"] == n > 4 * 256
