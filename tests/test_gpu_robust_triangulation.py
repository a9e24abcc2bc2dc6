"""Robust track triangulation on the device (msfm_triangulate_tracks_robust / msfm_fetch_point_inliers,
csrc/msfm_triangulate_robust.hip.h) against the host twin (csrc/msfm_triangulate.h, TriangulateTracksRobust, through
tests/robust_triangulation_twin.py): records, residuals, inlier bytes and the counters of both stats BYTE FOR BYTE -- on a clean job
(where it must equal the plain call), without tracks, on the corrupted tracks of real verified calls, on hand-built tracks around the
LDS tile boundaries and the enumerated | sampled threshold, with more retried tracks than the retry launch has waves and with exactly
one; and on the routes off the easy path ("routes"): a later round's winner, no consensus on long tracks, hypotheses
rejected by depth alone, rejected refits and flipped bytes, the retry list's append patterns, an empty ballot word, one tile of a long
track, and the first kernel's second grid-stride pass.  There the twin's trace (robust_triangulation_twin.run(..., trace=True)) is
asserted next to every byte comparison: a comparison proves nothing about a branch the input does not reach.  The twin itself is
checked against the independent numpy reference in tests/test_robust_triangulation_reference.py."""
import numpy as np
import pytest

import registration_twin as regtw
import robust_triangulation_twin as rtw
import test_robust_triangulation_reference as rb
import test_triangulation_reference as tb
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


def ring_job(lengths, outlier=None, rows=None, noise_px=0.3, seed=3, moved=None, turned=()):
    """Hand-built tracks: track j runs through the images 0 .. lengths[j] - 1 at keypoint row j; cameras 1.2 degrees apart on a circle
    around the scene; outlier: {track: position} moved by 40 px; moved: {track: [(position, dx, dy), ...]}, each observation by its own
    offset; turned: the images whose camera is turned round (half a turn about its own y axis: the scene lies behind it, its
    keypoints are the scene's image through the turned camera).  -> (ids, kps, poses, the list for tracks_add)"""
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
        if i in turned:
            R, t = np.diag([-1.0, 1.0, -1.0]) @ R, np.diag([-1.0, 1.0, -1.0]) @ t
        k = synth.keypoints(rows, seed=seed + i)
        Y = X @ R.T + t
        k[:n_tr, 0] = (CAM[0] * Y[:, 0] / Y[:, 2] + CAM[2] + rng.normal(0, noise_px, n_tr)).astype(np.float32)
        k[:n_tr, 1] = (CAM[1] * Y[:, 1] / Y[:, 2] + CAM[3] + rng.normal(0, noise_px, n_tr)).astype(np.float32)
        kps.append(k)
        poses[int(ids[i])] = (R, t)
    for j, pos in (outlier or {}).items():
        kps[pos][j, 0] += np.float32(40.0)
    for j, obs in (moved or {}).items():
        for pos, dx, dy in obs:
            kps[pos][j, 0] += np.float32(dx)
            kps[pos][j, 1] += np.float32(dy)
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


# ---- the routes off the easy path -----------------------------------------------------------------------------------------------------
def traced(ctx, host, ids, kps, poses, cam=CAM, params=rtw.DEFAULTS, tracks=None):
    """same(...), and the twin's trace of the same call"""
    tracks = ctx.tracks() if tracks is None else tracks
    out = same(ctx, host, ids, kps, poses, cam, params, tracks)
    return out + (rtw.run(host, tracks, ids, kps, poses, cam, params, trace=True)[4],)


def scattered(rng, positions, lo, hi):
    """an offset of its own for every position: length uniform in [lo, hi] px, direction uniform"""
    out = []
    for pos in positions:
        r, a = rng.uniform(lo, hi), rng.uniform(0.0, 2.0 * np.pi)
        out.append((int(pos), r * np.cos(a), r * np.sin(a)))
    return out


LATE_SEED = 4    # (searched on the CPU with the twin: the winners asserted below)


def late_job(seed=LATE_SEED):
    """three tracks each of 65, 130 and 300 elements with 60 - 75 % of the observations moved, each by its own 25 .. 120 px, between
    tracks with one outlier (round 0 wins there): 18 tracks, so that late and early winners share workgroups of four waves"""
    rng = np.random.default_rng(seed)
    lengths, moved, late = [], {}, []
    for m in (65, 130, 300) * 3:
        k = int(round(rng.uniform(0.62, 0.73) * m))
        late.append(len(lengths))
        moved[len(lengths)] = scattered(rng, np.sort(rng.choice(m, k, replace=False)), 25.0, 120.0)
        lengths.append(m)
        moved[len(lengths)] = [(int(rng.integers(0, 7)), 40.0, 0.0)]
        lengths.append(7)
    return lengths, moved, late


def test_a_later_round_wins(tctx, host):
    """`if (wc > best)` with h0 >= 64 and the shuffle from lane wh - h0: winners in round 1, in round 2 and later, and in the last,
    partial round of H = 65 (hypothesis 64, lane 0 of a round with one live lane).  max_error 0.6 px against 0.3 px of noise: the
    clean pairs' counts differ, so the first clean pair seldom wins."""
    lengths, moved, late = late_job()
    ids, kps, poses, lst = ring_job(lengths, moved=moved)
    open_ring(tctx, ids, kps, lst, len(lengths))
    tracks = tctx.tracks()
    winners = []
    for H in (65, 128, 1024):
        st, pts, res, mask, tr = traced(tctx, host, ids, kps, poses, params=(0.6, 1.5, 2, H), tracks=tracks)
        assert st["retried"] == len(lengths) and np.all(tr["retried"] == 1)
        assert np.all(pts["status"][late] & _lib.TRI_POINT) and np.all(tr["winner"][1::2] < 64)   # (the one-outlier tracks: round 0)
        winners += [(H, int(w)) for w in tr["winner"][late]]
    print("winners (H, hypothesis): %s" % winners)
    assert len(late) >= 9 and sum(w >= 64 for _, w in winners) >= 3 and sum(w >= 128 for _, w in winners) >= 1
    assert any(H == 65 and w == 64 for H, w in winners)
    tctx.tracks_end()


NONE_SEED = 0    # (checked on the CPU with the twin: no three observations agree in any of the four calls)
NONE_N = (3, 64, 65, 130, 200)


def none_job(seed=NONE_SEED):
    """tracks of 3, 64, 65, 130, 200 elements with every observation but two moved by its own 150 .. 900 px (no three agree), twice
    each, between clean tracks"""
    rng = np.random.default_rng(seed)
    lengths, moved, bad = [], {}, []
    for n in NONE_N * 2:
        keep = (n // 3, n - 2) if n > 3 else (0, 2)
        bad.append(len(lengths))
        moved[len(lengths)] = scattered(rng, [p for p in range(n) if p not in keep], 150.0, 900.0)
        lengths += [n, 5]
    return lengths, moved, bad


def test_no_consensus_clears_long_tracks(tctx, host):
    """best < need with n > 64: the clearing loop over all of the track's elements, the elements of unposed images in every ballot
    word among them (0, 63, 64, 127, 128 and the last elements unposed).  min_views = 3 where no three observations agree (the trace:
    valid hypotheses, a best count below 3), and min_angle = 170 where no hypothesis is valid."""
    lengths, moved, bad = none_job()
    ids, kps, poses, lst = ring_job(lengths, moved=moved)
    open_ring(tctx, ids, kps, lst, len(lengths))
    tracks = tctx.tracks()
    o = tracks[0]
    gone = {0, 63, 64, 127, 128, 129, 199}
    some = {i: (None if k in gone else p) for k, (i, p) in enumerate(sorted(poses.items()))}
    for ps in (poses, some):
        for prm in ((2.0, 1.5, 3, 64), (2.0, 170.0, 2, 64)):
            st, pts, res, mask, tr = traced(tctx, host, ids, kps, ps, params=prm, tracks=tracks)
            hit = [t for t in bad if tr["retried"][t]]
            assert len(hit) >= len(bad) - 2 and {int(o[t + 1] - o[t]) for t in hit} >= {64, 65, 130, 200}
            for t in hit:
                assert tr["mask1"][t] == -1 and ((tr["valid"][t] > 0 and 0 <= tr["best"][t] < 3) if prm[2] == 3 else tr["best"][t] == -1)
                assert int(pts["status"][t]) == _lib.TRI_ATTEMPTED | _lib.TRI_ROBUST and pts[t].tobytes()[4:] == bytes(44)
                assert not mask[o[t]:o[t + 1]].any() and np.all(res[o[t]:o[t + 1]] == -1.0)
            rest = [t for t in range(len(lengths)) if t not in bad]
            assert st["rescued"] == 0 and st["observations_rejected"] == 0 and st["retried"] == len(hit) + int(tr["retried"][rest].sum())
    tctx.tracks_end()


def laid_out(tracks, rows=2):
    """Tracks with cameras of their own: tracks[j] = (poses per element [(R, t) or None], pixels float32 [n, 2]); every element gets an
    image of its own (row 0 is the observation), in element order.  -> (ids, kps, poses, the list for tracks_add)"""
    total = sum(len(p) for p, _ in tracks)
    ids = np.arange(total, dtype=np.int32) * 3 + 1
    kps, poses, pairs = [], {}, []
    at = 0
    for ps, xy in tracks:
        for k, pose in enumerate(ps):
            kp = synth.keypoints(rows, seed=at + k)
            kp[0, :2] = np.asarray(xy[k], np.float32)
            kps.append(kp)
            if pose is not None:
                poses[int(ids[at + k])] = pose
            if k:
                pairs.append((ids[at + k - 1], ids[at + k]))
        at += len(ps)
    lst = (np.asarray(pairs, np.int32).reshape(-1, 2), np.arange(len(pairs) + 1, dtype=np.int64), np.zeros((len(pairs), 2), np.int32))
    return ids, kps, poses, lst


def as_laid(one, kps, poses):
    """a one-track result of the reference tests -> laid_out's track"""
    img, idx = one[1], one[2]
    return [poses.get(int(i)) for i in img], np.asarray([kps[int(i)][int(r), :2] for i, r in zip(img, idx)], np.float32)


def test_depth_only_rejects_and_rejected_refits(tctx, host):
    """The tracks of tests/test_robust_triangulation_reference.py for the depth line (a camera turned round), the rejected refit and
    the flipped bytes (a noisy capture's tracks, chosen by the twin's trace), and the identical-camera tracks of
    tests/test_triangulation_reference.py (a rank-2 normal matrix), each with cameras of its own."""
    c = rb.long_capture(CAM)
    laid = [as_laid(*rb.depth_job(c, *d)) for d in rb.DEPTH[CAM]]
    n_depth = len(laid)
    n = tb.capture(5, noise_px=1.0)
    tr = rtw.run(host, n["tracks"], n["ids"], n["kps"], n["poses"], CAM, trace=True)[4]
    lost = (tr["flipped"] - (tr["mask2"] - tr["mask1"])) // 2
    short = np.diff(n["tracks"][0]) <= 11                       # (55 pairs at most: enumerated, whatever the track's number)
    kinds = [short & (tr["mask1"] >= 0) & (tr["refit_stood"] == 0) & (tr["mask2"] < tr["mask1"]), short & (tr["refit_stood"] == 1) & (lost > 0),
             short & (tr["refit_stood"] == 1) & (tr["flipped"] - lost > 0)]
    o, img, idx, _ = n["tracks"]
    for kind in kinds:
        pick = np.nonzero(kind)[0][:3]
        assert len(pick) == 3
        laid += [as_laid((None, img[o[t]:o[t + 1]], idx[o[t]:o[t + 1]]), n["kps"], n["poses"]) for t in pick]
    laid += tb.identical_tracks()
    ids, kps, poses, lst = laid_out(laid)
    ts = open_ring(tctx, ids, kps, lst, 2)
    assert ts["tracks_kept"] == len(laid)
    st, pts, res, mask, tr = traced(tctx, host, ids, kps, poses)
    d = tr[:n_depth]
    assert np.all(d["retried"] == 1) and np.all(d["depth_rejected"] >= 1) and np.all(d["depth_rejected_best"] >= np.maximum(d["best"], 2))
    r = tr[n_depth:n_depth + 9]
    lost = (r["flipped"] - (r["mask2"] - r["mask1"])) // 2
    assert np.all(r["retried"] == 1) and np.all((r["refit_stood"][:3] == 0) & (r["mask2"][:3] < r["mask1"][:3]) & (r["mask2"][:3] >= 0))
    assert np.all((r["refit_stood"][3:] == 1) & (r["flipped"][3:] > 0)) and np.all(lost[3:6] > 0) and np.all((r["flipped"] - lost)[6:] > 0)
    for p in pts[n_depth + 9:]:                                # identical cameras and pixels: what the definition fixes
        s = int(p["status"])
        assert s & _lib.TRI_ATTEMPTED and not s & _lib.TRI_ANGLE_OK and (not s & _lib.TRI_POINT or np.all(np.isfinite(p["X"])))
    tctx.tracks_end()


@pytest.mark.parametrize("T", [63, 64, 65, 257])
def test_first_kernel_wave_patterns(tctx, host, T):
    """The retry list's append within one wave: every lane retried (a full ballot), lane 0 only, lane 63 only, every other lane, the
    last track only -- with a last wave that lies partly beyond T."""
    every, alt = list(range(T)), list(range(0, T, 2))
    for planted in (every, [0], [63] if T > 63 else [T - 1], alt, [T - 1]):
        ids, kps, poses, lst = ring_job([3] * T, {j: j % 3 for j in planted})
        open_ring(tctx, ids, kps, lst, T)
        st, pts, _, _ = same(tctx, host, ids, kps, poses)
        assert st["retried"] == len(planted) and st["hypotheses"] == 3 * len(planted)
        assert np.nonzero(pts["status"] & _lib.TRI_ROBUST)[0].tolist() == planted
        tctx.tracks_end()


def test_empty_ballot_word_and_one_tile_of_long_tracks(tctx, host):
    """Position compaction: n = 192 with the elements 64 .. 127 all unposed (the middle ballot word is 0), and n = 130 with exactly 64
    posed elements spread over all three words (one tile although n > 64); one moved observation in the last word of each."""
    ids, kps, poses, lst = ring_job([192, 130, 192, 130, 7], {0: 150, 1: 129, 2: 191, 3: 128})
    open_ring(tctx, ids, kps, lst, 5)
    tracks = tctx.tracks()
    by_pos = sorted(poses.items())
    middle = {i: (None if 64 <= k < 128 else p) for k, (i, p) in enumerate(by_pos)}
    st, pts, res, mask, tr = traced(tctx, host, ids, kps, middle, tracks=tracks)
    assert tr["m"].tolist() == [128, 66, 128, 66, 7] and tr["retried"].tolist() == [1, 1, 1, 1, 0]
    assert pts["n_views"].tolist() == [127, 65, 127, 65, 7] and np.all(_lib.succeeded(pts))
    keep = set(range(0, 62, 2)) | set(range(64, 126, 2)) | {128, 129}          # 31 + 31 + 2 of the first 130
    spread = {i: (p if k in keep or k >= 130 else None) for k, (i, p) in enumerate(by_pos)}
    st, pts, res, mask, tr = traced(tctx, host, ids, kps, spread, tracks=tracks)
    assert tr["m"][[1, 3]].tolist() == [64, 64] and tr["retried"][[1, 3]].tolist() == [1, 1] and pts["n_views"][[1, 3]].tolist() == [63, 63]
    assert np.all(_lib.succeeded(pts[[1, 3]])) and mask[tracks[0][1] + 129] == 0 and mask[tracks[0][3] + 128] == 0
    tctx.tracks_end()


def second_pass_job(T, rows=8192, seed=7):
    """T tracks of length 3 over triples of `rows`-keypoint images: track g * rows + r runs through row r of the images 3 g, 3 g + 1,
    3 g + 2, whose cameras stand 2.4 degrees apart; one observation moved by 40 px in every third track and in every track of the
    last 8192.  -> (ids, kps, poses, lists for tracks_add)"""
    rng = np.random.default_rng(seed)
    groups = (T + rows - 1) // rows
    ids = np.arange(3 * groups, dtype=np.int32) * 3 + 1
    kps, poses, lists = [], {}, []
    tno = np.arange(rows)
    for g in range(groups):
        n = min(rows, T - g * rows)
        X = rng.uniform(-1.0, 1.0, (rows, 3))
        t_abs = g * rows + tno
        hit = ((t_abs % 3 == 0) | (t_abs >= T - 8192)) & (tno < n)
        for k in range(3):
            th = 2 * np.pi * (2 * k) / 300.0
            z = np.asarray([-np.sin(th), 0.0, np.cos(th)])
            x = np.cross([0.0, 1.0, 0.0], z)
            R, t = np.stack([x, np.cross(z, x), z]), np.asarray([0.0, 0.02 * k, 6.5])
            kp = synth.keypoints(rows, seed=seed + 3 * g + k)
            Y = X @ R.T + t
            kp[:, 0] = (CAM[0] * Y[:, 0] / Y[:, 2] + CAM[2] + rng.normal(0, 0.3, rows)).astype(np.float32)
            kp[:, 1] = (CAM[1] * Y[:, 1] / Y[:, 2] + CAM[3] + rng.normal(0, 0.3, rows)).astype(np.float32)
            kp[hit & (t_abs % 3 == k), 0] += np.float32(40.0)
            kps.append(kp)
            poses[int(ids[3 * g + k])] = (R, t)
        q = np.stack([tno[:n], tno[:n]], 1).astype(np.int32)
        lists.append((np.asarray([(ids[3 * g], ids[3 * g + 1]), (ids[3 * g + 1], ids[3 * g + 2])], np.int32), np.asarray([0, n, 2 * n], np.int64),
                      np.concatenate([q, q])))
    return ids, kps, poses, lists


def test_first_kernel_second_pass(tctx, host):
    """trr_first_kernel's grid holds 8 x CUs x 256 lanes: with 8192 tracks more, its first 32 workgroups run a second pass of the
    wave-uniform t0 loop and append to the retry list from it (every track of the last 8192 is retried)."""
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
    ts = tctx.tracks_finish()
    assert ts["tracks_kept"] == T and ts["longest_track"] == 3
    st, pts, res, mask = same(tctx, host, ids, kps, poses)
    planted = sum(1 for t in range(T) if t % 3 == 0 or t >= T - 8192)
    assert st["retried"] == planted and np.all(pts["status"][T - 8192:] & _lib.TRI_ROBUST)
    print("second pass: T %d, triangulate_ms %.3f, robust_ms %.3f" % (T, st["triangulate_ms"], st["robust_ms"]))
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
