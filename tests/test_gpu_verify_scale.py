"""The staged E / H verification and the model selection at production shapes, against the host twins (tests/verify_twin.py) and
the staging schedule (host_staged_schedule): thousands of pairs per call, so that the persistent grids of ve_round_kernel /
vh_round_kernel (grid = min(P, groups per CU x CUs), csrc/msfm_job.hip.h issue_rounds) walk their round lists more than twice,
staged_decide_kernel appends hundreds of pairs per round from many workgroups, and d_vf_hyp passes 2^32 bytes.  Every test checks
the lists bit for bit, the selection records, verification_stats() exactly (a walk that skips or repeats a listed pair may leave
the lists alone and change only the count) and the number of sub-batches; every precondition that makes a test bite (pairs listed
after round 0 against the grid, rounds run, sub-batches, buffer size) is asserted from the twin's schedule.  A sample of the pairs
is also compared with the independent numpy references (tests/emat_ref.py, tests/hmat_ref.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emat_ref  # noqa: E402
import hmat_ref  # noqa: E402
import verify_twin  # noqa: E402
from test_gpu_model_selection import check_one_of, same_rec  # noqa: E402
from test_gpu_verify_essential import BARREL, NO_DIST, camera, same, two_view  # noqa: E402

from monocularsfm_amd import _lib, synth  # noqa: E402

pytestmark = pytest.mark.gpu
kVeGroupsPerCU = 2   # ve_round_kernel workgroups per CU (csrc/msfm_verify_e.hip.h)
kVhGroupsPerCU = 8   # vh_round_kernel waves per CU (csrc/msfm_verify_h.hip.h)
ROUND_E, ROUND_H = 32, 64   # kVeRound, kVhRound
CAM = (2500.0, 2500.0, 1536.0, 1152.0)   # synth's camera
GIB = 1 << 30

# job A (E): low-inlier pairs (28-33 % of >= 40 matches: E never decides before max_iters = 200, 7 rounds, the last one with 8 live
# lanes) interleaved with high-inlier ones (decided in round 0), and pairs of n = 0 .. 6
A_PAIRS, A_ITERS = 1100, 200
# job B (H): synth.mixed_capture, all pairs of 28 facade and 100 scene images: 3-D and cross pairs run every H round of
# max_iters = 320 (5 rounds), most facade pairs decide in round 0
B_FACADE, B_SCENE, B_ITERS = 28, 100, 320
_cache = {}


def grids(ctx, P):
    cu = ctx.device_info()["cu_count"]
    assert cu > 0
    return min(P, kVeGroupsPerCU * cu), min(P, kVhGroupsPerCU * cu)


def job_a(dist):
    """-> (scenes, pairs, kind per pair: 0 low, 1 high, 2 tiny)"""
    key = ("a", dist)
    if key not in _cache:
        scenes, kind = [], []
        for s in range(A_PAIRS):
            scenes.append(two_view(12 + s % 4, 30, 4, seed=10000 + s, dist=dist))
            kind.append(0)
            scenes.append(two_view(60, 6, 4, seed=20000 + s, dist=dist))
            kind.append(1)
            if s % 150 == 75:   # n = 0 .. 6 spread over the list
                scenes.append(two_view(s // 150, 0, 6, seed=30000 + s, dist=dist))
                kind.append(2)
        pairs = np.array([(2 * s, 2 * s + 1) for s in range(len(scenes))], np.int32)
        _cache[key] = (scenes, pairs, np.asarray(kind))
    return _cache[key]


def upload_scenes(ctx, scenes, first=0):
    kps = {}
    for s, (dA, kA, dB, kB, _) in enumerate(scenes):
        for k, (d, kp) in enumerate(((dA, kA), (dB, kB))):
            ctx.upload_image(first + 2 * s + k, d)
            ctx.upload_keypoints(first + 2 * s + k, kp)
            kps[first + 2 * s + k] = kp
    return kps


def job_b():
    """-> (descs, kps, facade flag per image, pairs)"""
    if "b" not in _cache:
        descs, kps, facade = synth.mixed_capture(n_facade=B_FACADE, n_scene=B_SCENE, n_desc=200, seed=2024)
        _cache["b"] = (descs, kps, facade, synth.all_pairs(B_FACADE + B_SCENE))
    return _cache["b"]


def upload_images(ctx, descs, kps):
    for i, (d, k) in enumerate(zip(descs, kps)):
        ctx.upload_image(i, d)
        ctx.upload_keypoints(i, k)
    return dict(enumerate(kps))


def rounds_of(want, k=0):
    """the rounds of each pair's k-th staged model (0 for a pair below the sample size)"""
    return np.array([s[k][1] for s in want["schedule"]])


def check(ctx, got, want, sub_batches, records=None):
    assert same(got, want["lists"])
    if want["records"] is not None:
        assert same_rec(records, want["records"])
    assert ctx.verification_stats() == want["stats"], (ctx.verification_stats(), want["stats"])
    assert ctx.profile()["sub_batches"] == sub_batches


@pytest.fixture(scope="module")
def host(built_lib):
    return verify_twin.load_host()


@pytest.fixture(scope="module")
def ctx_a(built_lib):
    """job A without distortion, under model 1"""
    scenes, pairs, kind = job_a(NO_DIST)
    ctx = _lib.Context(0)
    kps = upload_scenes(ctx, scenes)
    raw = ctx.match_pairs(pairs)
    yield ctx, kps, pairs, kind, raw
    ctx.close()


@pytest.fixture(scope="module")
def ctx_b(built_lib):
    descs, kps, facade, pairs = job_b()
    ctx = _lib.Context(0)
    kps = upload_images(ctx, descs, kps)
    raw = ctx.match_pairs(pairs)
    yield ctx, kps, pairs, facade, raw
    ctx.close()


def reset(ctx, model, cam=None, select=False):
    ctx.set_limits()
    ctx.set_model_selection(select)
    ctx.set_verification_model(model, cam)


def assert_wraps_a(ctx, want, kind, raw, P, max_iters=A_ITERS):
    grid_e = grids(ctx, P)[0]
    R = rounds_of(want)
    last = -(-max_iters // ROUND_E)
    assert (R >= 2).sum() >= 2 * grid_e + 37, ((R >= 2).sum(), grid_e)         # round 1 .. : the walk's third trip
    assert (R == last).sum() >= 2 * grid_e + 37, ((R == last).sum(), grid_e)   # the last, partial round too
    assert (R[kind == 0] == last).mean() >= 0.95 and (R[kind == 1] == 1).all()
    assert set(range(7)) <= set(np.diff(raw[0])[kind == 2].tolist())


@pytest.mark.parametrize("dist", [NO_DIST, BARREL], ids=["pinhole", "barrel"])
def test_a_grid_wrap_essential(host, ctx_a, dist):
    if dist == NO_DIST:
        ctx, kps, pairs, kind, raw = ctx_a
        own = None
    else:
        scenes, pairs, kind = job_a(dist)
        ctx = own = _lib.Context(0)
        kps = upload_scenes(ctx, scenes)
        raw = ctx.match_pairs(pairs)
    try:
        cam = camera(dist)
        reset(ctx, 1, cam)
        want = verify_twin.run(host, raw, pairs, kps, 1, cam=cam, max_iters=A_ITERS)
        assert_wraps_a(ctx, want, kind, raw, len(pairs))
        assert want["stats"][1] == 7
        got = ctx.match_pairs_verified(pairs, max_iters=A_ITERS)
        check(ctx, got, want, 1)
    finally:
        if own is not None:
            own.close()


def assert_wraps_b(ctx, want, pairs, facade, max_iters=B_ITERS, k=0):
    grid_h = grids(ctx, len(pairs))[1]
    R = rounds_of(want, k)
    last = -(-max_iters // ROUND_H)
    assert (R >= 2).sum() >= 2 * grid_h + 37, ((R >= 2).sum(), grid_h)
    assert (R == last).sum() >= 2 * grid_h + 37, ((R == last).sum(), grid_h)
    ff = facade[pairs[:, 0]] & facade[pairs[:, 1]]
    assert (R[ff] == 1).mean() >= 0.9


def test_b_grid_wrap_homography(host, ctx_b):
    ctx, kps, pairs, facade, raw = ctx_b
    reset(ctx, 2)
    want = verify_twin.run(host, raw, pairs, kps, 2, max_iters=B_ITERS)
    assert_wraps_b(ctx, want, pairs, facade)
    assert want["stats"][1] == 5
    got = ctx.match_pairs_verified(pairs, max_iters=B_ITERS)
    check(ctx, got, want, 1)


@pytest.mark.parametrize("model", [0, 1])
def test_c_selection_at_scale(host, ctx_b, model):
    ctx, kps, pairs, facade, raw = ctx_b
    cam = CAM if model == 1 else None
    reset(ctx, 2)
    hom = ctx.match_pairs_verified(pairs, max_iters=B_ITERS)
    reset(ctx, model, cam)
    epi = ctx.match_pairs_verified(pairs, max_iters=B_ITERS)
    reset(ctx, model, cam, select=True)
    sel = ctx.match_pairs_verified(pairs, max_iters=B_ITERS)
    rec = ctx.model_selection(len(pairs))
    want = verify_twin.run(host, raw, pairs, kps, model, cam=cam, select=True, max_iters=B_ITERS)
    assert_wraps_b(ctx, want, pairs, facade, k=1 if model == 1 else 0)
    check(ctx, sel, want, 1, rec)
    check_one_of(sel, rec, epi, hom, model)
    ff = facade[pairs[:, 0]] & facade[pairs[:, 1]]
    took_h = rec[0] == 2   # (a few 3-D pairs of the capture whose views barely translate keep >= 70 % of their matches under H too)
    assert took_h[ff].mean() >= 0.9 and took_h[~ff].sum() <= 0.001 * (~ff).sum(), (int(took_h[ff].sum()), int(took_h[~ff].sum()))
    reset(ctx, 0)


EDGES_E = [dict(max_iters=m) for m in (1, 31, 32, 33)] + [dict(seed=0), dict(seed=(1 << 64) - 1), dict(threshold=0.0),
                                                          dict(threshold=1.0, confidence=0.999999)]
EDGES_H = [dict(max_iters=m) for m in (1, 63, 64, 65)] + [dict(seed=0), dict(seed=(1 << 64) - 1), dict(threshold=0.0),
                                                          dict(threshold=1.0, confidence=0.999999)]


@pytest.mark.parametrize("vkw", EDGES_E + [dict(max_iters=4096)], ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()))
def test_d_parameter_edges_essential(host, ctx_a, vkw):
    ctx, kps, pairs, kind, raw = ctx_a
    vkw = dict(dict(max_iters=A_ITERS), **vkw)
    if vkw["max_iters"] == 4096:   # a subset: 40 low- and 40 high-inlier pairs, and the tiny ones (twin time)
        sub = np.r_[np.arange(80), np.nonzero(kind == 2)[0]]
        pairs, kind = pairs[sub], kind[sub]
        raw = ctx.match_pairs(pairs)
    reset(ctx, 1, camera())
    want = verify_twin.run(host, raw, pairs, kps, 1, cam=camera(), **vkw)
    R = rounds_of(want)
    if vkw["max_iters"] == A_ITERS and "seed" in vkw:
        assert_wraps_a(ctx, want, kind, raw, len(pairs))
    elif vkw["max_iters"] == 4096:
        assert (R >= 32).sum() >= 35 and R.max() > 64   # 1000 hypotheses and more: the low-inlier pairs' bound comes down late
    else:   # every pair with >= 5 matches is listed in round 0, the walk wraps there
        assert (R >= 1).sum() >= 2 * grids(ctx, len(pairs))[0] + 37
    got = ctx.match_pairs_verified(pairs, **vkw)
    check(ctx, got, want, 1)


@pytest.mark.parametrize("vkw", EDGES_H + [dict(max_iters=4096)], ids=lambda v: "-".join("%s=%s" % kv for kv in v.items()))
def test_d_parameter_edges_homography(host, ctx_b, vkw):
    ctx, kps, pairs, facade, raw = ctx_b
    vkw = dict(dict(max_iters=B_ITERS), **vkw)
    reset(ctx, 2)
    want = verify_twin.run(host, raw, pairs, kps, 2, **vkw)
    R = rounds_of(want)
    grid_h = grids(ctx, len(pairs))[1]
    if vkw["max_iters"] in (B_ITERS, 4096) and vkw.get("threshold", 3.0) == 3.0:
        assert_wraps_b(ctx, want, pairs, facade, max_iters=vkw["max_iters"])
    else:
        assert (R >= 1).sum() >= 2 * grid_h + 37
    got = ctx.match_pairs_verified(pairs, **vkw)
    check(ctx, got, want, 1)


def job_e():
    """182 facade images of 140 keypoints (cheap: nearly all pairs decide in round 0) and two distinct low-inlier pairs at list positions a and
    a + 16384, whose rows of d_vf_hyp lie 2^32 bytes apart at max_iters = 65536"""
    if "e" not in _cache:
        descs, kps, _ = synth.mixed_capture(n_facade=182, n_scene=0, n_desc=140, seed=77)
        low = [two_view(6, 194, 4, seed=40001), two_view(6, 196, 4, seed=40002)]   # 3 % inliers: no bound below 65536
        _cache["e"] = (descs, kps, low)
    return _cache["e"]


@pytest.mark.parametrize("model,select", [(1, False), (2, False), (1, True)], ids=["E", "H", "E-select"])
def test_e_hypothesis_buffer_past_4_gib(host, model, select):
    import torch
    free = torch.cuda.mem_get_info()[0]
    assert free >= 16 * GIB, "test_e needs 16 GiB of free device memory, %.1f GiB free" % (free / GIB)
    descs, kps0, low = job_e()
    n_img = len(descs)
    base = synth.all_pairs(n_img)
    a = 40
    pairs = np.insert(base, a, (n_img, n_img + 1), axis=0)
    pairs = np.insert(pairs, a + 16384, (n_img + 2, n_img + 3), axis=0)
    P, max_iters = len(pairs), 1 << 16
    assert P >= 16400 and P * max_iters * 4 >= 1 << 32 and (a + 16384) * max_iters * 4 - a * max_iters * 4 == 1 << 32
    with _lib.Context(0) as ctx:
        kps = upload_images(ctx, descs, kps0)
        kps.update(upload_scenes(ctx, low, first=n_img))
        ctx.set_limits(max_pairs_per_batch=P)
        raw = ctx.match_pairs(pairs)
        cam = CAM if model == 1 else None
        ctx.set_verification_model(model, cam)
        ctx.set_model_selection(select)
        want = verify_twin.run(host, raw, pairs, kps, model, cam=cam, select=select, max_iters=max_iters)
        for k in range(2 if select else 1):
            R = rounds_of(want, k)
            last = max_iters // (ROUND_E if (model == 1 and k == 0) else ROUND_H)
            assert R[a] == last and R[a + 16384] == last, (R[a], R[a + 16384])
            assert np.delete(R, [a, a + 16384]).max() <= 16
        got = ctx.match_pairs_verified(pairs, max_iters=max_iters)
        check(ctx, got, want, 1, ctx.model_selection(P) if select else None)


def cuts(ctx, pairs, want, select, **vkw):
    P = len(pairs)
    limit = (P // 5) | 1
    n_sub = -(-P // limit)
    ctx.set_limits(max_pairs_per_batch=limit)
    got = ctx.match_pairs_verified(pairs, **vkw)
    check(ctx, got, want, n_sub, ctx.model_selection(P) if select else None)
    qts, ds, offs, recs, chunks = [], [], [0], [[], [], []], 0
    for ch in ctx.match_pairs_stream(pairs, verified=True, verify=vkw):
        chunks += 1
        qts.append(ch["qt"])
        ds.append(ch["dist"])
        offs += (offs[-1] + ch["offsets"][1:]).tolist()
        if select:
            for k in range(3):
                recs[k].append(ch["model_selection"][k])
    assert chunks == n_sub
    streamed = (np.asarray(offs, np.int64), np.concatenate(qts), np.concatenate(ds))
    check(ctx, streamed, want, n_sub, tuple(np.concatenate(r) for r in recs) if select else None)
    ctx.set_limits()


def test_f_cuts_and_streaming_essential(host, ctx_a):
    ctx, kps, pairs, kind, raw = ctx_a
    reset(ctx, 1, camera())
    want = verify_twin.run(host, raw, pairs, kps, 1, cam=camera(), max_iters=A_ITERS)
    assert_wraps_a(ctx, want, kind, raw, len(pairs))
    cuts(ctx, pairs, want, False, max_iters=A_ITERS)


def test_f_cuts_and_streaming_selection(host, ctx_b):
    ctx, kps, pairs, facade, raw = ctx_b
    reset(ctx, 1, CAM, select=True)
    want = verify_twin.run(host, raw, pairs, kps, 1, cam=CAM, select=True, max_iters=B_ITERS)
    assert want["stats"][1] == B_ITERS // ROUND_E   # (the larger of E's rounds and H's)
    cuts(ctx, pairs, want, True, max_iters=B_ITERS)
    reset(ctx, 0)


def test_g_independent_reference_on_a_sample(ctx_a, ctx_b):
    """8 pairs per model: E from job A (high-inlier pairs beyond the grid's first pass, and low-inlier pairs decided in the last
    round) against emat_ref.ransac (equal masks); H from job B (facade pairs and 3-D pairs that ran every round) against
    hmat_ref.ransac_mask (<= 2 differing matches)."""
    rng = np.random.default_rng(8)
    ctx, kps, pairs, kind, raw = ctx_a
    reset(ctx, 1, camera())
    grid_e = grids(ctx, len(pairs))[0]
    got = ctx.match_pairs_verified(pairs, max_iters=A_ITERS)
    far = np.arange(len(pairs)) >= 2 * grid_e
    pick = np.r_[rng.choice(np.nonzero(far & (kind == 1))[0], 6, replace=False), rng.choice(np.nonzero(far & (kind == 0))[0], 2, replace=False)]
    for p in pick:
        i, j = pairs[p]
        s, e = raw[0][p], raw[0][p + 1]
        p1, p2 = kps[i][raw[1][s:e, 0], :2].astype(np.float64), kps[j][raw[1][s:e, 1], :2].astype(np.float64)
        m = emat_ref.ransac(camera(), p1, p2, max_iters=A_ITERS)
        assert m is not None
        assert np.array_equal(got[1][got[0][p]:got[0][p + 1]], raw[1][s:e][m.astype(bool)]), p
    ctx, kps, pairs, facade, raw = ctx_b
    reset(ctx, 2)
    got = ctx.match_pairs_verified(pairs, max_iters=B_ITERS)
    grid_h = grids(ctx, len(pairs))[1]
    ff = facade[pairs[:, 0]] & facade[pairs[:, 1]]
    ss = ~facade[pairs[:, 0]] & ~facade[pairs[:, 1]]
    far = np.arange(len(pairs)) >= 2 * grid_h
    pick = np.r_[rng.choice(np.nonzero(ff)[0], 4, replace=False), rng.choice(np.nonzero(far & ss)[0], 4, replace=False)]
    for p in pick:
        i, j = pairs[p]
        s, e = raw[0][p], raw[0][p + 1]
        p1, p2 = kps[i][raw[1][s:e, 0], :2], kps[j][raw[1][s:e, 1], :2]
        m = hmat_ref.ransac_mask(p1.astype(np.float64), p2.astype(np.float64), max_iters=B_ITERS)
        assert m is not None
        dev = np.zeros(e - s, bool)
        kept = {tuple(r) for r in got[1][got[0][p]:got[0][p + 1]].tolist()}
        dev[:] = [tuple(r) in kept for r in raw[1][s:e].tolist()]
        assert (dev != m).sum() <= 2, (p, int((dev != m).sum()))
