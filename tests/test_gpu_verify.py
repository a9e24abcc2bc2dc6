"""Batched device RANSAC (msfm_match_pairs_verified = matching + FeatureUtils::FilterMatches) against its host
twin (host/GeometricVerification.cpp through libmsfm_host.so): the two share the fp64 arithmetic of
csrc/msfm_fmat.h, the sampling stream and the adaptive stopping rule, so the verified lists must be IDENTICAL;
on data with a true epipolar geometry the inliers must be recovered.  (Not a parity claim against OpenCV's
findFundamentalMat -- SURVEY.md 8a-a13.)"""
import ctypes as C
import os

import numpy as np
import pytest

from monocularsfm_amd import synth
from oracle import fmat_ref

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(built_lib):
    L = C.CDLL(os.path.join(ROOT, "monocularsfm_amd", "host", "libmsfm_host.so"))
    L.host_fundamental_ransac.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_ubyte)]
    L.host_fundamental_ransac_ex.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_double, C.c_double,
                                             C.c_int, C.c_ulonglong, C.POINTER(C.c_ubyte)]
    return L


def host_mask(host, p1, p2):
    p1 = np.ascontiguousarray(p1, F32)
    p2 = np.ascontiguousarray(p2, F32)
    mask = np.zeros(max(len(p1), 1), np.uint8)
    fp = C.POINTER(C.c_float)
    n = host.host_fundamental_ransac(p1.ctypes.data_as(fp), p2.ctypes.data_as(fp), len(p1), mask.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return mask[:n].astype(bool) if n else np.zeros(len(p1), bool)


def host_mask_ex(host, p1, p2, threshold=3.0, confidence=0.99, max_iters=1000, seed=0x5eed5eed):
    p1 = np.ascontiguousarray(p1, F32)
    p2 = np.ascontiguousarray(p2, F32)
    mask = np.zeros(max(len(p1), 1), np.uint8)
    fp = C.POINTER(C.c_float)
    n = host.host_fundamental_ransac_ex(p1.ctypes.data_as(fp), p2.ctypes.data_as(fp), len(p1), threshold, confidence,
                                        max_iters, seed, mask.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return mask[:n].astype(bool) if n else np.zeros(len(p1), bool)


def two_view_scene(n_in, n_out, n_extra, seed, noise=0.4):
    """Two images whose descriptors match one-to-one on the first n_in + n_out rows (in shuffled order); the
    first n_in correspondences obey one epipolar geometry, the n_out others have random keypoints."""
    rng = np.random.default_rng(seed)
    n = n_in + n_out
    base = synth.rootsift_images(1, [n + 2 * n_extra], seed=seed, n_proto=4 * (n + 2 * n_extra) + 64)[0]
    dA = np.r_[base[:n], base[n:n + n_extra]]
    nb = np.abs(base[:n] + rng.normal(0, 0.004, (n, 128)).astype(F32))
    nb /= np.linalg.norm(nb, axis=1, keepdims=True)
    dB = np.r_[nb.astype(F32), base[n + n_extra:]]
    X = np.c_[rng.uniform(-2, 2, n_in), rng.uniform(-1.5, 1.5, n_in), rng.uniform(4, 9, n_in)]
    K = np.array([[2559.68, 0, 1536], [0, 2559.68, 1152], [0, 0, 1]])
    a = 0.1 + 0.1 * rng.random()
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t = np.array([0.8, 0.05, 0.1]) * (0.5 + rng.random())
    x1 = (K @ X.T).T
    x1 = x1[:, :2] / x1[:, 2:]
    x2 = (K @ (R @ X.T + t[:, None])).T
    x2 = x2[:, :2] / x2[:, 2:]
    x1 += rng.normal(0, noise, x1.shape)
    x2 += rng.normal(0, noise, x2.shape)
    rnd = lambda m: np.c_[rng.uniform(0, 3072, m), rng.uniform(0, 2304, m)]
    kA = np.r_[x1, rnd(n_out + n_extra)]
    kB = np.r_[x2, rnd(n_out + n_extra)]
    pa, pb = rng.permutation(len(dA)), rng.permutation(len(dB))
    kpA = np.c_[kA[pa], np.full(len(pa), 3.0), np.zeros(len(pa))].astype(F32)   # Database layout: x, y, size, angle
    kpB = np.c_[kB[pb], np.full(len(pb), 3.0), np.zeros(len(pb))].astype(F32)
    true_rows_A = np.zeros(len(dA), bool)
    true_rows_A[:n_in] = True
    return dA[pa].astype(F32), kpA, dB[pb].astype(F32), kpB, true_rows_A[pa]


def expected_lists(ctx, host, pairs, kps, **kw):
    offs, qt, d = ctx.match_pairs(pairs, **kw)
    out_q, out_d, out_off = [], [], [0]
    for p, (i, j) in enumerate(pairs):
        s, e = offs[p], offs[p + 1]
        q, t = qt[s:e, 0], qt[s:e, 1]
        keep = host_mask(host, kps[i][q, :2], kps[j][t, :2]) if e > s else np.zeros(0, bool)
        out_q.append(qt[s:e][keep])
        out_d.append(d[s:e][keep])
        out_off.append(out_off[-1] + int(keep.sum()))
    return np.asarray(out_off, np.int64), np.concatenate(out_q).reshape(-1, 2), np.concatenate(out_d), (offs, qt)


def test_verified_lists_equal_the_host_twin_and_recover_the_geometry(gpu_ctx, host):
    scenes = [two_view_scene(300, 120, 200, seed=3), two_view_scene(200, 120, 100, seed=4), two_view_scene(900, 50, 50, seed=5, noise=1.0)]
    descs, kps, truth = [], [], []
    for dA, kA, dB, kB, tr in scenes:
        descs += [dA, dB]
        kps += [kA, kB]
        truth.append(tr)
    for i, (dd, kk) in enumerate(zip(descs, kps)):
        gpu_ctx.upload_image(i, dd)
        gpu_ctx.upload_keypoints(i, kk)
    # the three true pairs (both orientations of the first), plus unrelated pairs (no consensus expected)
    pairs = np.array([(0, 1), (1, 0), (2, 3), (4, 5), (0, 3), (2, 5), (4, 1)], np.int32)
    exp_off, exp_qt, exp_d, (raw_off, raw_qt) = expected_lists(gpu_ctx, host, pairs, kps)
    offs, qt, d = gpu_ctx.match_pairs_verified(pairs)
    prof = gpu_ctx.profile()
    assert np.array_equal(offs, exp_off) and np.array_equal(qt, exp_qt) and np.array_equal(d.view(np.int32), exp_d.view(np.int32))
    assert prof["verify_ms"] > 0
    # geometry: the true correspondences survive, the planted false ones do not
    for p, sc in ((0, 0), (2, 1), (3, 2)):
        q = qt[offs[p]:offs[p + 1], 0]
        rq = raw_qt[raw_off[p]:raw_off[p + 1], 0]
        tr = truth[sc]
        assert tr[q].sum() >= 0.9 * tr[rq].sum() > 20
        assert (~tr[q]).sum() <= 0.15 * max(1, (~tr[rq]).sum())
    for p in (4, 5, 6):   # unrelated images: whatever matched by accident has no common geometry
        assert offs[p + 1] - offs[p] <= 12


@pytest.mark.parametrize("n_match", [0, 3, 6, 7, 8, 9, 20])
def test_small_match_counts_follow_findFundamentalMat_cases(gpu_ctx, host, n_match):
    """0 matches -> nothing; < 7 -> no model -> nothing; exactly 7 -> all kept; >= 8 -> RANSAC."""
    dA, kA, dB, kB, _ = two_view_scene(n_match, 0, 40, seed=100 + n_match, noise=0.1) if n_match else two_view_scene(0, 0, 40, seed=100)
    gpu_ctx.upload_image(0, dA)
    gpu_ctx.upload_image(1, dB)
    gpu_ctx.upload_keypoints(0, kA)
    gpu_ctx.upload_keypoints(1, kB)
    pairs = np.array([(0, 1)], np.int32)
    exp_off, exp_qt, exp_d, (raw_off, _) = expected_lists(gpu_ctx, host, pairs, [kA, kB])
    offs, qt, d = gpu_ctx.match_pairs_verified(pairs)
    assert np.array_equal(offs, exp_off) and np.array_equal(qt, exp_qt)
    n_raw = int(raw_off[1])
    if n_raw < 7:
        assert offs[1] == 0
    elif n_raw == 7:
        assert offs[1] == 7
    elif n_match >= 8 and n_raw == n_match:
        assert offs[1] >= n_match - 1     # clean geometry: (almost) everything is an inlier


def test_parameters_and_errors(gpu_ctx, host):
    dA, kA, dB, kB, _ = two_view_scene(200, 200, 50, seed=9)
    gpu_ctx.upload_image(0, dA)
    gpu_ctx.upload_image(1, dB)
    from monocularsfm_amd import _lib
    with pytest.raises(_lib.MsfmError):                      # no keypoints yet (upload_image resets them)
        gpu_ctx.match_pairs_verified(np.array([(0, 1)], np.int32))
    gpu_ctx.upload_keypoints(0, kA)
    gpu_ctx.upload_keypoints(1, kB)
    a = gpu_ctx.match_pairs_verified(np.array([(0, 1)], np.int32))
    b = gpu_ctx.match_pairs_verified(np.array([(0, 1)], np.int32))
    assert np.array_equal(a[1], b[1])                          # deterministic
    loose = gpu_ctx.match_pairs_verified(np.array([(0, 1)], np.int32), threshold=30.0)
    tight = gpu_ctx.match_pairs_verified(np.array([(0, 1)], np.int32), threshold=0.05)
    assert loose[0][1] >= a[0][1] >= tight[0][1]
    few = gpu_ctx.match_pairs_verified(np.array([(0, 1)], np.int32), max_iters=3, seed=7)
    assert few[0][1] <= a[0][1] + 5
    with pytest.raises(_lib.MsfmError):
        gpu_ctx.match_pairs_verified(np.array([(0, 1)], np.int32), confidence=1.5)
    with pytest.raises(_lib.MsfmError):
        gpu_ctx.upload_keypoints(0, kA[:10])                   # fewer keypoints than descriptor rows


# ---- against host_fundamental_ransac_ex and oracle/fmat_ref.py ------------------------------------------------------
def copy_scene(n, seed, outliers=0.3, noise=0.5, coords=None):
    """Two views of n rows whose descriptors are the same rows in another order, so every row matches its copy and
    the pair hands exactly n matches to the verification; the first (1 - outliers) n keypoint pairs (in row order of
    the first view) obey one epipolar geometry.  coords: (k1, k2) keypoint coordinates to use instead."""
    rng = np.random.default_rng(seed)
    d = synth.rootsift_images(1, [n], seed=seed, n_proto=max(64, n))[0] if n else np.zeros((0, 128), F32)
    if coords is None:
        n_in = int(round(n * (1 - outliers)))
        X = np.c_[rng.uniform(-2, 2, n_in), rng.uniform(-1.5, 1.5, n_in), rng.uniform(4, 9, n_in)]
        K = np.array([[2559.68, 0, 1536], [0, 2559.68, 1152], [0, 0, 1]])
        a = 0.15
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        x1 = (K @ X.T).T
        x1 = x1[:, :2] / x1[:, 2:] + rng.normal(0, noise, (n_in, 2))
        x2 = (K @ (R @ X.T + np.array([[0.8], [0.05], [0.1]]))).T
        x2 = x2[:, :2] / x2[:, 2:] + rng.normal(0, noise, (n_in, 2))
        rnd = lambda m: np.c_[rng.uniform(0, 3072, m), rng.uniform(0, 2304, m)]
        k1, k2 = np.r_[x1, rnd(n - n_in)], np.r_[x2, rnd(n - n_in)]
    else:
        k1, k2 = coords
    perm = rng.permutation(n)
    kp1 = np.c_[k1, np.full(n, 3.0), np.zeros(n)].astype(F32)
    kp2 = np.c_[np.asarray(k2)[perm], np.full(n, 3.0), np.zeros(n)].astype(F32)
    return d, kp1, np.ascontiguousarray(d[perm]), kp2


def upload(ctx, images):
    for i, (d, k) in enumerate(images):
        ctx.upload_image(i, d)
        ctx.upload_keypoints(i, k)


def expected_lists_ex(ctx, host, pairs, kps, **vp):
    """match_pairs + host_fundamental_ransac_ex on every pair with the verification parameters vp."""
    offs, qt, d = ctx.match_pairs(pairs)
    out_q, out_d, out_off = [], [], [0]
    for p, (i, j) in enumerate(pairs):
        s, e = offs[p], offs[p + 1]
        q, t = qt[s:e, 0], qt[s:e, 1]
        keep = host_mask_ex(host, kps[i][q, :2], kps[j][t, :2], **vp) if e > s else np.zeros(0, bool)
        out_q.append(qt[s:e][keep])
        out_d.append(d[s:e][keep])
        out_off.append(out_off[-1] + int(keep.sum()))
    return np.asarray(out_off, np.int64), np.concatenate(out_q).reshape(-1, 2), np.concatenate(out_d), (offs, qt)


def assert_same(got, exp):
    assert np.array_equal(got[0], exp[0])
    assert np.array_equal(got[1], exp[1])
    assert np.array_equal(np.asarray(got[2], F32).view(np.int32), np.asarray(exp[2], F32).view(np.int32))


PARAM_GRID = ([dict(threshold=t, confidence=c) for t in (0.05, 1.0, 3.0, 30.0) for c in (0.5, 0.99, 0.999999)]
              + [dict(max_iters=m, seed=s) for m in (1, 7, 255, 256, 257, 1000, 4096) for s in (0, 7, (1 << 64) - 1)]
              + [dict(threshold=1.0, confidence=0.999999, max_iters=4096, seed=(1 << 64) - 1),
                 dict(threshold=30.0, confidence=0.5, max_iters=257, seed=0)])


def test_parameter_grid_equals_the_twin_bit_for_bit(gpu_ctx, host):
    """threshold, confidence, max_iters and seed each reach the device exactly as the host twin uses them."""
    imgs = [copy_scene(400, 31, outliers=0.5), copy_scene(120, 32, outliers=0.2), copy_scene(60, 33, outliers=0.7)]
    upload(gpu_ctx, [x for d1, k1, d2, k2 in imgs for x in ((d1, k1), (d2, k2))])
    kps = [k for d1, k1, d2, k2 in imgs for k in (k1, k2)]
    pairs = np.array([(0, 1), (2, 3), (4, 5), (0, 3)], np.int32)
    kept = set()
    for vp in PARAM_GRID:
        exp = expected_lists_ex(gpu_ctx, host, pairs, kps, **vp)
        got = gpu_ctx.match_pairs_verified(pairs, **vp)
        assert_same(got, exp[:3])
        kept.add(tuple(np.diff(got[0])))
    assert len(kept) >= 8     # the parameters change the outcome


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097, 6000])
def test_lds_chunk_edges(gpu_ctx, host, n):
    """vf_hypotheses_kernel stages the matches in chunks of 2048: pairs that end just before, on and after a chunk
    edge, and pairs of three chunks."""
    d1, k1, d2, k2 = copy_scene(n, 50 + n, outliers=0.4)
    upload(gpu_ctx, [(d1, k1), (d2, k2)])
    pairs = np.array([(0, 1)], np.int32)
    exp = expected_lists_ex(gpu_ctx, host, pairs, [k1, k2])
    assert exp[3][0][1] == n                       # the verification sees exactly n matches
    got = gpu_ctx.match_pairs_verified(pairs)
    assert_same(got, exp[:3])
    assert got[0][1] >= 0.5 * n


def test_mixed_batch_sub_batches_and_stream(gpu_ctx, host):
    """One batch of pairs with 0, 6, 7, 8, 9 ... 2100 matches: one call, sub-batches of at most 3 pairs, and the
    streaming series all give the twin's lists."""
    sizes = [6, 7, 8, 9, 2100, 40, 300, 7, 9, 1200]
    imgs = [copy_scene(n, 70 + i, outliers=0.25) for i, n in enumerate(sizes)]
    upload(gpu_ctx, [x for d1, k1, d2, k2 in imgs for x in ((d1, k1), (d2, k2))])
    kps = [k for d1, k1, d2, k2 in imgs for k in (k1, k2)]
    pairs = np.array([(2 * i, 2 * i + 1) for i in range(len(sizes))] + [(0, 3), (9, 4)], np.int32)
    exp = expected_lists_ex(gpu_ctx, host, pairs, kps)
    assert list(np.diff(exp[3][0])[:len(sizes)]) == sizes
    whole = gpu_ctx.match_pairs_verified(pairs)
    assert_same(whole, exp[:3])
    try:
        gpu_ctx.set_limits(max_pairs_per_batch=3)
        assert_same(gpu_ctx.match_pairs_verified(pairs), exp[:3])
        offs, qs, ds = [0], [], []
        for ch in gpu_ctx.match_pairs_stream(pairs, verified=True):
            offs += list(offs[-1] + ch["offsets"][1:])
            qs.append(ch["qt"])
            ds.append(ch["dist"])
        assert_same((np.asarray(offs, np.int64), np.concatenate(qs), np.concatenate(ds)), exp[:3])
    finally:
        gpu_ctx.set_limits(0, 0)
    n = np.diff(whole[0])
    assert n[0] == 0 and n[1] == 7 and n[7] == 7      # < 7: nothing; exactly 7: all kept


@pytest.mark.parametrize("n,outliers,thr", [(300, 0.3, 3.0), (1500, 0.5, 3.0), (800, 0.1, 1.0)])
def test_device_lists_against_the_fp64_reference(gpu_ctx, host, n, outliers, thr):
    """The device's verified list against oracle/fmat_ref.py on planted geometry: same winner, same mask except inside
    the reference's margin, and every planted inlier whose reference error is clearly below thr^2 is kept."""
    d1, k1, d2, k2 = copy_scene(n, 90 + n, outliers=outliers)
    upload(gpu_ctx, [(d1, k1), (d2, k2)])
    pairs = np.array([(0, 1)], np.int32)
    raw_off, raw_qt, _ = gpu_ctx.match_pairs(pairs)
    q, t = raw_qt[:, 0], raw_qt[:, 1]
    assert len(q) == n and np.all(np.diff(q) > 0)
    p1, p2 = k1[q, :2], k2[t, :2]
    ref = fmat_ref.ransac(p1, p2, thr)
    assert ref["decided"]
    got = gpu_ctx.match_pairs_verified(pairs, threshold=thr)
    keep = np.zeros(n, bool)
    keep[np.searchsorted(q, got[1][:, 0])] = True       # the lists keep the matcher's row order
    assert np.array_equal(q[keep], got[1][:, 0])
    diff = keep != ref["mask"]
    assert not np.any(diff & ~ref["unsure"]) and ref["unsure"].sum() <= 2
    planted = q < int(round(n * (1 - outliers)))
    e = fmat_ref.epipolar_error(fmat_ref.fit(*[np.asarray(c, np.float64) for c in (p1[planted, 0], p1[planted, 1], p2[planted, 0], p2[planted, 1])])[0],
                                p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1])
    clear = planted & ref["mask"] & (e < 0.5 * thr * thr)
    assert keep[clear].all()


@pytest.mark.parametrize("kind", ["identical", "collinear", "offset"])
def test_coordinate_extremes_equal_the_twin(gpu_ctx, host, kind):
    n = 500
    rng = np.random.default_rng(5)
    if kind == "identical":
        coords = (np.tile([1000.0, 700.0], (n, 1)), np.tile([1200.0, 650.0], (n, 1)))
    elif kind == "collinear":
        s = rng.uniform(0, 3000, n)
        coords = (np.c_[s, 0.25 * s + 40], np.c_[0.9 * s + 60 + rng.normal(0, 0.5, n), 0.3 * s + 10])
    else:
        d1, k1, d2, k2 = copy_scene(n, 7, outliers=0.3)
        coords = (k1[:, :2] + 1e5, k2[:, :2] - 1e5)
    d1, k1, d2, k2 = copy_scene(n, 8, coords=coords)
    upload(gpu_ctx, [(d1, k1), (d2, k2)])
    pairs = np.array([(0, 1), (1, 0)], np.int32)
    exp = expected_lists_ex(gpu_ctx, host, pairs, [k1, k2])
    assert_same(gpu_ctx.match_pairs_verified(pairs), exp[:3])
