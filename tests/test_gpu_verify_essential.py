"""The calibrated device verification (msfm_set_verification_model(.., MSFM_VERIFY_ESSENTIAL, camera): staged 5-point RANSAC,
csrc/msfm_verify_e.hip.h) against its host twin EssentialRansacMask (host/GeometricVerification.cpp through libmsfm_host.so):
the two share csrc/msfm_emat.h, so the verified lists must be IDENTICAL -- with and without lens distortion, on a planar scene,
over a threshold / confidence grid, at the LDS chunk edges, for n = 0 .. 6, one call and streamed across sub-batch cuts.  The
twin itself is checked against an independent reference in tests/test_emat_reference.py."""
import ctypes as C
import os

import numpy as np
import pytest

from monocularsfm_amd import _lib, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FOCAL = 3072, 2304, 2500.0
NO_DIST = (0.0, 0.0, 0.0, 0.0)
BARREL = (-0.12, 0.03, 4e-4, -3e-4)
ROUND = 32   # kVeRound


def camera(dist=NO_DIST):
    return (FOCAL, FOCAL, W / 2.0, H / 2.0) + tuple(dist)


@pytest.fixture(scope="module")
def host(built_lib):
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "monocularsfm_amd", "host"), "-s", "libmsfm_host.so"])
    L = C.CDLL(os.path.join(ROOT, "monocularsfm_amd", "host", "libmsfm_host.so"))
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.host_essential_ransac.argtypes = [fp, fp, C.c_int, dp, C.c_double, C.c_double, C.c_int, C.c_ulonglong, C.POINTER(C.c_ubyte)]
    return L


@pytest.fixture()
def ectx(built_lib):
    """A context of its own (the verification model is per context and must not leak into the session's)."""
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def host_mask(host, cam, p1, p2, threshold=3.0, confidence=0.99, max_iters=1000, seed=0x5eed5eed):
    p1 = np.ascontiguousarray(p1, F32)
    p2 = np.ascontiguousarray(p2, F32)
    mask = np.zeros(max(len(p1), 1), np.uint8)
    c = np.ascontiguousarray(cam, np.float64)
    n = host.host_essential_ransac(p1.ctypes.data_as(C.POINTER(C.c_float)), p2.ctypes.data_as(C.POINTER(C.c_float)), len(p1),
                                   c.ctypes.data_as(C.POINTER(C.c_double)), threshold, confidence, max_iters, seed,
                                   mask.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return mask[:n].astype(bool) if n else np.zeros(len(p1), bool)


def distort_px(k, dist):
    """Apply the Brown model (k1, k2, p1, p2) to pixel rows of a pinhole camera (FOCAL, W / 2, H / 2)."""
    k1, k2, p1, p2 = dist
    x = (k[:, 0].astype(np.float64) - W / 2.0) / FOCAL
    y = (k[:, 1].astype(np.float64) - H / 2.0) / FOCAL
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 * r2
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    out = k.copy()
    out[:, 0] = (FOCAL * xd + W / 2.0).astype(F32)
    out[:, 1] = (FOCAL * yd + H / 2.0).astype(F32)
    return out


def two_view(n_in, n_out, n_extra, seed, dist=NO_DIST, planar=False, noise=0.5):
    """Two images whose descriptors match one-to-one on their first n_in + n_out rows (shuffled); the n_in first observe 3-D
    points through synth.scene_cameras (a planar patch if `planar`), the n_out others are planted outliers at random places."""
    rng = np.random.default_rng(seed)
    n = n_in + n_out
    base = synth.rootsift_images(1, [n + 2 * n_extra + 1], seed=seed, n_proto=4 * (n + 2 * n_extra) + 64)[0]
    dA = np.r_[base[:n], base[n:n + n_extra]]
    nb = np.abs(base[:n] + rng.normal(0, 0.004, (n, 128)).astype(F32))
    nb /= np.maximum(np.linalg.norm(nb, axis=1, keepdims=True), 1e-12)
    dB = np.r_[nb.astype(F32), base[n + n_extra:n + 2 * n_extra]]
    cams = synth.scene_cameras(2, seed=seed, width=W, height=H, focal=FOCAL)
    ids = np.r_[np.arange(n_in), np.full(n_out + n_extra, -1)]
    if planar:
        X = np.c_[rng.uniform(-1.6, 1.6, n_in), rng.uniform(-1.1, 1.1, n_in), np.zeros(n_in)]
        X[:, 2] = 0.25 * X[:, 0] - 0.15 * X[:, 1]
        kps = []
        for i in range(2):
            R, t, f, cx, cy = cams[i]
            k = synth.keypoints(n + n_extra, seed=seed + 1000 + i, width=W, height=H)
            Xc = X @ R.T + t
            k[:n_in, 0] = (f * Xc[:, 0] / Xc[:, 2] + cx + rng.normal(0, noise, n_in)).astype(F32)
            k[:n_in, 1] = (f * Xc[:, 1] / Xc[:, 2] + cy + rng.normal(0, noise, n_in)).astype(F32)
            kps.append(k)
    else:
        kps = synth.scene_keypoints([ids, ids], cams, max(n_in, 1), seed=seed, noise_px=noise)
    kA, kB = distort_px(kps[0], dist), distort_px(kps[1], dist)
    pa, pb = rng.permutation(len(dA)), rng.permutation(len(dB))
    truth = np.zeros(len(dA), bool)
    truth[:n_in] = True
    return dA[pa].astype(F32), kA[pa], dB[pb].astype(F32), kB[pb], truth[pa]


def load(ctx, scenes):
    kps, truth = [], []
    for s, (dA, kA, dB, kB, tr) in enumerate(scenes):
        ctx.upload_image(2 * s, dA)
        ctx.upload_keypoints(2 * s, kA)
        ctx.upload_image(2 * s + 1, dB)
        ctx.upload_keypoints(2 * s + 1, kB)
        kps += [kA, kB]
        truth.append(tr)
    return kps, truth


def expected(ctx, host, cam, pairs, kps, **vkw):
    offs, qt, d = ctx.match_pairs(pairs)
    out_q, out_d, out_off = [], [], [0]
    for p, (i, j) in enumerate(pairs):
        s, e = offs[p], offs[p + 1]
        keep = host_mask(host, cam, kps[i][qt[s:e, 0], :2], kps[j][qt[s:e, 1], :2], **vkw) if e > s else np.zeros(0, bool)
        out_q.append(qt[s:e][keep])
        out_d.append(d[s:e][keep])
        out_off.append(out_off[-1] + int(keep.sum()))
    return np.asarray(out_off, np.int64), np.concatenate(out_q).reshape(-1, 2), np.concatenate(out_d)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))


@pytest.mark.parametrize("dist,planar", [(NO_DIST, False), (BARREL, False), (NO_DIST, True), (BARREL, True)])
def test_lists_equal_the_twin_and_recover_the_inliers(ectx, host, dist, planar):
    cam = camera(dist)
    scenes = [two_view(300, 100, 150, seed=31, dist=dist, planar=planar), two_view(600, 60, 50, seed=32, dist=dist, planar=planar),
              two_view(120, 140, 40, seed=33, dist=dist, planar=planar)]
    kps, truth = load(ectx, scenes)
    ectx.set_verification_model(_lib.VERIFY_ESSENTIAL, cam)
    pairs = np.array([(0, 1), (1, 0), (2, 3), (4, 5), (0, 3), (2, 5)], np.int32)
    want = expected(ectx, host, cam, pairs, kps)
    got = ectx.match_pairs_verified(pairs)
    assert same(got, want)
    assert ectx.profile()["verify_ms"] > 0
    # recovery on the true pairs (rows of the first image of the pair): >= 99 % of the matched planted inliers over the three, >= 95 %
    # in each (no refit: the pair with 46 % inliers stops on a 5-point model from noisy matches); the outliers kept are the twin's
    kept = matched = 0
    for p, s in ((0, 0), (2, 1), (3, 2)):
        q = got[1][got[0][p]:got[0][p + 1], 0]
        tr = truth[s]
        raw_off, raw_qt, _ = ectx.match_pairs(pairs[p:p + 1])
        matched_true = int(tr[raw_qt[:, 0]].sum())
        assert tr[q].sum() >= 0.95 * matched_true, (p, tr[q].sum(), matched_true)
        kept += int(tr[q].sum())
        matched += matched_true
    assert kept >= 0.99 * matched, (kept, matched)


@pytest.mark.parametrize("threshold,confidence,max_iters", [(1.0, 0.999, 1000), (3.0, 0.99, 1000), (6.0, 0.9, 300), (2.0, 0.99, 100)])
def test_parameter_grid(ectx, host, threshold, confidence, max_iters):
    cam = camera(BARREL)
    kps, _ = load(ectx, [two_view(200, 150, 60, seed=41, dist=BARREL), two_view(90, 20, 30, seed=42, dist=BARREL)])
    ectx.set_verification_model(1, cam)
    pairs = np.array([(0, 1), (2, 3), (1, 2)], np.int32)
    vkw = dict(threshold=threshold, confidence=confidence, max_iters=max_iters, seed=0x1234567)
    want = expected(ectx, host, cam, pairs, kps, **vkw)
    got = ectx.match_pairs_verified(pairs, **vkw)
    assert same(got, want)


def test_chunk_edges_and_tiny_pairs(ectx, host):
    """n around the 128-match LDS chunk and the 64-lane wave, and n = 0 .. 6 (< 5: nothing kept)."""
    cam = camera(NO_DIST)
    sizes = [(60, 4), (100, 28), (100, 29), (110, 147), (200, 57)] + [(k, 0) for k in range(0, 7)]
    scenes = [two_view(a, b, 20, seed=50 + i) for i, (a, b) in enumerate(sizes)]
    kps, _ = load(ectx, scenes)
    ectx.set_verification_model(1, cam)
    pairs = np.array([(2 * s, 2 * s + 1) for s in range(len(scenes))], np.int32)
    raw = ectx.match_pairs(pairs)[0]
    ns = np.diff(raw)
    assert {0, 5, 6} <= set(ns.tolist()) and {127, 128, 129} & set(ns.tolist()), ns
    want = expected(ectx, host, cam, pairs, kps)
    got = ectx.match_pairs_verified(pairs)
    assert same(got, want)
    assert all(np.diff(got[0])[ns < 5] == 0)


def test_sub_batch_cuts_and_streaming(ectx, host):
    cam = camera(BARREL)
    scenes = [two_view(150 + 40 * s, 30 + 10 * s, 20, seed=60 + s, dist=BARREL) for s in range(4)]
    kps, _ = load(ectx, scenes)
    ectx.set_verification_model(1, cam)
    pairs = np.array([(0, 1), (2, 3), (4, 5), (6, 7), (1, 2), (3, 0), (5, 6), (7, 4), (1, 0)], np.int32)
    want = expected(ectx, host, cam, pairs, kps)
    assert same(ectx.match_pairs_verified(pairs), want)
    one = [ectx.match_pairs_verified(pairs[k:k + 1]) for k in range(len(pairs))]
    assert np.array_equal(np.diff(want[0]), [o[0][1] for o in one])
    assert np.array_equal(np.concatenate([o[1] for o in one]), want[1])
    for limit in (1, 2, 4):
        ectx.set_limits(max_pairs_per_batch=limit)
        assert same(ectx.match_pairs_verified(pairs), want)
        qts, offs = [], [0]
        for ch in ectx.match_pairs_stream(pairs, verified=True):
            qts.append(ch["qt"])
            offs += (offs[-1] + ch["offsets"][1:]).tolist()
        assert np.array_equal(np.asarray(offs), want[0]) and np.array_equal(np.concatenate(qts), want[1])
    ectx.set_limits()


def test_staging_stops_early_on_clean_pairs(ectx, host):
    cam = camera(NO_DIST)
    clean = [two_view(400, 20, 20, seed=70 + s) for s in range(3)]   # >= 90 % inliers
    kps, _ = load(ectx, clean)
    ectx.set_verification_model(1, cam)
    pairs = np.array([(0, 1), (2, 3), (4, 5)], np.int32)
    got = ectx.match_pairs_verified(pairs)
    solved, rounds = ectx.verification_stats()
    assert 0 < solved <= ROUND * len(pairs) and rounds == 1, (solved, rounds)
    assert same(got, expected(ectx, host, cam, pairs, kps))
    # a low-inlier pair (w^5 tiny: the bound never drops below max_iters) runs to its bound
    ectx.clear_images()
    kps, _ = load(ectx, [two_view(40, 260, 20, seed=75)])
    got = ectx.match_pairs_verified(np.array([(0, 1)], np.int32))
    solved, rounds = ectx.verification_stats()
    assert solved == 1000 and rounds == (1000 + ROUND - 1) // ROUND, (solved, rounds)
    assert same(got, expected(ectx, host, cam, np.array([(0, 1)], np.int32), kps))


def test_model_0_after_model_1_is_the_f_path(ectx, built_lib):
    scenes = [two_view(300, 100, 50, seed=81), two_view(200, 80, 40, seed=82)]
    kps, _ = load(ectx, scenes)
    pairs = np.array([(0, 1), (2, 3), (1, 2)], np.int32)
    ectx.set_verification_model(1, camera())
    e_lists = ectx.match_pairs_verified(pairs)
    ectx.set_verification_model(0)
    f_lists = ectx.match_pairs_verified(pairs)
    assert ectx.verification_stats() == (0, 0)
    with _lib.Context(0) as fresh:
        load(fresh, scenes)
        assert same(f_lists, fresh.match_pairs_verified(pairs))
    assert e_lists[0][-1] > 0


def test_parameter_errors(ectx):
    def code(*a):
        with pytest.raises(_lib.MsfmError) as e:
            ectx.set_verification_model(*a)
        return e.value.code
    assert code(2, camera()) == _lib.E_INVALID
    assert code(-1) == _lib.E_INVALID
    assert code(1) == _lib.E_INVALID
    assert code(1, (0.0, 100.0, 1.0, 1.0)) == _lib.E_INVALID
    assert code(1, (100.0, -1.0, 1.0, 1.0)) == _lib.E_INVALID
    assert code(1, (float("nan"), 100.0, 1.0, 1.0)) == _lib.E_INVALID
    assert code(1, (100.0, 100.0, float("inf"), 1.0)) == _lib.E_INVALID
    assert code(1, (100.0, 100.0, 1.0, 1.0, float("nan"))) == _lib.E_INVALID
    kps, _ = load(ectx, [two_view(100, 10, 10, seed=90)])
    ectx.set_limits(max_pairs_per_batch=1)
    gen = ectx.match_pairs_stream(np.array([(0, 1), (1, 0)], np.int32), verified=True)
    next(gen)   # the series is open
    assert code(1, camera()) == _lib.E_STATE
    assert code(0) == _lib.E_STATE
    gen.close()
    ectx.set_limits()
    ectx.set_verification_model(1, camera())
    ectx.set_verification_model(0)
