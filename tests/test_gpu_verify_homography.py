"""The homography device verification (msfm_set_verification_model(.., MSFM_VERIFY_HOMOGRAPHY, NULL): staged 4-point RANSAC,
csrc/msfm_verify_h.hip.h) against its host twin HomographyRansacMask (host/GeometricVerification.cpp through libmsfm_host.so): the
two share csrc/msfm_hmat.h, so the verified lists must be IDENTICAL -- on planar, rotation-only and general-scene pairs, for
low-inlier pairs that run every round, for n = 0 .. 5 and all-collinear points, one call and streamed across sub-batch cuts.  The
twin itself is checked against an independent reference in tests/test_hmat_reference.py."""
import ctypes as C
import os

import numpy as np
import pytest

from monocularsfm_amd import _lib, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = 64   # kVhRound
GENS = {"planar": synth.planar_view_pair, "rotation": synth.rotation_view_pair, "general": synth.general_view_pair}


@pytest.fixture(scope="module")
def host(built_lib):
    import subprocess
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "monocularsfm_amd", "host"), "-s", "libmsfm_host.so"])
    L = C.CDLL(os.path.join(ROOT, "monocularsfm_amd", "host", "libmsfm_host.so"))
    fp = C.POINTER(C.c_float)
    L.host_homography_ransac.argtypes = [fp, fp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_ulonglong, C.POINTER(C.c_ubyte)]
    return L


@pytest.fixture()
def hctx(built_lib):
    """A context of its own (the verification model is per context and must not leak into the session's)."""
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def host_mask(host, p1, p2, threshold=3.0, confidence=0.99, max_iters=1000, seed=0x5eed5eed):
    p1 = np.ascontiguousarray(p1, F32)
    p2 = np.ascontiguousarray(p2, F32)
    mask = np.zeros(max(len(p1), 1), np.uint8)
    n = host.host_homography_ransac(p1.ctypes.data_as(C.POINTER(C.c_float)), p2.ctypes.data_as(C.POINTER(C.c_float)), len(p1),
                                    threshold, confidence, max_iters, seed, mask.ctypes.data_as(C.POINTER(C.c_ubyte)))
    return mask[:n].astype(bool) if n else np.zeros(len(p1), bool)


def two_view(kind, n_in, n_out, n_extra, seed, noise=0.5, keypoints=None):
    """Two images whose descriptors match one-to-one on their first n_in + n_out rows (shuffled): the rows of a synth view pair of
    `kind` (n_in inliers, n_out planted outliers), plus n_extra unmatched rows each."""
    rng = np.random.default_rng(seed)
    n = n_in + n_out
    base = synth.rootsift_images(1, [n + 2 * n_extra + 1], seed=seed, n_proto=4 * (n + 2 * n_extra) + 64)[0]
    dA = np.r_[base[:n], base[n:n + n_extra]]
    nb = np.abs(base[:n] + rng.normal(0, 0.004, (n, 128)).astype(F32))
    nb /= np.maximum(np.linalg.norm(nb, axis=1, keepdims=True), 1e-12)
    dB = np.r_[nb.astype(F32), base[n + n_extra:n + 2 * n_extra]]
    if keypoints is None:
        k1, k2, inlier, _ = GENS[kind](n_in, n_out, seed=seed, noise_px=noise)
    else:
        k1, k2 = keypoints
        inlier = np.r_[np.ones(n_in, bool), np.zeros(n_out, bool)]
    kA = np.r_[k1, synth.keypoints(n_extra, seed=seed + 7)]
    kB = np.r_[k2, synth.keypoints(n_extra, seed=seed + 8)]
    pa, pb = rng.permutation(len(dA)), rng.permutation(len(dB))
    truth = np.r_[inlier, np.zeros(n_extra, bool)]
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


def expected(ctx, host, pairs, kps, **vkw):
    offs, qt, d = ctx.match_pairs(pairs)
    out_q, out_d, out_off = [], [], [0]
    for p, (i, j) in enumerate(pairs):
        s, e = offs[p], offs[p + 1]
        keep = host_mask(host, kps[i][qt[s:e, 0], :2], kps[j][qt[s:e, 1], :2], **vkw) if e > s else np.zeros(0, bool)
        out_q.append(qt[s:e][keep])
        out_d.append(d[s:e][keep])
        out_off.append(out_off[-1] + int(keep.sum()))
    return np.asarray(out_off, np.int64), np.concatenate(out_q).reshape(-1, 2), np.concatenate(out_d)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))


@pytest.mark.parametrize("kind", ["planar", "rotation", "general"])
def test_lists_equal_the_twin(hctx, host, kind):
    scenes = [two_view(kind, 300, 100, 150, seed=31), two_view(kind, 600, 60, 50, seed=32), two_view(kind, 120, 140, 40, seed=33)]
    kps, _ = load(hctx, scenes)
    hctx.set_verification_model(_lib.VERIFY_HOMOGRAPHY)
    pairs = np.array([(0, 1), (1, 0), (2, 3), (4, 5), (0, 3), (2, 5)], np.int32)
    want = expected(hctx, host, pairs, kps)
    got = hctx.match_pairs_verified(pairs)
    assert same(got, want)
    assert hctx.profile()["verify_ms"] > 0 and got[0][-1] > 0


@pytest.mark.parametrize("threshold,confidence,max_iters", [(1.0, 0.999, 1000), (6.0, 0.9, 300), (2.0, 0.99, 100)])
def test_parameter_grid(hctx, host, threshold, confidence, max_iters):
    kps, _ = load(hctx, [two_view("planar", 200, 150, 60, seed=41), two_view("rotation", 90, 20, 30, seed=42)])
    hctx.set_verification_model(2)
    pairs = np.array([(0, 1), (2, 3), (1, 2)], np.int32)
    vkw = dict(threshold=threshold, confidence=confidence, max_iters=max_iters, seed=0x1234567)
    assert same(hctx.match_pairs_verified(pairs, **vkw), expected(hctx, host, pairs, kps, **vkw))


def test_low_inlier_tiny_and_collinear_pairs(hctx, host):
    """Low-inlier pairs that need every hypothesis, n around the 256-match LDS chunk, n = 0 .. 5, and a pair whose points are all
    collinear in image 1 (every sample rejected: nothing kept)."""
    rng = np.random.default_rng(5)
    s = np.sort(rng.uniform(0, 1, 60))
    line = synth.keypoints(60, seed=91)
    line[:, 0] = (200 + 2500 * s).astype(F32)
    line[:, 1] = (300 + 0.5 * (line[:, 0] - 200)).astype(F32)
    collinear = two_view("planar", 0, 60, 10, seed=90, keypoints=(line, synth.keypoints(60, seed=92)))
    scenes = ([two_view("planar", 30, 270, 20, seed=60), two_view("rotation", 25, 240, 20, seed=61),
               two_view("planar", 200, 55, 10, seed=62), two_view("planar", 200, 57, 10, seed=63)]
              + [two_view("planar", k, 0, 20, seed=70 + k) for k in range(0, 6)] + [collinear])
    kps, _ = load(hctx, scenes)
    hctx.set_verification_model(2)
    pairs = np.array([(2 * s, 2 * s + 1) for s in range(len(scenes))], np.int32)
    ns = np.diff(hctx.match_pairs(pairs)[0])
    assert {0, 3, 4, 5} <= set(ns.tolist()) and ns[-1] >= 40, ns
    want = expected(hctx, host, pairs, kps)
    got = hctx.match_pairs_verified(pairs)
    assert same(got, want)
    kept = np.diff(got[0])
    assert all(kept[ns < 4] == 0) and kept[-1] == 0
    solved, rounds = hctx.verification_stats()
    assert rounds == (1000 + ROUND - 1) // ROUND, (solved, rounds)


def test_staging_stats(hctx, host):
    kps, _ = load(hctx, [two_view("planar", 400, 20, 20, seed=70 + s) for s in range(3)])   # >= 95 % inliers
    hctx.set_verification_model(2)
    pairs = np.array([(0, 1), (2, 3), (4, 5)], np.int32)
    got = hctx.match_pairs_verified(pairs)
    solved, rounds = hctx.verification_stats()
    assert 0 < solved <= ROUND * len(pairs) and rounds == 1, (solved, rounds)
    assert same(got, expected(hctx, host, pairs, kps))
    # a low-inlier pair (w^4 tiny: the bound never drops below max_iters) runs every round
    hctx.clear_images()
    kps, _ = load(hctx, [two_view("rotation", 20, 280, 20, seed=75)])
    got = hctx.match_pairs_verified(np.array([(0, 1)], np.int32))
    solved, rounds = hctx.verification_stats()
    assert solved == 1000 and rounds == (1000 + ROUND - 1) // ROUND, (solved, rounds)
    assert same(got, expected(hctx, host, np.array([(0, 1)], np.int32), kps))


def test_sub_batch_cuts_and_streaming(hctx, host):
    scenes = [two_view(("planar", "rotation", "general", "planar")[s], 150 + 40 * s, 30 + 10 * s, 20, seed=60 + s) for s in range(4)]
    kps, _ = load(hctx, scenes)
    hctx.set_verification_model(2)
    pairs = np.array([(0, 1), (2, 3), (4, 5), (6, 7), (1, 2), (3, 0), (5, 6), (7, 4), (1, 0)], np.int32)
    want = expected(hctx, host, pairs, kps)
    assert same(hctx.match_pairs_verified(pairs), want)
    for limit in (1, 2, 4):
        hctx.set_limits(max_pairs_per_batch=limit)
        assert same(hctx.match_pairs_verified(pairs), want)
        qts, offs = [], [0]
        for ch in hctx.match_pairs_stream(pairs, verified=True):
            qts.append(ch["qt"])
            offs += (offs[-1] + ch["offsets"][1:]).tolist()
        assert np.array_equal(np.asarray(offs), want[0]) and np.array_equal(np.concatenate(qts), want[1])
    hctx.set_limits()


def test_model_0_after_model_2_is_the_f_path(hctx, built_lib):
    scenes = [two_view("planar", 300, 100, 50, seed=81), two_view("general", 200, 80, 40, seed=82)]
    load(hctx, scenes)
    pairs = np.array([(0, 1), (2, 3), (1, 2)], np.int32)
    hctx.set_verification_model(2)
    h_lists = hctx.match_pairs_verified(pairs)
    hctx.set_verification_model(0)
    f_lists = hctx.match_pairs_verified(pairs)
    assert hctx.verification_stats() == (0, 0)
    with _lib.Context(0) as fresh:
        load(fresh, scenes)
        assert same(f_lists, fresh.match_pairs_verified(pairs))
    assert h_lists[0][-1] > 0


def test_parameter_errors(hctx):
    def code(*a):
        with pytest.raises(_lib.MsfmError) as e:
            hctx.set_verification_model(*a)
        return e.value.code
    assert code(2, (2500.0, 2500.0, 1536.0, 1152.0)) == _lib.E_INVALID
    assert code(3) == _lib.E_INVALID
    assert code(-1) == _lib.E_INVALID
    load(hctx, [two_view("planar", 100, 10, 10, seed=90)])
    hctx.set_limits(max_pairs_per_batch=1)
    gen = hctx.match_pairs_stream(np.array([(0, 1), (1, 0)], np.int32), verified=True)
    next(gen)   # the series is open
    assert code(2) == _lib.E_STATE
    gen.close()
    hctx.set_limits()
    hctx.set_verification_model(2)
    hctx.set_verification_model(0)


@pytest.mark.parametrize("kind", ["planar", "rotation"])
def test_quality_on_planted_outliers(hctx, kind):
    """Fixed seeds, 0.3 px of noise: over the pairs >= 95 % of the matched planted inliers kept and <= 1 % of the planted outliers
    (no refit: a pair's winner is a 4-point fit, so a single pair may keep fewer -- DESIGN.md 11)."""
    scenes = [two_view(kind, 300, 100, 40, seed=100 + s, noise=0.3) for s in range(4)]
    _, truth = load(hctx, scenes)
    hctx.set_verification_model(2)
    pairs = np.array([(2 * s, 2 * s + 1) for s in range(len(scenes))], np.int32)
    raw_off, raw_qt, _ = hctx.match_pairs(pairs)
    got = hctx.match_pairs_verified(pairs)
    kin = min_in = mout = kout = 0
    for p in range(len(pairs)):
        tr = truth[p]
        q = got[1][got[0][p]:got[0][p + 1], 0]
        raw = raw_qt[raw_off[p]:raw_off[p + 1], 0]
        kin += int(tr[q].sum())
        min_in += int(tr[raw].sum())
        kout += int((~tr[q]).sum())
        mout += int((~tr[raw]).sum())
    assert min_in > 1000 and mout > 300, (min_in, mout)
    assert kin >= 0.95 * min_in and kout <= 0.01 * mout, (kin, min_in, kout, mout)
