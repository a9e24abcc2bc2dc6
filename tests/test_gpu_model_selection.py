"""The two-view model selection on the device (msfm_set_model_selection, csrc/msfm_verify_select.hip.h): under model 0 (F) or 1 (E)
every pair also runs the homography and keeps one of the two lists.  Checked here:

  * each pair's list is bit for bit the model 0 / 1 list or the model 2 list of the same context, and the record {model, nE, nH}
    agrees with the two lists' lengths and the rule (planar, rotation-only and general pairs, cross pairs of them; F and E);
  * the device equals the host twin TwoViewSelectMask (host/GeometricVerification.cpp) over a parameter grid, low-inlier pairs that
    run every H round, and pairs of n = 0 .. 8;
  * sub-batch cuts and the streaming form give the same lists and records;
  * switching it off restores the old path; the errors;
  * quality on planted outliers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from monocularsfm_amd import _lib, synth
from test_gpu_verify_homography import load, same, two_view

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = (2500.0, 2500.0, 1536.0, 1152.0)
FP, DP, UP, IP = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def host(built_lib):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "monocularsfm_amd", "host"), "-s", "libmsfm_host.so"])
    L = C.CDLL(os.path.join(ROOT, "monocularsfm_amd", "host", "libmsfm_host.so"))
    L.host_two_view_select.argtypes = [FP, FP, C.c_int, C.c_int, DP, C.c_double, C.c_double, C.c_double, C.c_int, C.c_ulonglong, UP, IP]
    return L


@pytest.fixture()
def sctx(built_lib):
    """A context of its own (the model and the selection are per context)."""
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


def rule(ne, nh, r=0.7):
    return ne > 0 and float(nh) >= r * float(ne)


def set_model(ctx, model):
    ctx.set_verification_model(model, CAM if model == 1 else None)


def lists(res):
    offs, qt, d = res
    return [(qt[offs[p]:offs[p + 1]], d[offs[p]:offs[p + 1]]) for p in range(len(offs) - 1)]


def same_list(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


def check_one_of(sel, rec, epi, hom, model, h_ratio=0.7):
    """Every pair of `sel` is `epi`'s or `hom`'s list, as the record and the rule say.  -> number of pairs that took H."""
    m, ne, nh = rec
    took_h = 0
    for p, (s, e, h) in enumerate(zip(lists(sel), lists(epi), lists(hom))):
        assert (ne[p], nh[p]) == (len(e[0]), len(h[0])), p
        take_h = rule(len(e[0]), len(h[0]), h_ratio)
        assert m[p] == (_lib.VERIFY_HOMOGRAPHY if take_h else model), p
        assert same_list(s, h if take_h else e), p
        took_h += take_h
    return took_h


def twin(host, ctx, pairs, kps, model, h_ratio=0.7, threshold=3.0, confidence=0.99, max_iters=1000, seed=0x5eed5eed):
    """The host twin over the unverified lists of the same context: (offsets, qt, dist) and the records."""
    offs, qt, d = ctx.match_pairs(pairs)
    out_q, out_d, out_off, recs = [], [], [0], []
    cam = np.asarray(CAM + (0.0,) * 4, np.float64)
    for p, (i, j) in enumerate(pairs):
        s, e = offs[p], offs[p + 1]
        p1 = np.ascontiguousarray(kps[i][qt[s:e, 0], :2], F32)
        p2 = np.ascontiguousarray(kps[j][qt[s:e, 1], :2], F32)
        mask = np.zeros(max(e - s, 1), np.uint8)
        rec = np.zeros(3, np.int32)
        k = host.host_two_view_select(p1.ctypes.data_as(FP), p2.ctypes.data_as(FP), int(e - s), model,
                                      cam.ctypes.data_as(DP) if model == 1 else None, h_ratio, threshold, confidence, max_iters, seed,
                                      mask.ctypes.data_as(UP), rec.ctypes.data_as(IP))
        keep = mask[:k].astype(bool) if k else np.zeros(e - s, bool)
        out_q.append(qt[s:e][keep])
        out_d.append(d[s:e][keep])
        out_off.append(out_off[-1] + int(keep.sum()))
        recs.append(rec)
    recs = np.asarray(recs, np.int32).reshape(-1, 3)
    return (np.asarray(out_off, np.int64), np.concatenate(out_q).reshape(-1, 2), np.concatenate(out_d)), tuple(recs.T)


def same_rec(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


MIX = [("planar", 300, 100, 60, 11), ("rotation", 250, 60, 40, 12), ("general", 300, 100, 60, 13), ("planar", 120, 140, 30, 14),
       ("general", 150, 40, 20, 15), ("rotation", 400, 20, 20, 16)]
MIX_PAIRS = np.array([(0, 1), (2, 3), (4, 5), (6, 7), (8, 9), (10, 11), (1, 0), (0, 5), (2, 9), (4, 7), (3, 10), (8, 1)], np.int32)


@pytest.mark.parametrize("model", [0, 1])
def test_lists_come_from_one_of_the_two_models(sctx, model):
    load(sctx, [two_view(*m[:4], seed=m[4]) for m in MIX])
    set_model(sctx, model)
    epi = sctx.match_pairs_verified(MIX_PAIRS)
    with pytest.raises(_lib.MsfmError) as e:
        sctx.model_selection(len(MIX_PAIRS))
    assert e.value.code == _lib.E_STATE
    set_model(sctx, 2)
    hom = sctx.match_pairs_verified(MIX_PAIRS)
    h_solved, h_rounds = sctx.verification_stats()
    set_model(sctx, model)
    sctx.set_model_selection(True)
    sel = sctx.match_pairs_verified(MIX_PAIRS)
    rec = sctx.model_selection(len(MIX_PAIRS))
    took_h = check_one_of(sel, rec, epi, hom, model)
    kinds = [m[0] for m in MIX]
    for p in (0, 1, 2, 4, 5):   # the pairs of one scene (>= 70 % inliers): planar / rotation-only take H, general ones keep the epipolar list
        assert (rec[0][p] == 2) == (kinds[p] != "general"), (p, rec)
    assert 0 < took_h < len(MIX_PAIRS)
    solved, rounds = sctx.verification_stats()
    if model == 0:
        assert (solved, rounds) == (h_solved, h_rounds)
    else:
        assert solved > h_solved and rounds >= h_rounds
    assert sctx.profile()["verify_ms"] > 0


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("threshold,confidence,max_iters,h_ratio", [(1.0, 0.999, 1000, 0.7), (6.0, 0.9, 300, 0.8), (2.0, 0.99, 100, 1.0)])
def test_device_equals_the_host_twin(sctx, host, model, threshold, confidence, max_iters, h_ratio):
    kps, _ = load(sctx, [two_view("planar", 200, 150, 60, seed=41), two_view("rotation", 90, 20, 30, seed=42),
                         two_view("general", 200, 60, 30, seed=43)])
    set_model(sctx, model)
    sctx.set_model_selection(True, h_ratio)
    pairs = np.array([(0, 1), (2, 3), (4, 5), (1, 2), (3, 4)], np.int32)
    vkw = dict(threshold=threshold, confidence=confidence, max_iters=max_iters, seed=0x1234567)
    got = sctx.match_pairs_verified(pairs, **vkw)
    rec = sctx.model_selection(len(pairs))
    want, want_rec = twin(host, sctx, pairs, kps, model, h_ratio, **vkw)
    assert same(got, want) and same_rec(rec, want_rec), (rec, want_rec)


@pytest.mark.parametrize("model", [0, 1])
def test_low_inlier_and_tiny_pairs(sctx, host, model):
    """Low-inlier pairs that run every H round (and, under E, every E round), and pairs of n = 0 .. 8: below both sample sizes and
    F's n == 7 case."""
    scenes = ([two_view("planar", 30, 270, 20, seed=60), two_view("rotation", 25, 240, 20, seed=61), two_view("general", 25, 250, 20, seed=62)]
              + [two_view("planar", k, 0, 20, seed=70 + k) for k in range(0, 9)] + [two_view("general", k, 0, 20, seed=80 + k) for k in (7, 8)])
    kps, _ = load(sctx, scenes)
    set_model(sctx, model)
    sctx.set_model_selection(True)
    pairs = np.array([(2 * s, 2 * s + 1) for s in range(len(scenes))], np.int32)
    ns = np.diff(sctx.match_pairs(pairs)[0])
    assert {0, 3, 4, 5, 7, 8} <= set(ns.tolist()), ns
    got = sctx.match_pairs_verified(pairs)
    rec = sctx.model_selection(len(pairs))
    want, want_rec = twin(host, sctx, pairs, kps, model)
    assert same(got, want) and same_rec(rec, want_rec)
    assert all(rec[0][rec[1] == 0] == model)   # nE = 0 keeps the (empty) epipolar list
    solved, rounds = sctx.verification_stats()
    assert rounds == (1000 + 63) // 64 if model == 0 else rounds >= (1000 + 63) // 64


@pytest.mark.parametrize("model", [0, 1])
def test_sub_batch_cuts_and_streaming(sctx, model):
    scenes = [two_view(("planar", "rotation", "general", "planar")[s], 150 + 40 * s, 30 + 10 * s, 20, seed=60 + s) for s in range(4)]
    load(sctx, scenes)
    set_model(sctx, model)
    sctx.set_model_selection(True)
    pairs = np.array([(0, 1), (2, 3), (4, 5), (6, 7), (1, 2), (3, 0), (5, 6), (7, 4), (1, 0)], np.int32)
    want = sctx.match_pairs_verified(pairs)
    want_rec = sctx.model_selection(len(pairs))
    assert 0 < int((want_rec[0] == 2).sum()) < len(pairs)
    for limit in (1, 2, 4):
        sctx.set_limits(max_pairs_per_batch=limit)
        assert same(sctx.match_pairs_verified(pairs), want)
        assert same_rec(sctx.model_selection(len(pairs)), want_rec)
        qts, offs, recs = [], [0], [[], [], []]
        for ch in sctx.match_pairs_stream(pairs, verified=True):
            assert ch["n_pairs"] <= limit
            qts.append(ch["qt"])
            offs += (offs[-1] + ch["offsets"][1:]).tolist()
            for k in range(3):
                recs[k].append(ch["model_selection"][k])
        assert np.array_equal(np.asarray(offs), want[0]) and np.array_equal(np.concatenate(qts), want[1])
        assert same_rec(tuple(np.concatenate(r) for r in recs), want_rec)
    sctx.set_limits()
    gen = sctx.match_pairs_stream(pairs[:1], verified=False)
    assert "model_selection" not in next(gen)
    gen.close()


def test_selection_off_restores_the_old_path_and_errors(sctx):
    scenes = [two_view("planar", 300, 100, 50, seed=81), two_view("general", 200, 80, 40, seed=82)]
    load(sctx, scenes)
    pairs = np.array([(0, 1), (2, 3), (1, 2)], np.int32)
    sctx.set_model_selection(True, 0.7)
    sel = sctx.match_pairs_verified(pairs)
    assert sctx.model_selection(len(pairs))[0][0] == 2
    sctx.set_model_selection(False)
    f_lists = sctx.match_pairs_verified(pairs)
    assert sctx.verification_stats() == (0, 0)
    with pytest.raises(_lib.MsfmError) as e:   # fetching after an unselected call
        sctx.model_selection(len(pairs))
    assert e.value.code == _lib.E_STATE
    with _lib.Context(0) as fresh:
        load(fresh, scenes)
        assert same(f_lists, fresh.match_pairs_verified(pairs))
        fresh.set_verification_model(2)
        h_lists = fresh.match_pairs_verified(pairs)
    assert not same(sel, f_lists)
    # under model 2 the selection has no effect
    sctx.set_model_selection(True)
    sctx.set_verification_model(2)
    assert same(sctx.match_pairs_verified(pairs), h_lists)
    with pytest.raises(_lib.MsfmError) as e:
        sctx.model_selection(len(pairs))
    assert e.value.code == _lib.E_STATE
    sctx.set_verification_model(0)
    # an unverified call has no records either
    sctx.match_pairs(pairs)
    with pytest.raises(_lib.MsfmError) as e:
        sctx.model_selection(len(pairs))
    assert e.value.code == _lib.E_STATE

    def code(*a):
        with pytest.raises(_lib.MsfmError) as e:
            sctx.set_model_selection(*a)
        return e.value.code
    for bad in (0.0, -0.7, float("nan"), float("inf"), -float("inf")):
        assert code(True, bad) == _lib.E_INVALID
    sctx.set_limits(max_pairs_per_batch=1)
    gen = sctx.match_pairs_stream(np.array([(0, 1), (1, 0)], np.int32), verified=True)
    next(gen)   # the series is open
    assert code(False) == _lib.E_STATE
    gen.close()
    sctx.set_limits()
    sctx.set_model_selection(False)


@pytest.mark.parametrize("kind", ["planar", "rotation", "general"])
def test_quality_on_planted_outliers(sctx, kind):
    """Fixed seeds, 0.3 px of noise: on planar and rotation-only pairs the selection takes H and keeps >= 95 % of the matched planted
    inliers and <= 1 % of the planted outliers; on general pairs it keeps the F list."""
    scenes = [two_view(kind, 300, 100, 40, seed=100 + s, noise=0.3) for s in range(4)]
    _, truth = load(sctx, scenes)
    pairs = np.array([(2 * s, 2 * s + 1) for s in range(len(scenes))], np.int32)
    f_lists = sctx.match_pairs_verified(pairs)
    sctx.set_model_selection(True)
    raw_off, raw_qt, _ = sctx.match_pairs(pairs)
    got = sctx.match_pairs_verified(pairs)
    rec = sctx.model_selection(len(pairs))
    if kind == "general":
        assert all(rec[0] == 0) and same(got, f_lists)
        return
    assert all(rec[0] == 2)
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
