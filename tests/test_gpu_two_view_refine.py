"""The two-view pose refinement on the device (msfm_set_two_view_refinement, csrc/msfm_verify_pose_refine.hip.h) against its host twin
(RefineTwoView, host/GeometricVerification.cpp; the arithmetic of both is csrc/msfm_pose_refine.h).  The twin is fed the device's OWN
unrefined records and kept lists (a run of the same context without the refinement), so what is compared is the refinement alone:

  * the two-view records and the refinement records equal the twin's BYTE FOR BYTE on every edge scene of
    tests/two_view_refine_fixtures.py (kept sizes on both sides of the strides of the 256 partial sums, one short of min_matches, a
    pair that starts at the minimum, a near-singular translation block), in one call, cut into sub-batches of one pair, and streamed;
    the same with max_iters = 1 and with a tight step_tol;
  * a grid that walks through valid, invalid and sub-min_matches pairs in one sub-batch, and under the model selection H-kept pairs
    (valid = 0): those come out untouched with status 0;
  * the 276 pairs of the seed-5 reconstruction capture, one of which ends with accepted steps and a record that does NOT stand;
  * switched off again the records equal those of a context that never had it, and the fetch is E_STATE;
  * the error codes of the two entry points; the match lists never change."""
import numpy as np
import pytest

import pose_twin
import reconstruction_fixtures as rfx
import two_view_fixtures
import two_view_refine_fixtures as fx
import two_view_refine_twin as rtw
from monocularsfm_amd import _lib
from test_gpu_two_view_geometry import load_cases, same_records
from test_gpu_verify_homography import load, same

pytestmark = pytest.mark.gpu
CAM = fx.CAM


@pytest.fixture(scope="module")
def host(built_lib):
    return rtw.load_host()


@pytest.fixture()
def tctx(built_lib):
    ctx = _lib.Context(0)
    ctx.set_verification_model(_lib.VERIFY_ESSENTIAL, CAM)
    ctx.set_two_view_geometry(True)
    yield ctx
    ctx.close()


def invariants(before, after, rf, min_matches=15):
    refined = _lib.two_view_refined(rf)
    eligible = (before["valid"] == 1) & (before["n_kept"] >= min_matches)
    assert np.array_equal((rf["status"] & _lib.TVR_ELIGIBLE) != 0, eligible)
    assert rf[~eligible].tobytes() == np.zeros(int((~eligible).sum()), rf.dtype).tobytes()
    assert after[~refined].tobytes() == before[~refined].tobytes()
    assert np.array_equal(after["n_kept"], before["n_kept"]) and np.array_equal(after["valid"], before["valid"])
    assert np.all(after["n_positive_depth"] >= before["n_positive_depth"]) and np.all(after["n_triangulated"] >= before["n_triangulated"])
    assert np.all(rf["cost_after"][refined] < rf["cost_before"][refined]) and np.all(rf["accepted"][refined] >= 1)
    assert np.array_equal(rf["cost_after"][~refined], rf["cost_before"][~refined])


@pytest.mark.parametrize("refine_params", [rtw.REFINE_DEFAULTS, (1, 15, 1e-6), (40, 15, 1e-10)], ids=["defaults", "one-step", "tight"])
def test_records_equal_the_twin_on_the_edge_scenes(tctx, host, refine_params):
    cases = fx.edge_cases()
    kps, pairs = load_cases(tctx, cases)
    n = len(pairs)
    lists = tctx.match_pairs_verified(pairs)
    before = tctx.two_view_geometry(n).copy()
    assert before["n_kept"][:len(fx.SIZES) + 1].tolist() == [14] + list(fx.SIZES) and before["valid"].all()
    want, want_rf = rtw.run(host, before, lists[:2], pairs, kps, CAM, refine_params=refine_params)
    max_iters, min_matches, step_tol = refine_params
    tctx.set_two_view_refinement(True, max_iters=max_iters, step_tol=step_tol, min_matches=min_matches)

    def check(on, got, rf):
        assert same(on, lists)                                # the match lists never change
        assert same_records(rf, want_rf) and same_records(got, want)
        invariants(before, got, rf)

    check(tctx.match_pairs_verified(pairs), tctx.two_view_geometry(n), tctx.two_view_refinements(n))
    rf = tctx.two_view_refinements(n)
    assert rf["status"][0] == 0 and (rf["status"][1:] & _lib.TVR_ELIGIBLE).all()     # 14 kept against min_matches 15
    assert int(_lib.two_view_refined(rf).sum()) >= len(fx.SIZES) - 1
    assert rf["steps"].max() <= max_iters
    tctx.set_limits(max_pairs_per_batch=1)
    check(tctx.match_pairs_verified(pairs), tctx.two_view_geometry(n), tctx.two_view_refinements(n))
    recs, rfs, qts, ds, offs = [], [], [], [], [0]
    for ch in tctx.match_pairs_stream(pairs, verified=True):
        assert ch["n_pairs"] == 1 and len(ch["two_view_refinements"]) == 1
        recs.append(ch["two_view_geometry"].copy())
        rfs.append(ch["two_view_refinements"].copy())
        qts.append(ch["qt"])
        ds.append(ch["dist"])
        offs += (offs[-1] + ch["offsets"][1:]).tolist()
    check((np.asarray(offs, np.int64), np.concatenate(qts), np.concatenate(ds)), np.concatenate(recs), np.concatenate(rfs))
    tctx.set_limits()


def test_grid_walks_through_valid_invalid_and_small_pairs(tctx, host):
    """two_view_fixtures.walk_job: 3 * CUs + 7 pairs in ONE sub-batch; its own-scene pairs keep 40 .. 120 matches, so min_matches =
    80 makes some of the valid ones ineligible; then the planar variant under the model selection."""
    cu = tctx.device_info()["cu_count"]
    for planar_every in (0, 3):
        job = two_view_fixtures.walk_job(cu, planar_every)
        pairs = job["pairs"]
        n = len(pairs)
        tctx.set_two_view_refinement(False)
        tctx.clear_images()
        kps, _ = load(tctx, job["scenes"])
        tctx.set_pipeline(1)
        tctx.set_limits(max_pairs_per_batch=n)
        tctx.set_model_selection(bool(planar_every), 0.7)
        lists = tctx.match_pairs_verified(pairs)
        before = tctx.two_view_geometry(n).copy()
        want, want_rf = rtw.run(host, before, lists[:2], pairs, kps, CAM, refine_params=(10, 80, 1e-6))
        tctx.set_two_view_refinement(True, min_matches=80)
        on = tctx.match_pairs_verified(pairs)
        assert tctx.profile()["sub_batches"] == 1
        got, rf = tctx.two_view_geometry(n), tctx.two_view_refinements(n)
        assert same(on, lists) and same_records(rf, want_rf) and same_records(got, want)
        invariants(before, got, rf, min_matches=80)
        valid, eligible, refined = before["valid"] == 1, (rf["status"] & _lib.TVR_ELIGIBLE) != 0, _lib.two_view_refined(rf)
        assert int(refined.sum()) >= 8 and int((valid & ~eligible).sum()) >= 8 and int((~valid).sum()) > 2 * cu
        if planar_every:
            h_kept = tctx.model_selection(n)[0] == _lib.VERIFY_HOMOGRAPHY
            assert int(h_kept.sum()) >= 8 and not before["valid"][h_kept].any() and not rf["status"][h_kept].any()
            assert got[h_kept].tobytes() == np.zeros(int(h_kept.sum()), got.dtype).tobytes()
    tctx.set_model_selection(False)
    tctx.set_two_view_refinement(False)
    tctx.set_limits()
    tctx.set_pipeline()


def test_a_capture_with_a_result_that_does_not_stand(tctx, host):
    """tests/reconstruction_fixtures.py's seed-5 capture (24 images, 276 pairs, 0.7 px): one pair's refined pose loses a triangulated
    match, so its steps are accepted and its record is NOT replaced (status ELIGIBLE | STEP_ACCEPTED); two loops end at max_iters."""
    cap = rfx.variant("s5")
    for k, i in enumerate(cap["ids"]):
        tctx.upload_image(int(i), cap["imgs"][k])
        tctx.upload_keypoints(int(i), cap["kps"][int(i)])
    tctx.set_two_view_geometry(True, *rfx.TWO_VIEW)
    pairs, n = cap["pairs"], len(cap["pairs"])
    lists = tctx.match_pairs_verified(pairs)
    before = tctx.two_view_geometry(n).copy()
    want, want_rf = rtw.run(host, before, lists[:2], pairs, cap["kps"], CAM, params=rfx.TWO_VIEW)
    tctx.set_two_view_refinement(True)
    on = tctx.match_pairs_verified(pairs)
    got, rf = tctx.two_view_geometry(n), tctx.two_view_refinements(n)
    assert same(on, lists) and same_records(rf, want_rf) and same_records(got, want)
    invariants(before, got, rf)
    lost = rf["status"] == (_lib.TVR_ELIGIBLE | _lib.TVR_STEP_ACCEPTED)
    assert int(lost.sum()) >= 1 and got[lost].tobytes() == before[lost].tobytes()
    assert int(_lib.two_view_refined(rf).sum()) >= 270 and (rf["stop"] == rtw.STOP_MAX_ITERS).any() and (rf["stop"] == rtw.STOP_STEP).any()


def test_off_path_and_error_codes(tctx, built_lib):
    cases = [fx.sized(65), fx.sized(257)]
    kps, pairs = load_cases(tctx, cases)
    L, h = tctx._L, tctx._h
    never = _lib.Context(0)
    try:
        never.set_verification_model(_lib.VERIFY_ESSENTIAL, CAM)
        never.set_two_view_geometry(True)
        load_cases(never, cases)
        ref_lists = never.match_pairs_verified(pairs)
        ref_rec = never.two_view_geometry(2).copy()
        assert never._L.msfm_fetch_two_view_refinements(never._h, None) == _lib.E_STATE
    finally:
        never.close()

    def code(enable, mi=10, mm=15, tol=1e-6):
        return L.msfm_set_two_view_refinement(h, int(enable), _lib.C.byref(_lib.TwoViewRefineParams(mi, mm, tol)))

    for bad in (dict(mi=0), dict(mm=4), dict(tol=-1e-9), dict(tol=float("nan")), dict(tol=float("inf"))):
        assert code(1, **bad) == _lib.E_INVALID
    assert L.msfm_set_two_view_refinement(h, 2, None) == _lib.E_INVALID
    assert L.msfm_fetch_two_view_refinements(h, None) == _lib.E_STATE
    assert L.msfm_set_two_view_refinement(h, 1, None) == _lib.OK       # NULL: the defaults
    assert L.msfm_set_two_view_geometry(h, 0, None) == _lib.E_INVALID   # the geometry cannot go while the refinement is on
    on_lists = tctx.match_pairs_verified(pairs)
    rf = tctx.two_view_refinements(2)
    assert _lib.two_view_refined(rf).all() and same(on_lists, ref_lists)
    assert tctx.two_view_geometry(2).tobytes() != ref_rec.tobytes()
    # a series: the setters are E_STATE inside it
    tctx.set_limits(max_pairs_per_batch=1)
    gen = tctx.match_pairs_stream(pairs, verified=True)
    first = next(gen)
    assert same_records(first["two_view_refinements"], rf[:1])
    assert code(0) == _lib.E_STATE and code(1) == _lib.E_STATE
    gen.close()
    tctx.set_limits()
    # off again: the records of a context that never had it, and no refinement records
    assert code(0) == _lib.OK
    off_lists = tctx.match_pairs_verified(pairs)
    assert same(off_lists, ref_lists) and same_records(tctx.two_view_geometry(2), ref_rec)
    assert L.msfm_fetch_two_view_refinements(h, None) == _lib.E_STATE
    gen = tctx.match_pairs_stream(pairs, verified=True)
    assert "two_view_refinements" not in next(gen)
    gen.close()
    # enabling without the two-view geometry
    assert L.msfm_set_two_view_geometry(h, 0, None) == _lib.OK
    assert code(1) == _lib.E_INVALID
    assert code(0) == _lib.OK
