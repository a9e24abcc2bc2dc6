"""The two-view pose refinement's host twin (monocularsfm_amd/csrc/msfm_pose_refine.h, RefineTwoView, through libmsfm_host.so and
tests/two_view_refine_twin.py) against the independent numpy reference tests/two_view_refine_ref.py (long double), on the edge scenes
of tests/two_view_refine_fixtures.py, and against the GROUND TRUTH of tests/reconstruction_fixtures.py.  CPU only.  Every test prints
its figures before it asserts; DESIGN.md section 27 has the tables.

Arithmetic.  The twin's Jacobian against central differences of the twin's own residual through the twin's own update (h = 1e-6 in
the five unknowns: the truncation error is h^2 |r'''| / 6 ~ 1e-12 * 1e4 relative to entries of ~3e3 px per unit, the rounding error
eps |r| / h ~ 1e-9; bound 1e-6 relative to the largest entry) and against the reference's analytic one (1e-11 relative).

Twin against reference.  Runs at step_tol = 1e-10 with room to get there (max_iters = 50), the convention of
tests/test_refine_poses_reference.py; every sized scene and the short baseline end by STOP_STEP in the reference.  At that tolerance the
last accepted steps change the cost by parts in 1e16, so the NUMBER of evaluated steps is decided by rounding (the reference itself
takes 5 .. 25 in long double and 7 .. 35 in double on the same inputs) and is not compared; the status, the record's counts and its
verdict are.  The bound on R, t, the costs and the statistics is 16 x the reference's own scatter: the largest difference between the
reference run in long double and the same reference run in double over the compared scenes, measured in this module on the same
inputs (scatter() below; measured: R 1.44e-10, t 4.04e-11, cost 2.30e-14 relative, mean_residual 1.64e-10 px, angles 1.07e-8 degrees --
the largest of them from the scene of 256 matches, where the reference accepts one more step in long double than in double: the
conditioning of a minimum that rounding moves, not the twin; the twin's worst differences from the reference are R 1.24e-10, t 2.97e-11,
cost 2.92e-14, mean_residual 1.06e-10 px, angles 8.91e-9 degrees, on that scene too).

Benefit.  The records of reconstruction_fixtures' seeds 77 and 5 at 0.7 px, refined by the twin, against the true relative pose of the
pair as given.  MEASURED here (median / maximum rotation error, median / maximum translation direction error, degrees):
    s77   0.7941 / 5.016 / 0.8241 / 10.52  ->  0.1724 / 0.7344 / 0.1822 / 2.934     rotation error grows for 8.7 % of the records
    s5    0.7149 / 4.594 / 0.8303 / 28.98  ->  0.1650 / 1.055  / 0.1812 / 4.249     rotation error grows for 9.4 %
The refined medians are bound by 2 x those (REFINED_RECORDS); the share of records that end worse is printed, not bound."""
import functools

import numpy as np
import pytest

import pose_twin
import reconstruction_fixtures as rfx
import two_view_refine_fixtures as fx
import two_view_refine_ref as ref
import two_view_refine_twin as rtw
from test_reconstruction_reference import CLEAN, NOISY, chain, record_errors
from twin_context import TwinContext

CAM = fx.CAM
F = (CAM[0] + CAM[1]) * 0.5
TIGHT = (50, 15, 1e-10)
RECORD_BYTES = pose_twin.RECORD.itemsize
# per variant, refined: median and maximum rotation error, median and maximum translation direction error of the 276 records, degrees
REFINED_RECORDS = {
    "s77": (0.1724, 0.7344, 0.1822, 2.934),
    "s5": (0.1650, 1.055, 0.1812, 4.249),
    "s77-clean": (7.731e-06, 0.0001416, 7.270e-06, 0.0002503),
    "s5-clean": (9.583e-06, 0.0002129, 1.016e-05, 0.0003014),
}
# per variant, the whole chain started from the refined records (reconstruction_fixtures.figures), MEASURED here
REFINED_CHAIN = {
    "s77": dict(centre_max=0.005335, rotation_max=0.1203, point_median=0.01979, point_p95=0.03421, share_succeeded=0.9993, share_mixed=0),
    "s5": dict(centre_max=0.004213, rotation_max=0.1115, point_median=0.01791, point_p95=0.03798, share_succeeded=1, share_mixed=0),
    "s77-distorted": dict(centre_max=0.01722, rotation_max=0.4084, point_median=0.07972, point_p95=0.1055, share_succeeded=0.9986, share_mixed=0),
    "s5-distorted": dict(centre_max=0.005088, rotation_max=0.05142, point_median=0.004957, point_p95=0.03182, share_succeeded=1, share_mixed=0),
    "s77-permuted": dict(centre_max=0.004332, rotation_max=0.05689, point_median=0.003227, point_p95=0.02644, share_succeeded=0.9993, share_mixed=0),
    "s77-swapped": dict(centre_max=0.00407, rotation_max=0.04253, point_median=0.003187, point_p95=0.02194, share_succeeded=0.9993, share_mixed=0),
    "s77-clean": dict(centre_max=1.981e-07, rotation_max=3.415e-06, point_median=3.773e-07, point_p95=7.291e-07, share_succeeded=0.9993, share_mixed=0),
    "s5-clean": dict(centre_max=5.233e-07, rotation_max=9.353e-06, point_median=1.612e-06, point_p95=2.263e-06, share_succeeded=1, share_mixed=0),
}


@pytest.fixture(scope="module")
def host():
    return rtw.load_host()


@functools.lru_cache(maxsize=None)
def scene(name):
    """an edge scene through the twin's two-view geometry -> dict(case, mask, rec, q1, q2): the unrefined record and its kept list"""
    host = rtw.load_host()
    c = {c["name"]: c for c in fx.edge_cases()}[name]
    p1, p2 = fx.planted(c)
    mask, rec = pose_twin.geometry(host, p1, p2, CAM)
    return dict(case=c, mask=mask, rec=rec, q1=pose_twin.normalise(host, CAM, p1[mask]), q2=pose_twin.normalise(host, CAM, p2[mask]))


SIZED = ["sized-%d" % n for n in fx.SIZES]
COMPARED = SIZED + ["short-baseline"]


@functools.lru_cache(maxsize=None)
def runs(name, refine_params=TIGHT):
    """-> (twin's (record, refinement), the reference in long double, the reference in double)"""
    s = scene(name)
    twin = rtw.refine(rtw.load_host(), s["rec"], s["q1"], s["q2"], F, refine_params=refine_params)
    return twin, ref.refine(s["rec"], s["q1"], s["q2"], F, refine_params=refine_params), \
        ref.refine(s["rec"], s["q1"], s["q2"], F, refine_params=refine_params, dtype=np.float64)


def differences(a, ra, b, rb):
    """two results (record mapping, refinement mapping) -> worst differences: R, t absolute; costs relative; statistics absolute"""
    cb, ca = float(rb["cost_before"]), float(rb["cost_after"])
    return dict(R=float(np.abs(np.asarray(a["R"], np.longdouble).reshape(9) - np.asarray(b["R"], np.longdouble).reshape(9)).max()),
                t=float(np.abs(np.asarray(a["t"], np.longdouble) - np.asarray(b["t"], np.longdouble)).max()),
                cost=max(abs(float(ra["cost_before"]) - cb) / cb, abs(float(ra["cost_after"]) - ca) / ca),
                residual=abs(float(a["mean_residual"]) - float(b["mean_residual"])),
                angle=max(abs(float(a[k]) - float(b[k])) for k in ("median_tri_angle", "mean_tri_angle")))


@functools.lru_cache(maxsize=None)
def scatter():
    """the reference's own rounding scatter: long double against double on the compared scenes, the worst per quantity"""
    worst = dict(R=0.0, t=0.0, cost=0.0, residual=0.0, angle=0.0)
    for name in COMPARED:
        _, (oL, rL), (o6, r6) = runs(name)
        assert oL is not None and o6 is not None
        d = differences(o6, r6, oL, rL)
        worst = {k: max(worst[k], d[k]) for k in worst}
    return worst


# ---- arithmetic -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sized-15", "sized-257", "short-baseline"])
def test_jacobian_agrees_with_central_differences(host, name):
    s = scene(name)
    R, t = s["rec"]["R"], s["rec"]["t"]
    r, J = rtw.residuals(host, R, t, F, s["q1"], s["q2"], jacobian=True)
    assert np.array_equal(r, rtw.residuals(host, R, t, F, s["q1"], s["q2"]))
    h = 1e-6
    num = np.zeros_like(J)
    for k in range(5):
        d = np.zeros(5)
        d[k] = h
        num[:, k] = (rtw.residuals(host, *rtw.update(host, R, t, d), F, s["q1"], s["q2"]) -
                     rtw.residuals(host, *rtw.update(host, R, t, -d), F, s["q1"], s["q2"])) / (2 * h)
    scale = np.abs(J).max()
    Jr = ref.jacobian(R, t, F, s["q1"], s["q2"])
    worst = (float(np.abs(J - num).max() / scale), float(np.abs(J - Jr).max() / scale),
             float(np.abs(Jr - ref.jacobian_numeric(R, t, F, s["q1"], s["q2"], h=1e-9)).max() / scale))
    print("jacobian[%s] scale %.4g, relative: twin - differences %.3g, twin - reference %.3g, reference - its differences %.3g" % ((name, scale) + worst))
    assert scale > 100 and worst[0] < 1e-6 and worst[1] < 1e-11 and worst[2] < 1e-9
    assert np.abs(r - np.asarray(ref.residuals(R, t, F, s["q1"], s["q2"]), np.float64)).max() < 1e-11 * max(1.0, np.abs(r).max())


def test_update_keeps_a_proper_rotation_and_a_unit_direction(host):
    s = scene("sized-63")
    rng = np.random.default_rng(3)
    for _ in range(20):
        d = rng.normal(0, 0.05, 5)
        R, t = rtw.update(host, s["rec"]["R"], s["rec"]["t"], d)
        Rr, tr = ref.update(s["rec"]["R"], s["rec"]["t"], d)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and np.linalg.det(R) > 0 and abs(np.linalg.norm(t) - 1) < 4 * np.finfo(float).eps
        assert np.abs(R - np.asarray(Rr, np.float64)).max() < 1e-15 and np.abs(t - np.asarray(tr, np.float64)).max() < 1e-15


def test_scatter_is_measured():
    w = scatter()
    print("scatter (reference, long double against double) %s; bounds x16 %s" % (w, {k: 16 * v for k, v in w.items()}))
    # 2 x the figures measured (the module's docstring): the 16 x bounds below cannot grow unnoticed
    assert 0 < w["R"] <= 2 * 1.44e-10 and 0 < w["t"] <= 2 * 4.05e-11 and w["cost"] <= 2 * 2.30e-14
    assert w["residual"] <= 2 * 1.65e-10 and w["angle"] <= 2 * 1.07e-8


@pytest.mark.parametrize("name", COMPARED)
def test_twin_equals_reference(host, name):
    (out, rf), (oL, rL), _ = runs(name)
    tol = {k: 16 * v for k, v in scatter().items()}
    assert rL["stop"] == ref.STOP_STEP and rL["trace"]["accepted"] >= 3, "the comparison is over runs that end on the step criterion"
    assert oL is not None and rf["status"] == rL["status"] == 7 and rf["stop"] == ref.STOP_STEP
    d = differences(out, rf, oL, rL)
    print("twin - reference[%s] %s (bounds %s); steps twin %d reference %d, accepted %d / %d" %
          (name, d, tol, rf["steps"], rL["steps"], rf["accepted"], rL["accepted"]))
    assert all(d[k] <= tol[k] for k in tol), (d, tol)
    for k in ("valid", "n_kept", "n_positive_depth", "n_triangulated", "is_initial_candidate"):
        assert int(out[k]) == int(oL[k]), k
    assert rf["n_positive_depth_before"] == rL["n_positive_depth_before"] and rf["n_triangulated_before"] == rL["n_triangulated_before"]
    assert rL["stats"]["error_margin"] > 16 * tol["residual"]            # (no count of the reference sits on its threshold)


@pytest.mark.parametrize("name", [c for c in ["sized-14"] + COMPARED + ["noise-free"]])
@pytest.mark.parametrize("refine_params", [rtw.REFINE_DEFAULTS, (1, 15, 1e-6), TIGHT], ids=["defaults", "one-step", "tight"])
def test_refined_records_are_proper_and_others_untouched(host, name, refine_params):
    s = scene(name)
    out, rf = rtw.refine(host, s["rec"], s["q1"], s["q2"], F, refine_params=refine_params)
    assert out["n_kept"] == s["rec"]["n_kept"] == s["mask"].sum() and rf["steps"] <= refine_params[0]
    if name != "short-baseline":
        assert s["mask"].all() and s["rec"]["n_kept"] == s["case"]["nk"]          # what the device tests rely on
    if rf["status"] & rtw.REFINED:
        R, t = out["R"].reshape(3, 3), out["t"]
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0
        assert abs(np.linalg.norm(t) - 1) <= 4 * np.finfo(float).eps
        assert out["n_positive_depth"] >= s["rec"]["n_positive_depth"] and out["n_triangulated"] >= s["rec"]["n_triangulated"]
        assert rf["accepted"] >= 1 and rf["cost_after"] < rf["cost_before"] and rf["status"] == 7
    else:
        assert out.tobytes() == s["rec"].tobytes() and rf["cost_after"] == rf["cost_before"]
    if name == "sized-14":
        assert rf.tobytes() == np.zeros(1, rtw.REFINEMENT).tobytes()           # 14 kept against min_matches 15: not eligible
        out5, rf5 = rtw.refine(host, s["rec"], s["q1"], s["q2"], F, refine_params=(10, 14, 1e-6))
        assert rf5["status"] & rtw.ELIGIBLE
    else:
        assert rf["status"] & rtw.ELIGIBLE and rf["n_triangulated_before"] == s["rec"]["n_triangulated"]
    if refine_params[0] == 1 and name != "sized-14":
        assert rf["steps"] == 1 and rf["stop"] in (ref.STOP_MAX_ITERS, ref.STOP_STEP)


def test_an_invalid_record_is_not_eligible(host):
    s = scene("sized-63")
    rec = np.zeros(1, pose_twin.RECORD)[0]
    out, rf = rtw.refine(host, rec, s["q1"], s["q2"], F)
    assert out.tobytes() == rec.tobytes() and rf.tobytes() == np.zeros(1, rtw.REFINEMENT).tobytes()


def as_record(fields):
    rec = np.zeros(1, pose_twin.RECORD)[0]
    for k, v in fields.items():
        rec[k] = v
    return rec


def moved_by(out, rec):
    return float(np.abs(out["R"] - rec["R"]).max()), float(np.abs(out["t"] - rec["t"]).max())


@pytest.mark.parametrize("refine_params", [rtw.REFINE_DEFAULTS, TIGHT], ids=["defaults", "tight"])
def test_a_pair_that_starts_at_the_minimum_stays_there(host, refine_params):
    """The issue's noise-free pair: a start AT the minimum, whatever the outcome the twin's verdict is the reference's and the pose moves
    by less than the scatter bound (16 x scatter(): R 2.3e-9, t 6.5e-10).  two_view_refine_fixtures.exact_pair: exact fp64 projections,
    the record at the true pose, so nothing but rounding separates the start from the minimum (cost ~6e-25 px^2)."""
    fields, q1, q2 = fx.exact_pair()
    rec = as_record(fields)
    out, rf = rtw.refine(host, rec, q1, q2, F, refine_params=refine_params)
    oL, rL = ref.refine(rec, q1, q2, F, refine_params=refine_params)
    tol = {k: 16 * v for k, v in scatter().items()}
    mR, mt = moved_by(out, rec)
    print("exact pair %s: twin status %d stop %d steps %d accepted %d cost %.3g -> %.3g, moved R %.3g t %.3g (bounds %.3g, %.3g); reference "
          "status %d stop %d" % (refine_params, rf["status"], rf["stop"], rf["steps"], rf["accepted"], rf["cost_before"], rf["cost_after"], mR, mt,
                                 tol["R"], tol["t"], rL["status"], rL["stop"]))
    assert rf["status"] & rtw.ELIGIBLE and rf["cost_before"] < 1e-20
    assert mR <= tol["R"] and mt <= tol["t"]
    assert (rf["status"] & rtw.REFINED) == (rL["status"] & rtw.REFINED)
    if oL is not None:
        assert np.abs(out["R"] - np.asarray(oL["R"], np.float64).reshape(9)).max() <= tol["R"]
        assert np.abs(out["t"] - np.asarray(oL["t"], np.float64)).max() <= tol["t"]
        for k in ("n_positive_depth", "n_triangulated", "is_initial_candidate"):
            assert int(out[k]) == int(oL[k])
    else:
        assert out.tobytes() == rec.tobytes()


# the noise-free float32 scene: what the REFERENCE moves its pose by, long double, defaults and step_tol 1e-10 (R, t)
NOISE_FREE_MOVES = (2.56e-06, 2.36e-06)


def test_float32_keypoints_without_noise_are_not_at_the_minimum(host):
    """The device's noise-free scene (its keypoints are float32: the device takes no others) does NOT start at the minimum: rounding the
    keypoints to float32 (~1e-4 px) puts the five-point record 2.6e-6 from the minimum of the 120 rounded matches, and the refinement
    goes there in 4 steps (cost 2.1e-5 -> 9.3e-8 px^2).  So this scene cannot meet the issue's bound on the movement (the scatter bound,
    2.3e-9): the pair above does.  Here the twin's pose is within the scatter bound of the REFERENCE's, the verdict is the reference's,
    and the movement is within 2 x what the reference itself moves (NOISE_FREE_MOVES)."""
    (out, rf), (oL, rL), _ = runs("noise-free")
    s = scene("noise-free")
    tol = {k: 16 * v for k, v in scatter().items()}
    mR, mt = moved_by(out, s["rec"])
    ref_moved = (float(np.abs(np.asarray(oL["R"], np.float64).reshape(9) - s["rec"]["R"]).max()),
                 float(np.abs(np.asarray(oL["t"], np.float64) - s["rec"]["t"]).max()))
    print("noise-free (float32 keypoints): twin status %d stop %d steps %d cost %.4g -> %.4g, moved R %.4g t %.4g; reference status %d stop %d "
          "steps %d, moved R %.4g t %.4g" % (rf["status"], rf["stop"], rf["steps"], rf["cost_before"], rf["cost_after"], mR, mt, rL["status"],
                                             rL["stop"], rL["steps"], ref_moved[0], ref_moved[1]))
    assert rf["status"] == rL["status"] == 7 and rf["cost_before"] < 1e-3
    assert ref_moved[0] <= 2 * NOISE_FREE_MOVES[0] and ref_moved[1] <= 2 * NOISE_FREE_MOVES[1]
    assert mR <= 2 * NOISE_FREE_MOVES[0] and mt <= 2 * NOISE_FREE_MOVES[1]
    assert np.abs(out["R"] - np.asarray(oL["R"], np.float64).reshape(9)).max() <= tol["R"]
    assert np.abs(out["t"] - np.asarray(oL["t"], np.float64)).max() <= tol["t"]
    for k in ("n_positive_depth", "n_triangulated", "is_initial_candidate"):
        assert int(out[k]) == int(oL[k])


def test_a_short_baseline_changes_the_record_only_under_the_standing_rule(host):
    """baseline = 1e-4 of the depth (the issue's scene).  It gives NONE of the outcomes the issue names for it: with 0.7 px of noise the
    translation block is weak, not singular -- under the defaults 10 evaluated steps, 4 accepted, MAX_ITERS, and the refined record
    stands (counts 79 / 76 -> 107 / 107).  What holds is the rule: the record changes only because the standing rule holds, and the
    twin's route is the reference's.  The ceiling, the pivot rejection and a result that does not stand are reached by the three tests
    below."""
    s = scene("short-baseline")
    out, rf = rtw.refine(host, s["rec"], s["q1"], s["q2"], F)
    oL, rL = ref.refine(s["rec"], s["q1"], s["q2"], F)
    print("short-baseline: kept %d; twin status %d stop %d steps %d accepted %d, counts %d/%d -> %d/%d; reference status %d stop %d steps %d" %
          (s["rec"]["n_kept"], rf["status"], rf["stop"], rf["steps"], rf["accepted"], s["rec"]["n_positive_depth"], s["rec"]["n_triangulated"],
           out["n_positive_depth"], out["n_triangulated"], rL["status"], rL["stop"], rL["steps"]))
    assert rf["status"] == rL["status"] and rf["stop"] == rL["stop"] and rf["steps"] == rL["steps"] and rf["accepted"] == rL["accepted"]
    if rf["status"] & rtw.REFINED:
        assert rf["accepted"] >= 1 and out["n_positive_depth"] >= s["rec"]["n_positive_depth"] and out["n_triangulated"] >= s["rec"]["n_triangulated"]
    else:
        assert out.tobytes() == s["rec"].tobytes()


@pytest.mark.parametrize("refine_params", [rtw.REFINE_DEFAULTS, TIGHT], ids=["defaults", "tight"])
def test_a_rotation_only_pair_does_not_stand_and_reaches_the_ceiling(host, refine_params):
    """Both cameras at one centre, exact coordinates: every translation direction explains the matches, the cost is rounding noise
    (~2e-25 px^2) and nothing triangulates, while the record claims all 120 matches in front and triangulated.  Steps are accepted on
    noise, then rejected: the result does NOT stand (status ELIGIBLE | STEP_ACCEPTED) and not one byte of the record changes; given room
    (max_iters 50) the damping passes its ceiling.  Which steps the noise accepts is rounding's; the status, and the ceiling, are not."""
    fields, q1, q2 = fx.exact_pair(rotation_only=True)
    rec = as_record(fields)
    out, rf = rtw.refine(host, rec, q1, q2, F, refine_params=refine_params)
    oL, rL = ref.refine(rec, q1, q2, F, refine_params=refine_params)
    print("rotation-only %s: twin status %d stop %d steps %d accepted %d; reference status %d stop %d steps %d accepted %d, counts after %d / %d" %
          (refine_params, rf["status"], rf["stop"], rf["steps"], rf["accepted"], rL["status"], rL["stop"], rL["steps"], rL["accepted"],
           rL["stats"]["n_positive_depth"], rL["stats"]["n_triangulated"]))
    assert rf["status"] == rL["status"] == (rtw.ELIGIBLE | rtw.STEP_ACCEPTED) and oL is None
    assert out.tobytes() == rec.tobytes() and rf["cost_after"] == rf["cost_before"] and rf["steps"] > rf["accepted"] >= 1
    if refine_params == TIGHT:
        assert rf["stop"] == rL["stop"] == ref.STOP_CEILING
    else:
        assert rf["stop"] == rL["stop"] == ref.STOP_MAX_ITERS and rf["steps"] == 10


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_coordinate_is_rejected_at_the_pivot_up_to_the_ceiling(host, bad):
    """A non-finite coordinate among the kept matches (the device's kept list cannot hold one: its Sampson test fails): the cost and
    every sum are NaN, so every step is rejected at the first pivot (not > 0) without a cost evaluation, eight times, until the damping
    passes its ceiling (1e-3 x 10^8 > 1e4).  Nothing is accepted, the record is untouched, and the NaN cost is handed out as THE NaN."""
    fields, q1, q2 = fx.exact_pair()
    rec = as_record(fields)
    q1 = q1.copy()
    q1[7, 0] = bad
    out, rf = rtw.refine(host, rec, q1, q2, F)
    o6, r6 = ref.refine(rec, q1, q2, F, dtype=np.float64)
    assert r6["trace"]["pivot_rejected"] == r6["steps"] == 8 and r6["stop"] == ref.STOP_CEILING and o6 is None
    assert (rf["status"], rf["stop"], rf["steps"], rf["accepted"]) == (rtw.ELIGIBLE, ref.STOP_CEILING, 8, 0)
    assert out.tobytes() == rec.tobytes()
    assert rf["cost_before"].tobytes() == rf["cost_after"].tobytes() == np.uint64(0x7ff8000000000000).tobytes()


def test_a_record_that_does_not_stand_equals_the_reference():
    """seed 5's records hold one pair whose refined pose loses a count: the standing rule keeps the old record.  The reference, on the same
    record and kept list, comes to the same verdict."""
    c = chain("s5")
    cap = c["cap"]
    out, rf = refined_records("s5")
    lost = np.nonzero((rf["status"] & (rtw.STEP_ACCEPTED | rtw.REFINED)) == rtw.STEP_ACCEPTED)[0]
    assert len(lost) == 1
    p = int(lost[0])
    offs, qt = c["lists"][:2]
    i, j = cap["pairs"][p]
    q1, q2 = rtw.kept_normalised(rtw.load_host(), cap["cam"], cap["kps"][int(i)], cap["kps"][int(j)], qt[offs[p]:offs[p + 1]])
    oL, rL = ref.refine(c["records"][p], q1, q2, (cap["cam"][0] + cap["cam"][1]) * 0.5, params=rfx.TWO_VIEW)
    print("does not stand: pair %d (%d, %d), counts %d / %d -> reference %d / %d; twin status %d stop %d steps %d, reference status %d stop %d steps %d" %
          (p, i, j, c["records"][p]["n_positive_depth"], c["records"][p]["n_triangulated"], rL["stats"]["n_positive_depth"],
           rL["stats"]["n_triangulated"], rf["status"][p], rf["stop"][p], rf["steps"][p], rL["status"], rL["stop"], rL["steps"]))
    assert oL is None and rL["status"] == rf["status"][p] == 3 and rL["stop"] == rf["stop"][p] and rL["accepted"] == rf["accepted"][p]
    assert out[p].tobytes() == c["records"][p].tobytes()
    assert abs(float(rL["cost_before"]) - rf["cost_before"][p]) <= 1e-12 * rf["cost_before"][p] and rf["cost_after"][p] == rf["cost_before"][p]


# ---- benefit against ground truth ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refined_records(name):
    c = chain(name)
    cap = c["cap"]
    out, rf = rtw.run(rtw.load_host(), c["records"], c["lists"][:2], cap["pairs"], cap["kps"], cap["cam"], params=rfx.TWO_VIEW)
    return out, rf


def medians(cap, records):
    rot, tra = record_errors(cap, records)
    return (float(np.median(rot)), float(rot.max()), float(np.median(tra)), float(tra.max())), rot, tra


@pytest.mark.parametrize("name", ("s77", "s5"))
def test_refined_records_are_closer_to_the_truth(name):
    c = chain(name)
    out, rf = refined_records(name)
    before, rot0, tra0 = medians(c["cap"], c["records"])
    after, rot1, tra1 = medians(c["cap"], out)
    refined = (rf["status"] & rtw.REFINED) != 0
    print("records[%s] rotation median / max, direction median / max (degrees): %.4g / %.4g / %.4g / %.4g -> %.4g / %.4g / %.4g / %.4g; "
          "refined %d of %d; rotation error grows for %.1f %%, direction error for %.1f %%; stops %s" %
          ((name,) + before + after + (int(refined.sum()), len(rf), 100 * float((rot1 > rot0).mean()), 100 * float((tra1 > tra0).mean()),
                                       np.bincount(rf["stop"], minlength=4).tolist())))
    assert after[0] < before[0] and after[2] < before[2]
    want = REFINED_RECORDS[name]
    assert after[0] <= 2.0 * want[0] and after[2] <= 2.0 * want[2], (after, want)
    assert out[~refined].tobytes() == c["records"][~refined].tobytes() and int(refined.sum()) >= 270
    assert np.array_equal(out["n_kept"], c["records"]["n_kept"])


@pytest.mark.parametrize("seed", (77, 5))
def test_without_noise_the_refined_errors_stay_orders_of_magnitude_smaller(seed):
    noisy = medians(chain("s%d" % seed)["cap"], refined_records("s%d" % seed)[0])[0]
    clean = medians(chain("s%d-clean" % seed)["cap"], refined_records("s%d-clean" % seed)[0])[0]
    print("records[s%d-clean] refined %s against noisy %s" % (seed, clean, noisy))
    assert clean[0] <= noisy[0] / 100.0 and clean[2] <= noisy[2] / 100.0
    want = REFINED_RECORDS["s%d-clean" % seed]
    assert clean[0] <= 2.0 * want[0] and clean[2] <= 2.0 * want[2]


# ---- the chain -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refined_chain(name, min_points=rfx.MIN_POINTS):
    cap = rfx.variant(name)
    ctx = TwinContext()
    lists, records, _ = rfx.open_session(ctx, cap)
    out, rf = rtw.run(rtw.load_host(), records, lists[:2], cap["pairs"], cap["kps"], cap["cam"], params=rfx.TWO_VIEW)
    two_view = rfx.two_view_dict(cap, out)
    pair, trials, init = ctx.initialize(cap["cam"], two_view, min_points=min_points)
    loop = ctx.reconstruct(cap["cam"], **rfx.LOOP)
    batch = ctx.reconstruct(cap["cam"], **rfx.BATCH)
    return dict(cap=cap, ctx=ctx, pair=pair, record=two_view[pair], init=init, loop=loop, batch=batch, figures=rfx.measure(cap, ctx))


@pytest.mark.parametrize("name", NOISY + CLEAN)
def test_the_chain_from_refined_records(name):
    c = refined_chain(name)
    print("figures[%s, refined records] pair %s %s" % (name, c["pair"], {k: float("%.4g" % v) for k, v in c["figures"].items()}))
    assert sorted(c["ctx"].poses()) == sorted(int(i) for i in c["cap"]["ids"]), "every one of the 24 images must end posed"
    assert rfx.within(c["figures"], name, REFINED_CHAIN) == []


def test_the_start_that_ended_eleven_degrees_off():
    """initialize(min_points=30) on seed 77: unrefined, the chain starts from the pair (10, 1), whose record is 3.3 degrees off, and
    ends 11 degrees and 1.9 scene units off (tests/test_reconstruction_reference.py).  With refined records it starts from the same
    pair, whose record is now a fraction of a degree off, and ends inside the seed-77 bound."""
    c = refined_chain("s77", 30)
    R, t = rfx.relative_pose(c["cap"], *c["pair"])
    off = (rfx.angle_deg(c["record"]["R"], R), rfx.direction_deg(c["record"]["t"], t))
    print("initialize(min_points=30)[s77, refined records] pair %s, record %.3g / %.3g degrees off, %d points; figures %s" %
          (c["pair"], off[0], off[1], c["init"]["succeeded"], {k: float("%.4g" % v) for k, v in c["figures"].items()}))
    assert c["pair"] == (10, 1) and off[0] < 1.0
    assert sorted(c["ctx"].poses()) == sorted(int(i) for i in c["cap"]["ids"])
    assert rfx.within(c["figures"], "s77", REFINED_CHAIN) == []
