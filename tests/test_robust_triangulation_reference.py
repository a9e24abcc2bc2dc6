"""The robust track triangulation's host twin (monocularsfm_amd/csrc/msfm_triangulate.h, TriangulateTracksRobust, through
libmsfm_host.so and tests/robust_triangulation_twin.py) against the independent numpy reference tests/robust_triangulation_ref.py, on
tests/tracks_fixtures.scene_job's capture (seeds 77 and 5, with and without distortion, 0.3 px of noise) whose every fifth ground-truth
track has one observation moved by 40 px -- the first, a middle and the last position in turn -- and on hand-made edge cases.  CPU only.

Tolerances.  Worst differences twin - reference measured on the CPU over the four corrupted captures (python
tests/test_robust_triangulation_reference.py prints them):
    X              5.0e-13 (absolute; a scene of extent ~3 at distance ~6)
    residuals      1.9e-11 px  (mean_residual 6.6e-13)
    tri_angle      6.7e-13 degrees
The bounds are 16 x those, the project's rule:  TOL_X = 8.0e-12,  TOL_RES = 3.0e-10 px,  TOL_MEAN = 1.1e-11 px,  TOL_ANGLE = 1.1e-11
degrees.  A residual of a REJECTED observation is tens of pixels: the figures above are absolute
differences over all used observations, rejected ones included.
Guards, asserted on the reference alone before anything is compared: no error any decision looks at (the plain pass, every hypothesis'
score, both masks) lies within 16 x TOL_RES of max_error, no hypothesis or scanned angle within 16 x TOL_ANGLE of min_angle.  With
them the twin and the reference hold the same count for every hypothesis, so the stated tie rule (the lowest hypothesis among equal
counts) picks the same winner on both sides.  The third guard of the feature's description -- no retried track whose two best counts
are EQUAL -- cannot hold on any capture: a track with four or more clean views has several clean pairs, and every one of them
counts all clean views.  The number of such tracks is printed, not asserted (245 + 235 + 244 + 235 of the 266 + 271 + 266 + 271 retried tracks here)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import robust_triangulation_ref as rref  # noqa: E402
import robust_triangulation_twin as rtw  # noqa: E402
import triangulation_ref as ref  # noqa: E402
import triangulation_twin as tw  # noqa: E402
from test_triangulation_reference import CAM, CAM_D, capture  # noqa: E402
from monocularsfm_amd import synth  # noqa: E402

TOL_X = 8.0e-12
TOL_RES = 3.0e-10
TOL_MEAN = 1.1e-11
TOL_ANGLE = 1.1e-11
CASES = [(77, CAM), (5, CAM), (77, CAM_D), (5, CAM_D)]
OFFSET = (40.0, 0.0)


@pytest.fixture(scope="module")
def host():
    return rtw.load_host()


def corrupted(seed, cam):
    """the capture with every fifth track corrupted -> the capture dict plus chosen [(track, position)], moved (observation numbers)"""
    c = capture(seed, noise_px=0.3, cam=cam)
    o = c["tracks"][0]
    chosen = []
    for n, t in enumerate(range(0, len(o) - 1, 5)):
        length = int(o[t + 1] - o[t])
        chosen.append((t, (0, length // 2, length - 1)[n % 3]))
    kps, moved = synth.corrupt_observations(c["ids"], [c["kps"][int(i)] for i in c["ids"]], c["tracks"], chosen, OFFSET)
    c.update(clean_kps=c["kps"], kps={int(i): k for i, k in zip(c["ids"], kps)}, chosen=chosen, moved=moved)
    return c


_CACHE = {}


def case(seed, cam):
    """the corrupted capture and the reference's result on it, computed once"""
    key = (seed, cam)
    if key not in _CACHE:
        c = corrupted(seed, cam)
        c["want"] = rref.run(c["tracks"], c["kps"], c["poses"], c["cam"])
        _CACHE[key] = c
    return _CACHE[key]


def worst(want, got):
    """reference list against the twin's (points, residuals, mask, counts): equal status, n_views and masks on EVERY track; -> the
    worst differences"""
    pts, res, mask = got[:3]
    w = dict(X=0.0, res=0.0, mean=0.0, angle=0.0)
    at = 0
    for t, r in enumerate(want):
        n = len(r["residuals"])
        assert int(pts[t]["status"]) == r["status"], (t, int(pts[t]["status"]), r["status"])
        assert int(pts[t]["n_views"]) == r["n_views"], t
        assert np.array_equal(mask[at:at + n], r["mask"]), (t, mask[at:at + n], r["mask"])
        assert np.array_equal(res[at:at + n] < 0, r["residuals"] < 0), t
        if r["status"] & ref.POINT:
            w["X"] = max(w["X"], float(np.abs(pts[t]["X"] - r["X"]).max()))
            used = r["residuals"] >= 0
            w["res"] = max(w["res"], float(np.abs(res[at:at + n][used] - r["residuals"][used]).max()))
            w["mean"] = max(w["mean"], abs(float(pts[t]["mean_residual"]) - r["mean_residual"]))
            w["angle"] = max(w["angle"], abs(float(pts[t]["tri_angle"]) - r["tri_angle"]))
        at += n
    return w


def guards_hold(want):
    assert min(r["error_margin"] for r in want) > 16 * TOL_RES
    assert min(r["angle_margin"] for r in want) > 16 * TOL_ANGLE


def within(w):
    assert w["X"] <= TOL_X and w["res"] <= TOL_RES and w["mean"] <= TOL_MEAN and w["angle"] <= TOL_ANGLE, w


def counts_of(want):
    ret = [r for r in want if r["retried"]]
    return dict(retried=len(ret), rescued=sum((r["status"] & (ref.POINT | ref.ANGLE_OK)) == (ref.POINT | ref.ANGLE_OK) for r in ret),
                observations_rejected=sum(int((r["residuals"] >= 0).sum() - r["mask"].sum()) for r in ret if r["status"] & ref.POINT),
                hypotheses=sum(r["hypotheses"] for r in ret))


@pytest.mark.parametrize("seed,cam", CASES)
def test_twin_equals_reference_on_the_corrupted_capture(host, seed, cam):
    c = case(seed, cam)
    want = c["want"]
    guards_hold(want)
    assert sum(r["retried"] for r in want) >= len(c["chosen"]) // 2
    got = rtw.run(host, c["tracks"], c["ids"], c["kps"], c["poses"], c["cam"])
    w = worst(want, got)
    print("seed %d distortion %s: worst twin - reference %s; literal ties %d of %d retried" % (
        seed, bool(any(cam[4:])), w, sum(r["literal_tie"] for r in want), sum(r["retried"] for r in want)))
    within(w)
    assert got[3] == counts_of(want)


@pytest.mark.parametrize("seed,cam", CASES)
def test_recovery(host, seed, cam):
    """Every corrupted track with at least 3 clean posed views is rescued in the reference: its mask is 0 exactly on the moved
    observation and its point lies within the reference's own worst distance from the truth over the clean tracks."""
    c = case(seed, cam)
    want, o = c["want"], c["tracks"][0]
    hit = {t for t, _ in c["chosen"]}
    clean = [t for t in range(len(want)) if t not in hit and want[t]["status"] & ref.POINT]
    d_clean = max(float(np.linalg.norm(want[t]["X"] - c["X"][t])) for t in clean)
    n = 0
    for (t, pos), obs in zip(c["chosen"], c["moved"]):
        if int(o[t + 1] - o[t]) - 1 < 3:
            continue
        r = want[t]
        n += 1
        assert r["retried"] and (r["status"] & (ref.SUCCESS | rref.ROBUST)) == (ref.SUCCESS | rref.ROBUST), (t, r["status"])
        expect = np.ones(int(o[t + 1] - o[t]), np.uint8)
        expect[pos] = 0
        assert np.array_equal(r["mask"], expect) and obs == o[t] + pos, (t, r["mask"])
        assert float(np.linalg.norm(r["X"] - c["X"][t])) <= d_clean, (t, float(np.linalg.norm(r["X"] - c["X"][t])), d_clean)
    assert n > 100
    print("recovery: %d rescued tracks within the clean tracks' worst distance %.4g" % (n, d_clean))


@pytest.mark.parametrize("seed,cam", [(77, CAM), (5, CAM_D)])
def test_identity_with_the_plain_call_on_the_uncorrupted_job(host, seed, cam):
    c = capture(seed, noise_px=0.3, cam=cam)
    pp, pr = tw.run(host, c["tracks"], c["ids"], c["kps"], c["poses"], c["cam"])
    for prm in ((2.0, 1.5, 2, 64), (2.0, 1.5, 2, 1)):
        rp, rr, mask, cnt = rtw.run(host, c["tracks"], c["ids"], c["kps"], c["poses"], c["cam"], prm)
        if cnt["retried"] == 0:
            assert rp.tobytes() == pp.tobytes() and rr.tobytes() == pr.tobytes()
        same = (rp["status"] & rref.ROBUST) == 0          # (a clean capture may still hold a track whose plain point fails)
        assert same.sum() == len(rp) - cnt["retried"] and rp[same].tobytes() == pp[same].tobytes()
        used = np.repeat((pp["status"] & ref.ATTEMPTED) != 0, np.diff(c["tracks"][0]))
        o = c["tracks"][0]
        for t in np.nonzero(same)[0]:
            assert rr[o[t]:o[t + 1]].tobytes() == pr[o[t]:o[t + 1]].tobytes() and np.all(mask[o[t]:o[t + 1]] == used[o[t]:o[t + 1]])
    if seed == 5:   # every pure track of this capture succeeds (tests/test_triangulation_reference.py): nothing is retried
        assert cnt["retried"] == 0 and not (rp["status"] & rref.ROBUST).any() and np.all(mask == 1)


def hand(host, kps, poses, tracks, cam=CAM, params=rtw.DEFAULTS):
    ids = np.asarray(sorted(kps), np.int32)
    got = rtw.run(host, tracks, ids, kps, poses, cam, params)
    want = rref.run(tracks, kps, poses, cam, *params)
    guards_hold(want)
    within(worst(want, got))
    assert got[3] == counts_of(want)
    return got, want


def long_track(c, length):
    """the first track of the capture with at least `length` elements, cut to `length`, as a one-track result"""
    o, img, idx, _ = c["tracks"]
    t = int(np.nonzero(np.diff(o) >= length)[0][0])
    e = slice(int(o[t]), int(o[t]) + length)
    return (np.asarray([0, length], np.int64), img[e].copy(), idx[e].copy(), np.ones(1, np.uint8)), t


def moved(c, one, pos, offset=OFFSET):
    kps, _ = synth.corrupt_observations(c["ids"], [c["kps"][int(i)] for i in c["ids"]], one, [(0, pos)], offset)
    return {int(i): k for i, k in zip(c["ids"], kps)}


def test_further_cases(host):
    c = capture(5, noise_px=0.3)
    # m = 3 with one outlier: every pair is a hypothesis and each fits its own two views; the definition's answer, whatever it is
    one, _ = long_track(c, 3)
    (p, r, m, cnt), w = hand(host, moved(c, one, 1), c["poses"], one)
    assert cnt["retried"] == 1 and w[0]["hypotheses"] == 3 and int(p[0]["status"]) & rref.ROBUST
    # a rescue that leaves fewer than min_views = 3: four views, two of them moved apart -> at most two agree
    one, _ = long_track(c, 4)
    k2 = moved(c, one, 0, (40.0, 0.0))
    k2, _ = synth.corrupt_observations(c["ids"], [k2[int(i)] for i in c["ids"]], one, [(0, 3)], (0.0, -55.0))
    k2 = {int(i): k for i, k in zip(c["ids"], k2)}
    (p, r, m, cnt), w = hand(host, k2, c["poses"], one, params=(2.0, 1.5, 3, 64))
    assert int(p[0]["status"]) == ref.ATTEMPTED | rref.ROBUST and p[0].tobytes()[4:] == bytes(44) and np.all(r == -1.0) and not m.any()
    assert cnt == dict(retried=1, rescued=0, observations_rejected=0, hypotheses=6)
    # every pair below min_angle: no hypothesis is valid
    one, _ = long_track(c, 5)
    (p, r, m, cnt), w = hand(host, moved(c, one, 2), c["poses"], one, params=(2.0, 170.0, 2, 64))
    assert int(p[0]["status"]) == ref.ATTEMPTED | rref.ROBUST and not m.any() and cnt["rescued"] == 0
    # unposed elements interleaved with the outlier: positions are not elements
    one, _ = long_track(c, 7)
    poses = {i: (None if i in (int(one[1][1]), int(one[1][4])) else q) for i, q in c["poses"].items()}
    (p, r, m, cnt), w = hand(host, moved(c, one, 3), poses, one)
    assert m.tolist() == [1, 0, 1, 0, 0, 1, 1] and r[1] == -1.0 and r[4] == -1.0 and r[3] > 20.0 and int(p[0]["n_views"]) == 4
    assert (int(p[0]["status"]) & (ref.SUCCESS | rref.ROBUST)) == (ref.SUCCESS | rref.ROBUST) and cnt["observations_rejected"] == 1
    # m = 2 is never retried; an inconsistent track stays unattempted
    one, _ = long_track(c, 2)
    (p, r, m, cnt), w = hand(host, moved(c, one, 1), c["poses"], one)
    assert cnt["retried"] == 0 and not int(p[0]["status"]) & (rref.ROBUST | ref.ERROR_OK) and m.tolist() == [1, 1]
    one, _ = long_track(c, 5)
    (p, r, m, cnt), w = hand(host, moved(c, one, 2), c["poses"], one[:3] + (np.zeros(1, np.uint8),))
    assert p[0].tobytes() == bytes(48) and not m.any() and cnt["retried"] == 0


def test_sampled_hypotheses(host):
    """More pairs than max_hypotheses: sample2 against the Python integers, and a track whose hypotheses are sampled."""
    for track, m in ((0, 3), (7, 12), (123456789, 300)):
        for h in (0, 1, 63, 1023):
            got = rtw.sample2(host, track, h, m)
            assert got == rref.sample2(rref.mix64(rref.TRI_SEED ^ track), h, m) and got[0] != got[1] and 0 <= min(got) and max(got) < m
    c = capture(5, noise_px=0.3)
    one, _ = long_track(c, 12)
    for prm in ((2.0, 1.5, 2, 64), (2.0, 1.5, 2, 66), (2.0, 1.5, 2, 5)):
        (p, r, m, cnt), w = hand(host, moved(c, one, 11), c["poses"], one, params=prm)
        assert cnt["hypotheses"] == min(66, prm[3]) and cnt["retried"] == 1


if __name__ == "__main__":   # the figures of the module docstring
    h = rtw.load_host()
    tot = dict(X=0.0, res=0.0, mean=0.0, angle=0.0)
    for seed, cam in CASES:
        c = case(seed, cam)
        w = worst(c["want"], rtw.run(h, c["tracks"], c["ids"], c["kps"], c["poses"], c["cam"]))
        tot = {k: max(tot[k], w[k]) for k in tot}
        print(seed, bool(any(cam[4:])), w, "margins", min(r["error_margin"] for r in c["want"]), min(r["angle_margin"] for r in c["want"]),
              "retried", sum(r["retried"] for r in c["want"]), "literal ties", sum(r["literal_tie"] for r in c["want"]), counts_of(c["want"]))
    print("worst", tot)
