"""The map alignment's host twins (csrc/msfm_align.h through libmsfm_host.so, tests/align_twin.py) against tests/align_ref.py, an
independent numpy reference in long double (Umeyama through np.linalg.svd, its own errors, its own transform).  The reference does not
replay the sampler: every robust scene has ONE consensus set (gross outliers moved by >= 50 x max_error, inlier noise sigma <=
max_error / 8, no inlier within 1e-6 relative of the threshold), so the twin's final inlier set and model are the reference's fit of the
planted set.  The bounds are 16 x the reference's own scatter, long double against double on the same inputs, the worst per quantity
over the compared scenes (scatter() and transform_scatter() below; measured: s 4.2e-16 relative, Q 2.0e-14, d 5.8e-15 of |d| = 1e3,
errors 6.2e-13; after a transform residuals 2.3e-12 px, angles 9.4e-13 degrees, poses 2.8e-16 relative -- DESIGN.md section 28).  The chain: section
26's reconstruction on the twins for seeds 77 and 5, aligned to the true centres under a known similarity with three gross outliers,
then held against the truth directly."""
import functools

import numpy as np
import pytest

import align_ref as ar
import align_twin as atw
import reconstruction_fixtures as rfx
import refine_points_twin as rtw
import refine_poses_fixtures as pfx
import refine_poses_twin as ptw
import robust_triangulation_twin as robtw
import triangulation_twin as tw
import twin_host as th
from monocularsfm_amd import _lib
from test_robust_triangulation_reference import corrupted
from test_triangulation_reference import CAM, capture

LD = ar.LD
OK = _lib.ALN_ATTEMPTED | _lib.ALN_MODEL | _lib.ALN_SUCCEEDED
THR = (2.0, 1.5)
MAX_ERROR = 0.05


@pytest.fixture(scope="module")
def host():
    return atw.load_host()


def similarity(seed, s=40.0, far=1e3):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=3)
    return s, ar.random_rotation(rng), d * far / np.linalg.norm(d)


@functools.lru_cache(maxsize=None)
def cameras(name):
    """-> (ids, poses, centres [m, 3] as the library computes them: float64)"""
    if name == "capture":
        cap = rfx.variant("s77")
        ids, poses = np.asarray(sorted(cap["poses"]), np.int32), cap["poses"]
    else:
        ids, poses = pfx.ring_cameras(int(name))
    C = np.zeros((len(ids), 3))
    for k, i in enumerate(ids):                      # msfm_tri::centre itself: the centres the call will see, to the bit
        R, t = (np.ascontiguousarray(v, np.float64) for v in poses[int(i)])
        atw.load_host().host_tri_centre(R.ctypes.data_as(th.DP), t.ctypes.data_as(th.DP), C[k].ctypes.data_as(th.DP))
    return ids, poses, C


SETS = ("capture", "3", "4", "255", "256", "257")


def noisy_priors(name, seed, sigma=MAX_ERROR / 8, outliers=()):
    ids, poses, C = cameras(name)
    rng = np.random.default_rng(seed)
    s, Q, d = similarity(seed)
    p = s * C @ Q.T + d + rng.normal(0, sigma, C.shape)
    for k in outliers:
        g = rng.normal(size=3)
        p[k] += g / np.linalg.norm(g) * 50 * MAX_ERROR * rng.uniform(1.0, 40.0)
    return ids, poses, C, p


def diffs(a, b):
    """(s relative, Q absolute, d relative to |d|) between two similarities"""
    return (abs(float(a[0] - b[0])) / abs(float(b[0])), float(np.abs(np.asarray(a[1], LD) - np.asarray(b[1], LD)).max()),
            float(np.abs(np.asarray(a[2], LD) - np.asarray(b[2], LD)).max() / np.abs(np.asarray(b[2], LD)).max()))


@functools.lru_cache(maxsize=None)
def scatter():
    """the reference's own rounding scatter: long double against double on the compared fits, the worst per quantity; and the errors'"""
    w = np.zeros(4)
    for name in SETS:
        for seed in (1, 2):
            _, _, C, p = noisy_priors(name, seed)
            a, b = ar.umeyama(C, p, LD), ar.umeyama(C, p, np.float64)
            e = np.abs(ar.errors(*a, C, p, LD) - ar.errors(*b, C, p, np.float64)).max()
            w = np.maximum(w, diffs(b, a) + (float(e),))
    return dict(zip(("s", "Q", "d", "error"), w))


def close(got, want, tol):
    d = diffs(got, want)
    return d[0] <= 16 * tol["s"] and d[1] <= 16 * tol["Q"] and d[2] <= 16 * tol["d"], d


def test_scatter_is_measured():
    w = scatter()
    print("scatter (reference, long double against double) %s; bounds x16 %s" % (w, {k: 16 * v for k, v in w.items()}))
    # 2 x the figures measured (the module's docstring): the 16 x bounds below cannot grow unnoticed
    assert w["s"] <= 2 * 4.2e-16 and w["Q"] <= 2 * 2.0e-14 and w["d"] <= 2 * 5.8e-15 and w["error"] <= 2 * 6.2e-13


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("seed", [1, 2])
def test_fit_equals_the_reference(host, name, seed):
    ids, poses, C, p = noisy_priors(name, seed)
    want = ar.umeyama(C, p)
    ok, s, Q, d = atw.fit(host, C, p)
    fine, dd = close((s, Q, d), want, scatter())
    print("fit %s seed %d: s, Q, d differ by %s" % (name, seed, dd))
    assert ok and fine, dd
    assert np.abs(Q.T @ Q - np.eye(3)).max() <= 1e-12 and np.linalg.det(Q) > 0 and s > 0
    # the least-squares route of the call is that fit, every prior an inlier
    a, rec = atw.estimate(host, ids, poses, {int(i): p[k] for k, i in enumerate(ids)})
    assert a["status"] == OK | _lib.ALN_LEAST_SQUARES and a["hypotheses"] == 0 and a["refits"] == 0 and a["n_inliers"] == len(ids)
    assert (a["s"], a["Q"].tobytes(), a["d"].tobytes()) == (s, Q.tobytes(), d.tobytes()) and np.all(rec["flags"] == 3)
    e = ar.errors(*want, C, p)
    assert np.abs(rec["error"] - e).max() <= 16 * scatter()["error"]
    assert abs(a["rms"] - float(np.sqrt((e * e).mean()))) <= 16 * scatter()["error"]


def test_scale_sign_on_random_sets_in_general_position(host):
    """500 random six-prior sets in general position (sigma2 is not small): the scale needs the sign of det U det V, which the ordering
    network's swaps hide from a3 . u3 alone.  The twin's scale equals the reference's on every one, to 1e-12 relative (the sets are
    well conditioned: a wrong sign is off by 2 sigma2 / va, tens of percent)."""
    rng = np.random.default_rng(8)
    worst = 0.0
    for _ in range(500):
        C = rng.normal(size=(6, 3))
        p = 2.0 * C @ ar.random_rotation(rng).T + 5.0 + rng.normal(0, 0.01, C.shape)
        ok, s, Q, d = atw.fit(host, C, p)
        worst = max(worst, abs(s - float(ar.umeyama(C, p)[0])) / s)
        assert ok and np.linalg.det(Q) > 0
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("name,n_out,seed", [("capture", 3, 1), ("257", 64, 1), ("capture", 0, 2), ("256", 1, 2), ("4", 1, 3)])
def test_robust_estimate_finds_the_planted_set(host, name, n_out, seed):
    m = len(cameras(name)[0])
    out = sorted(np.random.default_rng(seed + 40).choice(m, n_out, replace=False).tolist())
    ids, poses, C, p = noisy_priors(name, seed, outliers=out)
    keep = np.ones(m, bool)
    keep[out] = False
    want = ar.umeyama(C[keep], p[keep])
    e = ar.errors(*want, C, p)
    # the scene is decidable: no inlier's error on the threshold, every planted outlier far beyond it
    assert np.abs(e[keep] / MAX_ERROR - 1).min() > 1e-6 and e[keep].max() < MAX_ERROR and (n_out == 0 or e[~keep].min() > 49 * MAX_ERROR)
    a, rec = atw.estimate(host, ids, poses, {int(i): p[k] for k, i in enumerate(ids)}, max_error=MAX_ERROR)
    inl = (rec["flags"] & _lib.ALN_INLIER) != 0
    assert a["status"] & OK == OK and not a["status"] & _lib.ALN_LEAST_SQUARES and np.array_equal(inl, keep), (a, np.nonzero(inl != keep)[0])
    assert a["n_inliers"] == keep.sum() and a["n_used"] == a["n_listed"] == m and 1 <= a["hypotheses"] <= 1024
    fine, dd = close((a["s"], a["Q"], a["d"]), want, scatter())
    print("robust %s, %d outliers: %d hypotheses, %d refits, s, Q, d differ by %s" % (name, n_out, a["hypotheses"], a["refits"], dd))
    assert fine, dd
    assert np.abs(rec["error"] - e).max() <= 16 * scatter()["error"]
    assert np.array_equal(inl, rec["error"] <= MAX_ERROR) and np.all(rec["flags"] & _lib.ALN_USED)
    # a fixed point of refit-and-recount, or the refits ran out
    ok, s, Q, d = atw.fit(host, C[inl], p[inl])
    again = np.asarray(ar.errors(s, Q, d, C, p), np.float64) <= MAX_ERROR
    assert ok and (np.array_equal(again, inl) or a["refits"] == atw.K_REFITS)
    assert abs(a["rms"] - float(np.sqrt((e[keep] ** 2).mean()))) <= 16 * scatter()["error"]


def test_edges(host):
    ids, poses, C, p = noisy_priors("capture", 4, sigma=0.0)
    pos = {int(i): p[k] for k, i in enumerate(ids)}
    first = lambda n: {int(i): pos[int(i)] for i in ids[:n]}   # noqa: E731
    # three priors: one hypothesis
    a, rec = atw.estimate(host, ids, poses, first(3), max_error=MAX_ERROR)
    assert a["status"] & OK == OK and a["hypotheses"] == 1 and a["n_inliers"] == 3
    # two usable priors: not attempted; a listed image without a pose is reported as unused
    a, rec = atw.estimate(host, ids, poses, first(2), max_error=MAX_ERROR)
    assert a["status"] == 0 and a["n_used"] == 2 and np.all(rec["flags"] == _lib.ALN_USED) and np.all(rec["error"] == -1.0)
    some = {i: (None if k in (1, 3) else q) for k, (i, q) in enumerate(sorted(poses.items()))}
    a, rec = atw.estimate(host, ids, some, pos, max_error=MAX_ERROR)
    assert a["n_listed"] == 24 and a["n_used"] == 22 == a["n_inliers"] and list(np.nonzero(rec["flags"] == 0)[0]) == [1, 3]
    assert np.all(rec["error"][[1, 3]] == -1.0) and a["status"] & OK == OK
    a, _ = atw.estimate(host, ids, {i: some[i] for i in list(some)[:4]}, first(4))
    assert a["status"] == 0 and a["n_used"] == 2
    # exactly collinear centres, both routes: attempted, no model
    line = {int(i): (np.eye(3), np.asarray([-0.3 * k, 0.0, 6.5])) for k, i in enumerate(ids)}
    for kw in (dict(max_error=MAX_ERROR), {}):
        a, rec = atw.estimate(host, ids, line, pos, **kw)
        assert a["status"] & ~_lib.ALN_LEAST_SQUARES == _lib.ALN_ATTEMPTED and a["s"] == 0.0 and not a["Q"].any() and not a["d"].any()
    # all priors at one spot (M = 0), all centres at one spot (va = 0)
    for bad in (atw.estimate(host, ids, poses, {int(i): (1.0, 2.0, 3.0) for i in ids}, max_error=MAX_ERROR),
                atw.estimate(host, ids, {int(i): poses[int(ids[0])] for i in ids}, pos)):
        assert bad[0]["status"] & ~_lib.ALN_LEAST_SQUARES == _lib.ALN_ATTEMPTED
    # a mirrored prior set is no similarity of the centres: Q stays a proper rotation, nothing fits within max_error
    mirrored = {i: q * (1.0, 1.0, -1.0) for i, q in pos.items()}
    a, rec = atw.estimate(host, ids, poses, mirrored)
    want = ar.umeyama(C, np.stack([mirrored[int(i)] for i in ids]))
    assert a["status"] & OK == OK and np.linalg.det(a["Q"]) > 0 and np.abs(a["Q"].T @ a["Q"] - np.eye(3)).max() <= 1e-12
    assert close((a["s"], a["Q"], a["d"]), want, scatter())[0] and rec["error"].max() > 100 * MAX_ERROR
    # min_inliers above the consensus: a model, no success
    a, rec = atw.estimate(host, ids, poses, pos, max_error=MAX_ERROR, min_inliers=25)
    assert a["status"] == _lib.ALN_ATTEMPTED | _lib.ALN_MODEL and a["n_inliers"] == 24 and a["s"] == 0.0 and np.all(rec["error"] == -1.0)
    # every MSFM_E_INVALID
    for kw, args in ((dict(max_error=MAX_ERROR, max_hypotheses=4097), pos), (dict(max_error=MAX_ERROR, max_hypotheses=-1), pos),
                     (dict(max_error=0.0), pos), (dict(max_error=np.inf), pos), (dict(max_error=np.nan), pos),
                     (dict(max_error=MAX_ERROR, confidence=1.0), pos), (dict(confidence=0.0), pos),
                     ({}, {**pos, int(ids[3]): (np.nan, 0.0, 0.0)}), ({}, {**pos, 2: (0.0, 0.0, 0.0)})):
        with pytest.raises(_lib.MsfmError) as e:
            atw.estimate(host, ids, poses, args, **kw)
        assert e.value.code == _lib.E_INVALID, kw
    with pytest.raises(_lib.MsfmError) as e:                     # an id given twice
        atw.estimate(host, ids, poses, None, listed=(ids[[0, 1, 0]], p[[0, 1, 0]]))
    assert e.value.code == _lib.E_INVALID


# ---- the transform ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_map(kind, seed):
    """scene_job's capture of `seed` triangulated under the true poses: plain, robust (with corrupted observations), or refined (points,
    then poses) -> dict(c: the capture, poses: the pose list, state: (points, residuals, mask))"""
    host = atw.load_host()
    if kind == "robust":
        c = corrupted(seed, CAM)
        pp, pr, pm, _ = robtw.run(host, c["tracks"], c["ids"], c["kps"], c["poses"], CAM, THR + (2, 64))
        return dict(c=c, poses=_lib.pose_table(c["poses"]), state=(pp, pr, pm))
    c = capture(seed, cam=CAM)
    pp, pr = tw.run(host, c["tracks"], c["ids"], c["kps"], c["poses"], CAM, THR + (2,))
    poses = _lib.pose_table(c["poses"])
    if kind == "refined":
        pp, pr, _ = rtw.run(host, c["tracks"], c["ids"], c["kps"], poses, CAM, pp, pr, None, THR, (10, 1e-10))
        pp, pr, poses, _, _ = ptw.run(host, c["tracks"], c["ids"], c["kps"], poses, CAM, pp.copy(), pr.copy(), None, THR, (10, 1e-6, 15), [])
    return dict(c=c, poses=(poses[0].copy(), poses[1].copy()), state=(pp.copy(), pr.copy(), None))


def moved(host, m, sim, state=None, poses=None):
    pp, pr, pm = state or m["state"]
    c = m["c"]
    return atw.transform(host, c["tracks"], c["ids"], c["kps"], poses or m["poses"], CAM, pp, pr, pm, THR, *sim)


def ref_after(m, sim, dtype, stride=7):
    """the reference's transform: every pose and every 7th standing point moved, the residuals of the point's used observations and its
    pairwise parallax angles computed at the new place -> (residuals {(track, element): px}, angles {(track, i, j): degrees}, poses)"""
    c, (ids, tab), (pp, pr, pm) = m["c"], m["poses"], m["state"]
    offs, img, idx = c["tracks"][:3]
    new = {int(i): ar.transform_pose(*sim, q["R"], q["t"], dtype) for i, q in zip(ids, tab) if q["valid"]}
    f = dtype((CAM[0] + CAM[1]) / 2)
    res, ang = {}, {}
    for t in np.nonzero((pp["status"] & 14) == 14)[0][::stride]:
        X = ar.transform_points(*sim, pp[t]["X"], dtype)
        el = [e for e in range(int(offs[t]), int(offs[t + 1])) if int(img[e]) in new]
        for e in el:
            k = c["kps"][int(img[e])][int(idx[e])]
            uw = ((dtype(k[0]) - dtype(CAM[2])) / dtype(CAM[0]), (dtype(k[1]) - dtype(CAM[3])) / dtype(CAM[1]))
            res[(int(t), e)] = ar.reprojection(*new[int(img[e])], X, f, uw, dtype)
        O = [ar.centre(*new[int(img[e])], dtype) for e in el]
        for i in range(1, len(el)):
            for j in range(i):
                a, b = X - O[i], X - O[j]
                ang[(int(t), i, j)] = np.degrees(np.arccos(np.clip((a @ b) / np.sqrt((a @ a) * (b @ b)), -1, 1)))
    return res, ang, new


MAPS = [(k, s) for s in (77, 5) for k in ("plain", "robust", "refined")]


@functools.lru_cache(maxsize=None)
def transform_scatter():
    w = np.zeros(3)
    for kind, seed in MAPS:
        m, sim = scene_map(kind, seed), similarity(seed + 10)
        (ra, aa, pa), (rb, ab, pb) = ref_after(m, sim, LD), ref_after(m, sim, np.float64)
        w = np.maximum(w, (max(abs(float(ra[k] - rb[k])) for k in ra), max(abs(float(aa[k] - ab[k])) for k in aa),
                           max(float(max(np.abs(pa[i][0] - pb[i][0]).max(), np.abs(pa[i][1] - pb[i][1]).max() / np.abs(pa[i][1]).max()))
                               for i in pa)))
    return dict(zip(("residual", "angle", "pose"), w))


def test_transform_scatter_is_measured():
    w = transform_scatter()
    print("transform scatter (reference, long double against double) %s; bounds x16 %s" % (w, {k: 16 * v for k, v in w.items()}))
    assert w["residual"] <= 2 * 2.3e-12 and w["angle"] <= 2 * 9.4e-13 and w["pose"] <= 2 * 2.8e-16


@pytest.mark.parametrize("kind,seed", MAPS)
def test_identity_changes_nothing_but_the_bits_it_says(host, kind, seed):
    m = scene_map(kind, seed)
    pp, pr, pm = m["state"]
    (ids, tab), gp, gr, counts = moved(host, m, (1.0, np.eye(3), np.zeros(3)))
    assert gp["X"].tobytes() == pp["X"].tobytes() and all(np.array_equal(tab[k], m["poses"][1][k]) for k in ("valid", "R", "t"))
    el = (pp["status"] & 3) == 3
    assert np.array_equal(gp["status"][el], (pp["status"][el] & ~_lib.TRI_RECALIBRATED) | _lib.TRI_ALIGNED)
    assert np.array_equal(gp["status"][~el], pp["status"][~el]) and np.array_equal(gp["n_views"], pp["n_views"])
    assert gr.tobytes() == pr.tobytes() and gp["mean_residual"].tobytes() == pp["mean_residual"].tobytes()
    assert counts == dict(poses_transformed=24, points_transformed=int(el.sum()), points_lost=0, points_gained=0,
                          succeeded=int(((pp["status"] & 14) == 14).sum()))


@pytest.mark.parametrize("kind,seed", MAPS)
def test_a_general_similarity_moves_the_map_and_keeps_every_verdict(host, kind, seed):
    m, sim = scene_map(kind, seed), similarity(seed + 10)
    pp, pr, pm = m["state"]
    tol = {k: 16 * v for k, v in transform_scatter().items()}
    used = pr >= 0
    assert np.abs(pr[used] - THR[0]).min() > 1e-6, "a residual on the threshold: the verdict would be rounding's"
    assert np.abs(pp["tri_angle"][(pp["status"] & 3) == 3] - THR[1]).min() > 1e-9, "an angle on the threshold"
    (ids, tab), gp, gr, counts = moved(host, m, sim)
    assert counts["points_lost"] == counts["points_gained"] == 0 and counts["poses_transformed"] == 24
    el = (pp["status"] & 3) == 3
    assert np.array_equal(gp["status"][el], (pp["status"][el] & ~_lib.TRI_RECALIBRATED) | _lib.TRI_ALIGNED) and _lib.aligned(gp[el]).all()
    assert np.array_equal(gr < 0, pr < 0) and np.array_equal(gp["n_views"], pp["n_views"])
    ok = (pp["status"] & 14) == 14
    worst = (np.abs(gr[used] - pr[used]).max(), np.abs(gp["mean_residual"][ok] - pp["mean_residual"][ok]).max(),
             np.abs(gp["tri_angle"][ok] - pp["tri_angle"][ok]).max())
    print("transform %s %d: residuals move by %.3g px, mean_residual %.3g px, tri_angle %.3g degrees" % ((kind, seed) + worst))
    # against the reference at the new place, and against the figures before the call
    res, ang, new = ref_after(m, sim, LD)
    assert max(abs(float(gr[e] - v)) for (t, e), v in res.items() if pr[e] >= 0) <= tol["residual"]
    assert worst[0] <= tol["residual"] and worst[1] <= tol["residual"] and worst[2] <= tol["angle"]
    for i, q in zip(ids, tab):
        R, t = new[int(i)]
        assert np.abs(q["R"].reshape(3, 3) - R).max() <= tol["pose"] and np.abs(q["t"] - t).max() <= tol["pose"] * float(np.abs(t).max())
    X = ar.transform_points(*sim, pp["X"][ok])
    assert np.abs(gp["X"][ok] - X).max() <= tol["pose"] * float(np.abs(X).max())
    # the inverse brings everything back (not bitwise)
    (ids2, tab2), bp, br, c2 = moved(host, m, tuple(np.asarray(v, np.float64) for v in ar.inverse(*sim)), (gp, gr, pm), (ids, tab))
    assert c2["points_lost"] == c2["points_gained"] == 0
    scale = float(np.abs(gp["X"][ok]).max()) / sim[0]               # the rounding of the far frame, seen from the near one
    assert np.abs(bp["X"][ok] - pp["X"][ok]).max() <= tol["pose"] * scale
    assert np.abs(tab2["R"] - m["poses"][1]["R"]).max() <= tol["pose"] and np.abs(tab2["t"] - m["poses"][1]["t"]).max() <= tol["pose"] * scale
    assert np.abs(br[used] - pr[used]).max() <= tol["residual"]


def test_transform_refuses_what_is_no_similarity_and_overflows_by_the_rule(host):
    m = scene_map("plain", 77)
    pp, pr, _ = m["state"]
    for bad in ((0.0, np.eye(3), np.zeros(3)), (-1.0, np.eye(3), np.zeros(3)), (np.nan, np.eye(3), np.zeros(3)),
                (1.0, np.diag([1.0, 1.0, -1.0]), np.zeros(3)), (1.0, np.eye(3) * (1 + 1e-8), np.zeros(3)), (1.0, np.eye(3), (0.0, np.inf, 0.0)),
                (1e308, np.eye(3), np.zeros(3))):                 # the last: s t overflows -- a new pose would not be finite
        with pytest.raises(_lib.MsfmError) as e:
            moved(host, m, bad)
        assert e.value.code == _lib.E_INVALID
        held = e.value.held                                       # what the twin worked on: not one byte of the map changed
        assert held.poses.tobytes() == m["poses"][1].tobytes() and held.pose_ids.tobytes() == m["poses"][0].tobytes()
        assert held.points[:held.T].tobytes() == pp.tobytes() and held.residuals[:held.O].tobytes() == pr.tobytes()
    # s = 1e300: poses and points stay finite, the verdict's squares do not: every point is lost, by the verdict
    (ids, tab), gp, gr, counts = moved(host, m, (1e300, similarity(1)[1], np.zeros(3)))
    ok = (pp["status"] & 14) == 14
    assert np.isfinite(gp["X"]).all() and np.isfinite(tab["t"]).all() and counts["points_lost"] == ok.sum() and counts["succeeded"] == 0
    # the overflow rule itself: cameras near the origin, points far from it, s t finite and s X not
    c = m["c"]
    near = {i: (R, np.asarray(t) * 1e-3) for i, (R, t) in c["poses"].items()}
    far = pp.copy()
    far["X"][ok] *= 4.0
    (ids, tab), gp, gr, counts = atw.transform(host, c["tracks"], c["ids"], c["kps"], near, CAM, far, pr, None, THR, 1e308, np.eye(3), np.zeros(3))
    with np.errstate(over="ignore"):
        lost = ok & ~np.isfinite(far["X"] * 1e308).all(1)
    assert lost.sum() > 100 and counts["points_lost"] >= lost.sum()
    assert np.all(gp["status"][lost] == _lib.TRI_ATTEMPTED | _lib.TRI_ALIGNED) and not gp["X"][lost].any() and not gp["n_views"][lost].any()
    offs = c["tracks"][0]
    assert all(np.all(gr[offs[t]:offs[t + 1]] == -1.0) for t in np.nonzero(lost)[0][:50])


# ---- the chain --------------------------------------------------------------------------------------------------------------------------------
# measured on the twin chain (test_chain_figures prints them): the largest centre error in the PRIOR's units (the similarity has s = 40:
# section 26's scene units x 40) and the largest rotation error in degrees, both directly against the truth after align
CHAIN = {"s77": dict(centre_max=0.2310, rotation_max=0.1459), "s5": dict(centre_max=2.385, rotation_max=1.180)}
# max_error of the chain's estimate, in the prior's units: 2 x section 26's measured centre error of the worse seed (0.063 scene units)
# under s = 40
CHAIN_MAX_ERROR = 5.0
PLANTED = (2, 9, 17)


def chain_priors(cap):
    sim = similarity(cap["seed"])
    order = sorted(cap["poses"])
    rng = np.random.default_rng(cap["seed"] + 1)
    pos = {}
    for k, i in enumerate(order):
        R, t = cap["poses"][i]
        pos[i] = sim[0] * sim[1] @ (-R.T @ t) + sim[2]
        if k in PLANTED:
            g = rng.normal(size=3)
            pos[i] = pos[i] + g / np.linalg.norm(g) * 60 * CHAIN_MAX_ERROR
    return sim, order, pos


def against_truth(cap, ctx, sim):
    s, Q, d = sim
    ce, re = [], []
    for i, (R, t) in ctx.poses().items():
        Rt, tt = cap["poses"][i]
        ce.append(float(np.linalg.norm(-R.T @ t - (s * Q @ (-Rt.T @ tt) + d))))
        re.append(rfx.angle_deg(R, Rt @ Q.T))
    return dict(centre_max=max(ce), rotation_max=max(re))


@functools.lru_cache(maxsize=None)
def chain(name, align_after):
    """section 26's chain on the twins; align after `align_after` increments (None: at the end) -> (ctx, alignment, records, stats)"""
    cap = rfx.variant(name)
    sim, order, pos = chain_priors(cap)
    ctx = atw.AlignTwinContext()
    _, records, _ = rfx.open_session(ctx, cap)
    ctx.initialize(cap["cam"], rfx.two_view_dict(cap, records), min_points=rfx.MIN_POINTS)
    got = None
    for k, _ in enumerate(rfx.increments(ctx, cap["cam"])):
        if k + 1 == align_after:
            got = ctx.align(pos, max_error=CHAIN_MAX_ERROR)
    if align_after is None:
        got = ctx.align(pos, max_error=CHAIN_MAX_ERROR)
    return (ctx,) + got


@pytest.mark.parametrize("name", ["s77", "s5"])
def test_chain_figures(name):
    cap = rfx.variant(name)
    sim, order, pos = chain_priors(cap)
    ctx, a, rec, st = chain(name, None)
    f = against_truth(cap, ctx, sim)
    print("chain %s: %s, %d inliers of %d, %d hypotheses, %d refits, rms %.4g" % (name, f, a["n_inliers"], a["n_used"], a["hypotheses"],
                                                                                a["refits"], a["rms"]))
    assert a["status"] & OK == OK and sorted(ctx.poses()) == order and st["points_lost"] == st["points_gained"] == 0
    assert [k for k, r in enumerate(rec) if not r["flags"] & _lib.ALN_INLIER] == list(PLANTED)
    assert f["centre_max"] <= 2 * CHAIN[name]["centre_max"] and f["rotation_max"] <= 2 * CHAIN[name]["rotation_max"]


@pytest.mark.parametrize("name", ["s77", "s5"])
def test_a_map_aligned_midway_ends_where_the_map_aligned_at_the_end_does(name):
    cap = rfx.variant(name)
    sim, order, pos = chain_priors(cap)
    (end, a, _, _), (mid, b, _, st) = chain(name, None), chain(name, 10)
    assert b["status"] & OK == OK and st is not None and b["n_used"] == 12
    assert sorted(mid.poses()) == order                                   # registration, extension, refinement, filter and completion went on
    f = against_truth(cap, mid, sim)
    print("chain %s aligned after ten increments: %s" % (name, f))
    assert f["centre_max"] <= 2 * CHAIN[name]["centre_max"] and f["rotation_max"] <= 2 * CHAIN[name]["rotation_max"]
    # the same reconstruction in another gauge: the two maps agree within the chain's own bound
    pe, pm = end.poses(), mid.poses()
    assert max(float(np.linalg.norm(-pe[i][0].T @ pe[i][1] + pm[i][0].T @ pm[i][1])) for i in order) <= 2 * CHAIN[name]["centre_max"]
    assert max(rfx.angle_deg(pe[i][0], pm[i][0]) for i in order) <= 2 * CHAIN[name]["rotation_max"]
    # the points: on the tracks that stand in both maps, against section 26's own point figures (scene units, x 40 under this
    # similarity), each map being that close to the truth
    xe, xm = end.points3d()[0], mid.points3d()[0]
    ok = ((xe["status"] & 14) == 14) & ((xm["status"] & 14) == 14)
    dist = np.linalg.norm(xe["X"][ok] - xm["X"][ok], axis=1)
    print("chain %s: points of the two maps differ by median %.4g, p95 %.4g (prior units) on %d common tracks" %
          (name, np.median(dist), np.percentile(dist, 95), ok.sum()))
    assert ok.mean() > 0.95
    assert np.median(dist) <= 2 * 40 * rfx.MEASURED[name]["point_median"] and np.percentile(dist, 95) <= 2 * 40 * rfx.MEASURED[name]["point_p95"]
