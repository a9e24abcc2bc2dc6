"""tests/triangulation_fixtures.py driven with the host twin (csrc/msfm_triangulate.h through tests/triangulation_twin.py): every planted
exit of triangulate_track sits at its lane with its status word, the numpy reference (tests/triangulation_ref.py) agrees wherever its
margins hold, and the equality, parameter and scan-order checks that tests/test_gpu_triangulation_edges.py runs on the device pass on
the twin.  CPU only."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_triangulation_reference as tb  # noqa: E402
import triangulation_fixtures as tf  # noqa: E402
import triangulation_ref as ref  # noqa: E402
import triangulation_twin as tw  # noqa: E402


@pytest.fixture(scope="module")
def host():
    return tw.load_host()


def reference_agrees(job, pts, res, cam=tf.CAM, params=tw.DEFAULTS, skip=()):
    """the reference on every track; where its margins hold (tb.margins_hold, track by track) the twin's status word and n_views are
    the reference's and the numbers lie within tb.within's tolerances.  -> the tracks compared"""
    kps = {int(i): k for i, k in zip(job["ids"], job["kps"])}
    want = ref.run(job["tracks"], kps, job["poses"], cam, *params)
    o = job["tracks"][0]
    compared = []
    for t, r in enumerate(want):
        if t in skip:
            continue
        try:
            tb.margins_hold([r])
        except AssertionError:
            continue
        if job.get("planted", {}).get(t) == "no_point":
            # t = 1e200: the definition's normal matrix holds r^T r ~ 1e400 = inf, so the twin has no point on every such track.  The
            # reference's SVD of the stacked rows does not square; in about one track of ten LAPACK's rounding leaves it an h[3] != 0
            # and a "point" some 1e200 away.  Either is the reference's way of saying what the twin says.
            assert r["status"] == ref.ATTEMPTED or np.abs(r["X"]).max() > 1e150, (t, r)
            assert int(pts[t]["status"]) == ref.ATTEMPTED and int(pts[t]["n_views"]) == r["n_views"] == 2
            compared.append(t)
            continue
        tb.within(tb.worst([r], (pts[t:t + 1], res[o[t]:o[t + 1]])))
        compared.append(t)
    return compared


@pytest.mark.parametrize("layout", range(len(tf.LAYOUTS)))
def test_planted_routes_sit_at_their_lanes(host, layout):
    """routes() raises unless exactly the planted tracks take their exits; the status words by position; the reference's status on
    every track whose margins hold, the planted ones among them; the neighbours of the tracks without residuals."""
    job = tf.routes_job(layout=layout)
    T = len(job["tracks"][0]) - 1
    assert T == tf.N_TRACKS and len(job["ids"]) < 1300 and set(np.diff(job["tracks"][0]).tolist()) == {2, 3, 4, 5}
    assert set(tf.EDGES) <= set(job["planted"]) and set(job["planted"].values()) == set(tf.ROUTES)
    for cam in (tf.CAM, tf.CAM_D):
        pts, res, found = tf.routes(host, job, cam)
        for p, r in job["planted"].items():
            assert int(pts[p]["status"]) == tf.ROUTE_STATUS[r] and bool(job["tracks"][3][p]) == (r != "inconsistent"), (p, r)
        bare = tf.neighbours_hold_residuals(job, pts, res)
        assert sorted(bare) == sorted(p for p, r in job["planted"].items() if r in tf.NO_RESIDUALS)
        if layout == 0:   # the layout of the prefixes: both neighbours succeed
            assert all(int(pts[nb]["status"]) == tf.SUCCEEDED for t in bare for nb in (t - 1, t + 1) if 0 <= nb < T)
        tf.verdicts_follow(job, pts, res, tw.DEFAULTS)
        compared = reference_agrees(job, pts, res, cam)
        assert len(compared) >= T - 4 and set(job["planted"]) <= set(compared), sorted(set(range(T)) - set(compared))


def test_every_route_stands_at_every_edge_lane():
    for lane in tf.EDGES:
        assert {plan[lane] for plan in tf.LAYOUTS} == set(tf.ROUTES), lane


@pytest.mark.parametrize("T", tf.PREFIXES)
def test_a_prefix_is_the_same_job_cut_short(host, T):
    full, job = tf.routes_job(), tf.routes_job(T)
    n = len(job["ids"])
    assert len(job["tracks"][0]) - 1 == T and np.array_equal(job["ids"], full["ids"][:n])
    assert all(np.array_equal(a, b) for a, b in zip(job["kps"], full["kps"][:n]))
    pts, res, _ = tf.routes(host, job)
    fp, fr, _ = tf.routes(host, full)
    assert pts.tobytes() == fp[:T].tobytes() and res.tobytes() == fr[:len(res)].tobytes()


def test_thresholds_met_with_equality(host):
    job = tf.routes_job()
    seen = tf.equality_checks(tf.twin_run(host, job), job)
    print("equality: {track: (threshold, status at it, status one place off)} %s" % seen)
    assert len(seen) == 6 and {63, 64} <= set(seen)


def test_parameters_at_their_limits(host):
    job = tf.routes_job()
    worst = tf.parameter_checks(tf.twin_run(host, job), job, tb.TOL_ANGLE)
    print("parameters: worst |tri_angle - reference angle| %.3g degrees" % worst)


def test_scan_stops_at_the_first_pair(host):
    job = tf.scan_order_job()
    ang = tf.scan_order_check(tf.twin_run(host, job), job, tb.TOL_ANGLE)
    print("scan order: reference angles %s" % {k: round(v, 4) for k, v in ang.items()})
    # the same under a threshold no pair reaches: the largest angle of all pairs, (5, 3)
    pts, _ = tf.twin_run(host, job)((2.0, 91.0, 2))
    assert not int(pts[0]["status"]) & ref.ANGLE_OK and abs(float(pts[0]["tri_angle"]) - max(ang.values())) <= tb.TOL_ANGLE
    assert max(ang, key=ang.get) == (5, 3)


def test_conditioning_jobs(host):
    """The capture's list rebuilds its tracks (a host union over the list's matches); the recorded worst tracks are the 20 farthest
    from the 50-digit solution in every case (mp_case is shared with tests/test_triangulation_reference.py: solved once per run);
    the small-parallax job equals that module's."""
    c, small = tf.conditioning_jobs()
    pairs, offs, qt = c["lst"]
    o, img, idx, _ = c["tracks"]
    assert len(qt) == len(img) - (len(o) - 1) and np.all(pairs[:, 0] < pairs[:, 1]) and offs[-1] == len(qt)
    track_of = {(int(i), int(r)): t for t in range(len(o) - 1) for i, r in zip(img[o[t]:o[t + 1]], idx[o[t]:o[t + 1]])}
    for p, (a, b) in enumerate(pairs):
        for q, t in qt[offs[p]:offs[p + 1]]:
            assert track_of[(int(a), int(q))] == track_of[(int(b), int(t))]
    assert [n for n, _ in c["cases"]] == [m[0] for m in tb.MP_CASES] == list(tf.MP_WORST)
    for name, poses in c["cases"]:
        pts, _, X = tb.mp_case(host, name)
        d = np.abs(pts["X"] - X).max(axis=1)
        assert np.argsort(-d, kind="stable")[:20].tolist() == tf.MP_WORST[name], name
        assert tf.mp_distance(c, poses, pts, tf.MP_WORST[name][0]) == d[tf.MP_WORST[name][0]] <= tb.MP_BOUNDS[name]
    tracks, ids, kps, poses = tb.laid_job(tb.small_parallax_tracks()[0])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(small["tracks"], tracks)) and np.array_equal(small["ids"], ids)
    a = tw.run(host, tracks, ids, kps, poses, tf.CAM, (2.0, 0.0, 2))
    b = tf.twin_run(host, small)((2.0, 0.0, 2))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
