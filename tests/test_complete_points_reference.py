"""The map completion's host twin (csrc/msfm_complete.h, CompletePoints) against the independent numpy reference tests/complete_ref.py,
and the twin's own invariants.  CPU only.

Cases (tests/complete_fixtures.py): (1) the robust session extended in two increments and filtered at (1.0, 2.5), completed with NULL
parameters -- without a scope, scoped to the last increment's images, and scoped to an image that holds no candidate; (2) a plain
session whose next increment is extended under perturbed poses and then repaired by the pose refinement twin: REPOSED
records; (3) the distorted camera with fx != fy, filtered at 6 px under its 40 px session and completed at an explicit 15 px; (4) one
generated group with what those scenes lack.  In every case the reference is fed the twin's state BEFORE the call.

Compared per track: the kind, the candidates, the admitted and the rejected by depth, every inlier byte, the status and n_views
exactly; X bit for bit (it is never written); the residual slots, mean_residual and tri_angle of completed tracks within TOL.  A track is
left out only where the REFERENCE sees an error within GUARD_ERR of a threshold it compared it with (the call's for admission, the
session's for ERROR_OK), or a scanned angle within GUARD_ANGLE of min_angle; with the committed seed, none (smallest margins: DESIGN.md
section 23).

TOL: section 22's bounds as they stand (16 x the worst twin-minus-reference difference measured THERE): the same point_verdict code runs
on the same kind of scene.  The worst differences measured here are in MEASURED and in DESIGN.md section 23."""
import numpy as np
import pytest

import complete_fixtures as cfx
import complete_ref as cr
import complete_twin as ctw
import extend_twin as etw
import filter_fixtures as ffx
import filter_ref as fr
import filter_twin as ftw
from monocularsfm_amd import _lib

GUARD_ERR, GUARD_ANGLE = 1e-6, 1e-6
TOL = dict(residual=2.1e-12, mean_residual=6.7e-13, tri_angle=7.4e-12)
MEASURED = dict(residual=1.2e-13, mean_residual=3.0e-14, tri_angle=5.5e-13)   # the worst over the committed cases (printed by the test)
OK_BITS = 4 | 8
KEEP = _lib.TRI_ROBUST | _lib.TRI_REFINED | _lib.TRI_REPOSED | _lib.TRI_EXTENDED | _lib.TRI_FILTERED


@pytest.fixture(scope="module")
def host():
    return ctw.load_host()


_cache = {}


def case(host, name):
    """-> the state, the twin's result with its trace (`got`) and the reference's (`want`), computed once per module"""
    if name not in _cache:
        c = cfx.CASES[name](host)
        pp, pr, pm = c["before"]
        c["got"] = ctw.run(host, c["tracks"], c["ids"], c["kps"], c["lst"], c["cam"], pp, pr, pm, c["thr"], c["params"], c["scope"], trace=True)
        kd = {int(i): k for i, k in zip(c["ids"], c["kps"])}
        c["want"] = cr.run(c["tracks"], kd, ffx.poses_dict(c["lst"]), c["cam"], pp, pr, pm, c["thr"], c["params"], c["scope"])
        c["name"] = name
        _cache[name] = c
    return _cache[name]


def compare(c):
    """-> (worst differences per quantity, eligible, left out, smallest margins)"""
    pp = c["before"][0]
    pts, res, mask, cnt, tr = c["got"]
    o = c["tracks"][0]
    worst = {k: 0.0 for k in TOL}
    eligible, left, margins = 0, [], dict(error=np.inf, angle=np.inf)
    tally = {k: 0 for k in ctw.COUNT_KEYS}
    for t, w in enumerate(c["want"]):
        b, e = int(o[t]), int(o[t + 1])
        if w["kind"] != cr.NOT_ELIGIBLE:
            eligible += 1
            if w["error_margin"] < GUARD_ERR or w["angle_margin"] < GUARD_ANGLE:
                left.append(t)
                continue
            margins["error"] = min(margins["error"], w["error_margin"])
            margins["angle"] = min(margins["angle"], w["angle_margin"])
            tally["eligible"] += 1
            for k in ("candidates", "admitted", "rejected_by_depth", "rejected_by_error"):
                tally[k] += w[k]
            tally["completed"] += w["kind"] == cr.COMPLETED
        assert tr[t]["kind"] == w["kind"], (c["name"], t, tr[t], w["kind"])
        assert (tr[t]["candidates"], tr[t]["admitted"], tr[t]["rejected_by_depth"]) == (w["candidates"], w["admitted"], w["rejected_by_depth"])
        assert pts[t]["status"] == w["status"] and pts[t]["n_views"] == w["n_views"], (c["name"], t, pts[t], w["status"], w["n_views"])
        assert np.array_equal(mask[b:e], w["mask"]), (c["name"], t, mask[b:e], w["mask"])
        assert pts[t]["X"].tobytes() == pp[t]["X"].tobytes()
        if w["kind"] != cr.COMPLETED:
            continue
        both = np.isnan(res[b:e]) & np.isnan(w["residuals"])           # (a NaN candidate's slot is a NaN on both sides)
        worst["residual"] = max(worst["residual"], float(np.max(np.abs(np.where(both, 0.0, res[b:e] - w["residuals"])))))
        worst["mean_residual"] = max(worst["mean_residual"], abs(float(pts[t]["mean_residual"]) - w["mean_residual"]))
        worst["tri_angle"] = max(worst["tri_angle"], abs(float(pts[t]["tri_angle"]) - w["tri_angle"]))
    if not left:
        assert {k: cnt[k] for k in tally} == {k: int(v) for k, v in tally.items()}, (cnt, tally)
    return worst, eligible, left, margins


def twin_invariants(host, c):
    """what must hold on the twin alone: the consequences of the rule"""
    pp, pr, pm = c["before"]
    pts, res, mask, cnt, tr = c["got"]
    o = c["tracks"][0]
    args = (host, c["tracks"], c["ids"], c["kps"], c["lst"], c["cam"])
    call = c["thr"][0] if c["params"] is None else c["params"]
    assert pm is not None
    per_obs = np.repeat(tr["kind"], np.diff(o))
    same, same_obs = tr["kind"] != ctw.KIND_COMPLETED, per_obs != ctw.KIND_COMPLETED
    # untouched and ineligible tracks identical in record, slots and bytes
    assert pts[same].tobytes() == pp[same].tobytes() and res[same_obs].tobytes() == pr[same_obs].tobytes()
    assert mask[same_obs].tobytes() == pm[same_obs].tobytes()
    done = ~same
    assert np.all(_lib.completed(pts)[done]) and np.array_equal(_lib.completed(pts)[same], _lib.completed(pp)[same])
    assert np.array_equal(pts["status"][done] & KEEP, pp["status"][done] & KEEP) and pts["X"].tobytes() == pp["X"].tobytes()
    # every completed record still stands; the bytes only rise, by exactly `admitted`
    assert np.all((pts["status"][done] & (2 | OK_BITS)) == (2 | OK_BITS))
    assert np.all(mask >= pm) and int(mask.sum()) - int(pm.sum()) == cnt["admitted"] == int(tr["admitted"].sum())
    assert np.array_equal(pts["n_views"][done], pp["n_views"][done] + tr["admitted"][done])
    assert cnt["candidates"] == cnt["admitted"] + cnt["rejected_by_depth"] + cnt["rejected_by_error"]
    assert cnt["succeeded"] == int(_lib.succeeded(pts).sum()) and cnt["observations_used"] == int(pts["n_views"].sum())
    assert cnt["observations_used"] == int(pp["n_views"].sum()) + cnt["admitted"]
    # a second call with the same parameters changes no byte and reports zero admitted and completed
    p2, r2, m2, c2, t2 = ctw.run(*args, pts, res, mask, c["thr"], c["params"], c["scope"], trace=True)
    assert p2.tobytes() == pts.tobytes() and r2.tobytes() == res.tobytes() and m2.tobytes() == mask.tobytes()
    assert c2["admitted"] == 0 and c2["completed"] == 0 and c2["eligible"] == cnt["eligible"]
    assert c2["candidates"] == cnt["candidates"] - cnt["admitted"] and c2["rejected_by_depth"] == cnt["rejected_by_depth"]
    # a filter at the call's max_error, or looser, right after the completion drops none of what was admitted
    gained = (mask != 0) & (pm == 0)
    for e in (call, c["thr"][0]):
        fm = ftw.run(*args, pts, res, mask, c["thr"], (e, 0.0), ())[2]
        assert np.all(fm[gained] == 1), (c["name"], e)
    # bytes made by a no-op ExtendPoints equal those of have_mask = false: on a session without bytes there is no candidate
    # (the case's records and slots WITHOUT its bytes: what a plain session would hold)
    pm0 = etw.run(host, c["tracks"], c["ids"], c["kps"], c["lst"], {}, c["cam"], pp, pr, None, c["thr"])[2]
    a = ctw.run(*args, pp, pr, None, c["thr"], c["params"], c["scope"], trace=True)
    b = ctw.run(*args, pp, pr, pm0, c["thr"], c["params"], c["scope"], trace=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3] + a[4:], b[:3] + b[4:])) and a[3] == b[3]
    assert a[3]["candidates"] == 0 and a[0].tobytes() == pp.tobytes() and a[1].tobytes() == pr.tobytes() and a[2].tobytes() == pm0.tobytes()
    # NULL parameters are the session's value passed explicitly
    x = ctw.run(*args, pp, pr, pm, c["thr"], None, c["scope"])
    y = ctw.run(*args, pp, pr, pm, c["thr"], c["thr"][0], c["scope"])
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x[:3], y[:3])) and x[3] == y[3]


@pytest.mark.parametrize("name", sorted(cfx.CASES))
def test_twin_against_the_reference(host, name):
    c = case(host, name)
    worst, eligible, left, margins = compare(c)
    print("%s: eligible %d, left out %d, margins %s, worst %s, counts %s" % (name, eligible, len(left), margins,
                                                                            {q: "%.3g" % v for q, v in worst.items()}, c["got"][3]))
    assert eligible > 0
    assert not left                                                    # the cap on what may be left out: zero tracks
    for q in TOL:
        assert worst[q] <= TOL[q], (name, q, worst[q], TOL[q])


@pytest.mark.parametrize("name", sorted(cfx.CASES))
def test_twin_invariants(host, name):
    twin_invariants(host, case(host, name))


def test_nothing_the_filter_dropped_comes_back_at_its_own_threshold(host):
    """right after a filter at (e, a) a completion at max_error = e admits none of the observations that filter dropped"""
    for name, e in (("1_filtered_tight_null", cfx.TIGHT_C[0]), ("3_distorted_explicit", cfx.D_FILTER[0])):
        c = case(host, name)
        pp, pr, pm = c["before"]
        got = ctw.run(host, c["tracks"], c["ids"], c["kps"], c["lst"], c["cam"], pp, pr, pm, c["thr"], e, ())
        assert got[3]["candidates"] > 0 and got[3]["admitted"] == 0 and got[2].tobytes() == pm.tobytes() and got[0].tobytes() == pp.tobytes()
    g = ffx.case_group(host)                                           # the filter's own group, filtered at (2.0, 1.5): drops by depth as well
    pp, pr, pm = g["before"]
    args = (host, g["tracks"], g["ids"], g["kps"], g["lst"], g["cam"])
    fp, fres, fm, fc = ftw.run(*args, pp, pr, pm, g["thr"], g["params"], ())
    assert fc["dropped_by_depth"] > 0 and fc["dropped_by_error"] > 0
    got = ctw.run(*args, fp, fres, fm, g["thr"], g["params"][0], ())
    assert got[3]["admitted"] == 0 and got[3]["rejected_by_depth"] > 0 and got[2].tobytes() == fm.tobytes()


def test_the_cases_reach_every_kind(host):
    """every Trace kind and every counter is non-zero somewhere, and the generated group does what it was built for"""
    kinds, counts = set(), {k: 0 for k in ctw.ALL_KEYS}
    for name in cfx.CASES:
        c = case(host, name)
        kinds |= set(int(k) for k in c["got"][4]["kind"])
        for k in counts:
            counts[k] += c["got"][3][k]
    assert kinds == {0, 1, 2} and all(v > 0 for v in counts.values()), (kinds, counts)
    one, last, none = (case(host, n) for n in sorted(cfx.CASES)[:3])
    assert _lib.filtered(one["before"][0]).any() and _lib.extended(one["before"][0]).any() and (one["before"][0]["status"] & _lib.TRI_ROBUST).any()
    assert 0 < last["got"][3]["candidates"] < one["got"][3]["candidates"] and 0 < last["got"][3]["admitted"] < one["got"][3]["admitted"]
    assert none["got"][3]["candidates"] == 0 and none["got"][0].tobytes() == none["before"][0].tobytes()
    two = case(host, "2_extended_reposed")
    assert two["extend_counts"]["observations_rejected"] > 20 and two["extend_counts"]["observations_added"] > 20
    assert two["pose_counts"]["refined"] == 2 and two["got"][3]["admitted"] > 20
    done = two["got"][4]["kind"] == ctw.KIND_COMPLETED
    want = _lib.TRI_REPOSED | _lib.TRI_COMPLETED
    # (the pose refinement's re-verdict drops EXTENDED from every record it visits: the records are REPOSED, the extension's work is
    # in their bytes)
    assert np.all((two["got"][0]["status"][done] & want) == want) and _lib.extended(two["before"][0]).sum() == 0
    three = case(host, "3_distorted_explicit")
    assert three["cam"][0] != three["cam"][1] and cfx.D_FILTER[0] < three["params"] < three["thr"][0] and three["got"][3]["rejected_by_error"] > 0
    g = case(host, "4_group")
    pp = g["before"][0]
    pts, res, mask, cnt, tr = g["got"]
    o, img = g["tracks"][0], g["tracks"][1]
    K = ctw
    assert tr["kind"].tolist() == [K.KIND_UNTOUCHED] * 6 + [K.KIND_COMPLETED] * 6 + [K.KIND_NOT_ELIGIBLE] * 3 + [K.KIND_COMPLETED] * 2 + \
        [K.KIND_UNTOUCHED] * 3
    assert tr["candidates"].tolist() == [1] * 6 + [2, 2] + [1] * 4 + [0] * 3 + [1, 1] + [0] * 3
    assert tr["admitted"].tolist() == [0] * 6 + [1] * 6 + [0] * 3 + [1, 1] + [0] * 3
    assert tr["rejected_by_depth"].tolist() == [1, 1] + [0] * 18                           # the turned camera
    assert cnt["rejected_by_error"] == 6                                                 # 30 px off (2, 3, 6, 7) and the NaNs (4, 5)
    for t in (4, 5):                                                                     # the NaN candidate: rejected, nothing written
        k = int(o[t]) + 3
        assert np.isnan(g["kps"][3][t, :2]).any() and mask[k] == 0 and res[k] == g["before"][1][k]
    for t in (6, 7):                                                                     # both outcomes in one track
        b = int(o[t])
        assert mask[b:int(o[t + 1])].tolist() == [1, 1, 1, 1, 0, 1] and res[b + 4] > 20.0
    # the admitted observation changes which pair ends the parallax scan (8, 9: the scan ended at (3, 1), now at (2, 0)) or not (10, 11)
    assert np.all(pts["tri_angle"][[8, 9]] != pp["tri_angle"][[8, 9]]) and pts["tri_angle"][[10, 11]].tobytes() == pp["tri_angle"][[10, 11]].tobytes()
    poses = ffx.poses_dict(g["lst"])
    for t, before, after in ((8, (1, 2, 3), (0, 1, 2, 3)), (10, (0, 2, 3), (0, 1, 2, 3))):
        cen = {p: -(np.asarray(poses[int(g["ids"][p])][0]).T @ np.asarray(poses[int(g["ids"][p])][1])).astype(np.longdouble) for p in after}
        X = pp[t]["X"].astype(np.longdouble)
        a0, a1 = fr.scan(X, cen, list(before), 1.5)[1], fr.scan(X, cen, list(after), 1.5)[1]
        assert abs(float(a0) - pp[t]["tri_angle"]) < 1e-9 and abs(float(a1) - pts[t]["tri_angle"]) < 1e-9 and (a0 != a1) == (t == 8)
    # a track that does not stand with a candidate that would fit: bit for bit
    for t in (12, 13):
        b = int(o[t])
        assert (pp["status"][t] & 14) == 6 and mask[b + 2] == 0 and g["want"][t]["kind"] == cr.NOT_ELIGIBLE
        assert pts[t].tobytes() == pp[t].tobytes()
        forced = pp.copy()
        forced["status"][t] |= 8
        would = ctw.run(host, g["tracks"], g["ids"], g["kps"], g["lst"], g["cam"], forced, g["before"][1], g["before"][2], g["thr"], None, (),
                        select=[t], trace=True)[4]
        assert would[t]["admitted"] == 1                                                 # (it WOULD fit, were the track eligible)
    assert g["tracks"][3][cfx.GROUP_INCONSISTENT] == 0 and pts[14].tobytes() == pp[14].tobytes()
    for t in (15, 16):                                                                   # next to an element in an unposed image
        b = int(o[t])
        assert int(img[b + 4]) == int(g["ids"][cfx.GROUP_UNPOSED]) and res[b + 4] == -1.0 and mask[b:b + 5].tolist() == [1, 1, 1, 1, 0]


def test_scope_and_parameters(host):
    """an empty list is every image; a listed image without a valid pose selects nothing; the order of the list reaches nothing; a
    threshold above the session's is refused by the twin's export"""
    c = case(host, "1_filtered_tight_null_last_increment")
    full = case(host, "1_filtered_tight_null")
    pp, pr, pm = c["before"]
    args = (host, c["tracks"], c["ids"], c["kps"], c["lst"], c["cam"], pp, pr, pm, c["thr"])
    empty = ctw.run(*args, None, ())
    assert all(a.tobytes() == b.tobytes() for a, b in zip(empty[:3], full["got"][:3])) and empty[3] == full["got"][3]
    rev = ctw.run(*args, None, tuple(reversed(c["scope"])))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rev[:3], c["got"][:3])) and rev[3] == c["got"][3]
    # only candidates IN a listed image: the bytes that rose all lie in the scope
    rose = (c["got"][2] != 0) & (pm == 0)
    assert rose.any() and np.isin(c["tracks"][1][rose], c["scope"]).all()
    ids, poses = c["ids"], ffx.poses_dict(c["lst"])
    early = {int(ids[p]): poses[int(ids[p])] for p in cfx.efx.FIRST + cfx.efx.TWO[0]}
    unposed = [int(i) for i in ids if int(i) not in early]
    none = ctw.run(host, c["tracks"], ids, c["kps"], early, c["cam"], pp, pr, pm, c["thr"], None, unposed[:2])
    assert none[3]["candidates"] == 0 and none[0].tobytes() == pp.tobytes() and none[2].tobytes() == pm.tobytes()
    with pytest.raises(AssertionError):
        ctw.run(*args, np.nextafter(c["thr"][0], np.inf), ())                           # host_complete_points returns 3
