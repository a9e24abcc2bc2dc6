"""Non-finite and huge keypoint coordinates through the host twins of the reconstruction and verification stages (DESIGN.md section
21).  CPU only.  msfm_upload_keypoints validates nothing, so a NaN (plain, signed, with a payload), +-inf, +-3e38, 1e30, the smallest
denormal and -0.0 reach every function that reads a keypoint; the shared headers promise that "a NaN fails" every test it takes part
in.  These tests hold the twins -- and through the byte comparisons of tests/test_gpu_nonfinite.py the kernels -- to that, for every
entry of nonfinite_fixtures.CASES, under CAM and the distorted CAM_D, on the placements of tests/nonfinite_fixtures.py.  That every
case returns at all is the proof that no shared loop needs a finite value to end.

WHICH PLACEMENT IS COMPARED WHICH WAY
  first form    GROSS-OUTLIER EQUIVALENCE: the chain on the scene equals, byte for byte, the chain on the twin scene whose bad coordinates
                are 1e6 -- records, inlier bytes, pose lists, registration and pose-refinement records, every counter and every residual
                slot outside the bad mask.  Every track whose record comes from a consensus or from a continuation: every track of the
                robust session; the tracks the extension creates with max_hypotheses 8 (robust or plain session); every clean track
                anywhere.
  second form   a PLAIN track whose DLT takes the bad observation in: the bad tracks of the plain triangulation and of the point
                refinement that follows it (plain session), and the bad 3-view tracks that the extension creates with max_hypotheses 0
                (either session).  The DLT over a NaN is not the DLT over 1e6, so there the documented result is asserted instead:
                ATTEMPTED and never ERROR_OK (so the track supports nothing downstream); for a non-finite value ATTEMPTED alone, every
                other field 0, every slot -1, n_views = the posed elements (msfm_triangulate.h, "DLT").  The counters and cost sums of
                a step that has such tracks follow them (eligible, iterations, points_reposed, the costs) and are not compared there.
The 1e6 scene itself is anchored: test_the_gross_scene_against_the_references holds its twins to the independent numpy references
with those modules' own comparisons, margins and tolerances.

THE FILTER (msfm_filter_points' twin, FilterPoints) runs at the end of the chain under the three pairs of nf.FILTER_PAIRS, each from the
state after the last point refinement -- under the session's own thresholds it drops nothing there and would only walk its no-op path
-- and, on the plain session, behind the first point refinement under the session's thresholds, where it creates the inlier bytes
(compare_filter, test_the_plain_session_filter).  A trimmed track goes through point_verdict in its `residuals != nullptr` mode, which
rewrites the slot of every USED observation, the bad ones included: one more store of a NaN.

THE COMPLETION (msfm_complete_points' twin, CompletePoints) runs as a side step of the chain behind the filter under FILTER_MIX and
FILTER_TRIM, and on the PLANTED route (nf.complete_planted): there one clean observation of every third track and of every bad
8-view track is moved by 40 px, dropped by the filter under the session's thresholds and found again under the original keypoints.
Every bad observation in a posed image has byte 0 and is USED: it is a candidate of every completion call, and it must be rejected
by its error -- `!(err <= max_error)`, the one comparison a NaN passes through -- never by depth, which reads X and the pose alone
(compare_complete, test_the_cure, test_completion_call_parameters)."""
import numpy as np
import pytest

import complete_twin as ctw
import extend_twin as etw
import filter_twin as ftw
import nonfinite_fixtures as nf
import refine_poses_twin as ptw
import triangulation_twin as tw
from monocularsfm_amd import _lib

CANONICAL = 0x7ff8000000000000
PLACEMENTS = {"lanes": nf.lanes, "wave": nf.whole_wave, "images": nf.images}
CAMS = {"cam": nf.CAM, "cam_d": nf.CAM_D}
STEPS = ("plain", "robust", "refine1", "register", "extend", "poses", "refine2")


@pytest.fixture(scope="module")
def host():
    return nf.load_host()


_GROSS = {}


def gross_chain(host, place, case, cam, mh, robust):
    """the chain on the twin scene: the same for every value that sits in the same coordinates"""
    key = (place, case[2], cam, mh, robust)
    if key not in _GROSS:
        _GROSS[key] = nf.chain(host, PLACEMENTS[place](case)[2], CAMS[cam], mh=mh, robust=robust)
    return _GROSS[key]


def posed_after(step, sc):
    """the image positions that have a pose when `step` has run"""
    return set(nf.OLD) | (set(nf.NEW) | {nf.REG} if step in ("extend", "poses", "refine2") else set())


def loose_tracks(step, sc, out, mh, robust):
    """the second form's tracks at `step` (module docstring): bad tracks whose record is a plain DLT over a bad observation"""
    o = sc.tracks[0]
    bad_posed = np.asarray([any(sc.bad[o[t] + k] for k in range(n) if k in posed_after(step, sc)) for t, n in enumerate(sc.lengths)])
    if step in ("plain",) or (not robust and step in ("refine1",)):
        return bad_posed
    if step in ("extend", "poses", "refine2") and mh == 0:
        return bad_posed & (out["extend"][5]["kind"] == etw.KIND_CREATE)
    return np.zeros(len(sc.lengths), bool)


def arrays_of(step, o):
    """(records per track, residuals per slot, bytes per slot or None, everything else that must be byte-equal, counters) of a step"""
    if o is None:
        return None
    if step == "plain":
        return o[0], o[1], None, [], None
    if step == "robust":
        return o[0], o[1], o[2], [], o[3]
    if step in ("refine1", "refine2"):
        return o[0], o[1], None, [], o[2]
    if step == "extend":
        return o[0], o[1], o[2], list(o[4]), o[3]
    if step == "poses":
        return o[0], o[1], None, list(o[2]) + [o[3]], o[4]
    raise AssertionError(step)


def nan_bits(a):
    a = np.ascontiguousarray(a, np.float64)
    return set(int(v) for v in a.view(np.uint64)[np.isnan(a)])


def float_fields_finite(rec):
    for name in rec.dtype.names:
        if rec.dtype[name].base.kind == "f":
            assert np.all(np.isfinite(rec[name])), name


def same_number(a, b):
    return a == b or (a != a and b != b)


def compare(sc, case, a, b, mh, robust, canonical=True):
    """the chain outputs `a` (the scene) against `b` (the twin scene): the first form wherever it applies, the second form elsewhere;
    every float field of every record finite; NaNs only inside the bad mask and, with `canonical`, only THE NaN"""
    o = sc.tracks[0]
    per_slot = np.repeat(np.arange(len(sc.lengths)), np.diff(o))
    for step in STEPS:
        if a.get(step) is None:
            assert b.get(step) is None
            continue
        if step == "register":
            ra, rb = a[step], b[step]
            badc = nf.registration_bad(sc, ra)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(ra[:4], rb[:4])), (case[0], step)     # records, offsets, track ids, flags
            assert ra[4][~badc].tobytes() == rb[4][~badc].tobytes() and not np.isnan(ra[4][~badc]).any(), (case[0], step)
            assert not ra[3][badc].any()                                  # a bad correspondence is never an inlier
            float_fields_finite(ra[0])
            if canonical:
                assert nan_bits(ra[4]) <= {CANONICAL}, (case[0], step, [hex(v) for v in nan_bits(ra[4])])
            continue
        pa, sa, ma, xa, ca = arrays_of(step, a[step])
        pb, sb, mb, xb, cb = arrays_of(step, b[step])
        loose = loose_tracks(step, sc, a, mh, robust)
        tight = ~loose
        slot_ok = tight[per_slot] & ~sc.bad
        assert pa[tight].tobytes() == pb[tight].tobytes(), (case[0], step, np.nonzero(pa != pb)[0][:8])
        assert sa[slot_ok].tobytes() == sb[slot_ok].tobytes(), (case[0], step)
        if ma is not None:
            assert ma[tight[per_slot]].tobytes() == mb[tight[per_slot]].tobytes(), (case[0], step)
            assert not ma[sc.bad & tight[per_slot]].any(), (case[0], step)     # a bad observation never supports a consensus point
        assert all(x.tobytes() == y.tobytes() for x, y in zip(xa, xb)), (case[0], step)
        if ca is not None and not loose.any():
            assert all(same_number(ca[k], cb[k]) for k in ca), (case[0], step, ca, cb)
            # which cost sums are finite (tests/test_gpu_nonfinite.py asserts the same of the device): all of them where no track is
            # of the second form
            assert all(np.isfinite(ca[k]) for k in ca if k.startswith("cost_")), (case[0], step, ca)
        elif ca is not None and (nf.non_finite(case) or case[0].startswith(("denormal", "minus_zero"))):
            # ... and where the second-form tracks have no point (a non-finite value) or an error that does not overflow (0 px)
            assert all(np.isfinite(ca[k]) for k in ca if k.startswith("cost_")), (case[0], step, ca)
        # the second form
        for t in np.nonzero(loose)[0]:
            s = int(pa[t]["status"])
            assert s & _lib.TRI_ATTEMPTED and not s & _lib.TRI_ERROR_OK, (case[0], step, t, s)
            if nf.non_finite(case):
                posed = sum(1 for k in range(sc.lengths[t]) if k in posed_after(step, sc))
                assert (s & ~_lib.TRI_EXTENDED) == _lib.TRI_ATTEMPTED and pa[t]["n_views"] == posed, (case[0], step, t, pa[t])
                assert pa[t].tobytes()[8:] == bytes(40) and np.all(sa[o[t]:o[t + 1]] == -1.0), (case[0], step, t, pa[t])
        # finiteness and THE NaN (a second-form track under 3e38 or 1e30 has a finite X whose errors overflow: mean_residual = +inf)
        float_fields_finite(pa[tight])
        assert not any(np.isnan(pa[n]).any() for n in ("X", "mean_residual", "tri_angle")), (case[0], step)
        for x in xa:
            if x.dtype.names:
                float_fields_finite(x)
        assert not np.isnan(sa[~sc.bad]).any(), (case[0], step)
        if canonical:
            assert nan_bits(sa) <= {CANONICAL}, (case[0], step, [hex(v) for v in nan_bits(sa)])


def compare_filter(host, sc, case, cam, a, b, mh, robust, routes=True, mix_trims_bad=True):
    """The filter steps at the end of the chain outputs `a` (the scene) against those of `b` (the twin scene), under every pair of
    nf.FILTER_PAIRS.  FIRST FORM on every track but the second-form tracks of the last point refinement: records, inlier bytes, the
    twin's trace and every residual slot but the bad observations' own byte for byte, the counters where no track is of the second
    form; no inlier byte on a bad observation.  THE EXCEPTION in its own form: a second-form track (created on the plain route with
    max_hypotheses 0) under a non-finite value is ATTEMPTED alone, so not eligible: record, slots and bytes stay bit for bit, the
    bytes 1 on every element, the bad one included (the extension made them so); under a finite value it either has no point as well
    and stays the same way, or has a point without ERROR_OK, is eligible and is trimmed or removed.  Everywhere: every float field of every record finite after the call, NaNs only in the bad
    slots and only THE NaN, a second call that changes no byte and counts nothing.  With `routes`, on the robust session, the twin's
    trace shows that the pair did what it is for (a pair that quietly reaches nothing proves nothing)."""
    o = sc.tracks[0]
    per_slot = np.repeat(np.arange(len(sc.lengths)), np.diff(o))
    loose = loose_tracks("refine2", sc, a, mh, robust)
    tight, tight_slot = ~loose, ~loose[per_slot]
    badt = np.zeros(len(sc.lengths), bool)
    badt[sc.bad_tracks()] = True
    p0, r0, m0, lst = a["refine2"][0], a["refine2"][1], a["extend"][2], a["poses"][2]
    quiet = [k for k in ftw.ALL_KEYS if k not in ("eligible", "succeeded", "observations_used")]
    for name, pair in nf.FILTER_PAIRS:
        what = (case[0], name, mh, robust)
        pa, sa, ma, ca, ta = a["filter"][name]
        pb, sb, mb, cb, tb = b["filter"][name]
        assert pa[tight].tobytes() == pb[tight].tobytes(), (what, np.nonzero(pa != pb)[0][:8])
        assert sa[tight_slot & ~sc.bad].tobytes() == sb[tight_slot & ~sc.bad].tobytes(), what
        assert ma[tight_slot].tobytes() == mb[tight_slot].tobytes() and ta[tight].tobytes() == tb[tight].tobytes(), what
        assert not ma[sc.bad & tight_slot].any(), what
        if not loose.any():
            assert ca == cb, (what, ca, cb)
        for t in np.nonzero(loose)[0]:
            sl = slice(int(o[t]), int(o[t + 1]))
            has_point = bool(int(p0[t]["status"]) & _lib.TRI_POINT)
            if nf.non_finite(case):
                assert not has_point and (int(p0[t]["status"]) & ~_lib.TRI_EXTENDED) == _lib.TRI_ATTEMPTED, (what, t, p0[t])
                assert ma[sl].all() and sc.bad[sl].any(), (what, t, ma[sl])
            if has_point:       # (it lacks ERROR_OK under the session's 2 px: one fitting observation at least fails every pair's max_error)
                assert ta[t]["kind"] >= ftw.KIND_TRIMMED, (what, t, ta[t])
            else:               # (a DLT over 3e38 may end without a point as well)
                assert ta[t]["kind"] == ftw.KIND_NOT_ELIGIBLE, (what, t, ta[t])
                assert pa[t].tobytes() == p0[t].tobytes() and sa[sl].tobytes() == r0[sl].tobytes() and ma[sl].tobytes() == m0[sl].tobytes(), (what, t)
        float_fields_finite(pa)
        assert not np.isnan(sa[~sc.bad]).any() and nan_bits(sa) <= {CANONICAL}, (what, [hex(v) for v in nan_bits(sa)])
        again = ftw.run(host, sc.tracks, sc.ids, sc.kps, lst, cam, pa, sa, ma, nf.THR[:2], pair)
        assert again[0].tobytes() == pa.tobytes() and again[1].tobytes() == sa.tobytes() and again[2].tobytes() == ma.tobytes(), what
        assert all(again[3][k] == 0 for k in quiet) and all(again[3][k] == ca[k] for k in ("succeeded", "observations_used")), (what, again[3])
        if not (routes and robust):
            continue
        kind = ta["kind"]
        drops = int((ta["dropped_by_depth"] + ta["dropped_by_error"])[tight].sum())
        if name in ("mix", "trim"):
            # a bad track is trimmed (its bad slots are rewritten: under a NaN, THE NaN stands in every one of them afterwards) and
            # a clean one is untouched.  `mix_trims_bad` False: the lane placement under CAM, whose five bad tracks FILTER_MIX leaves
            # untouched or removes by views (nonfinite_fixtures.FILTER_TRIM) -- there FILTER_TRIM alone reaches the route
            trimmed_bad = badt & tight & (kind == ftw.KIND_TRIMMED)
            assert (kind[~badt] == ftw.KIND_UNTOUCHED).any() and (kind == ftw.KIND_TRIMMED).any(), (what, np.bincount(kind, minlength=5))
            assert trimmed_bad.any() or (name == "mix" and not mix_trims_bad), (what, ta[badt])
            if case[0].startswith("nan"):
                assert np.isnan(sa[sc.bad & trimmed_bad[per_slot]]).all(), what
        elif name == "angle":
            assert ca["removed_by_angle"] > 0 and drops == 0, (what, ca)
        else:
            assert ca["removed_by_views"] > 0 and drops > 0, (what, ca)


# ---- the completion ---------------------------------------------------------------------------------------------------------------------------
def completion_steps(out):
    """(name, the state before the call, first, again) of every completion step of nf.chain's outputs"""
    steps = [(name, out["filter"][name][:3]) + tuple(out["complete"][name]) for name in nf.COMPLETE_BEHIND]
    pl = out["complete_planted"]
    return steps + [("planted", pl["filter"][:3], pl["first"], pl["again"])]


def compare_complete(host, sc, gr, case, cam, a, b, mh, robust, routes=True):
    """The completion steps of the chain outputs `a` (the scene) against those of `b` (the twin scene `gr`): behind FILTER_MIX, behind
    FILTER_TRIM and on the planted route, each call and its repetition.
      equivalence   FIRST FORM on every track but the second-form tracks of the last point refinement (compare_filter): records,
                    inlier bytes, traces and every residual slot but the bad observations' own byte for byte; the six counters and
                    the two sums where no track is of the second form; the planted route's filter step the same way.
      rejection     no bad observation gets byte 1; every bad observation of an eligible track is a candidate and is rejected by its
                    error: the track's rejections by depth are 0 and its rejections by error at least its bad observations;
                    rejected_by_depth equals the twin scene's (0 on every fixture here).
      untouched     a track that is not COMPLETED -- untouched or not eligible -- is bit for bit what it was, its bad slots included,
                    and at least one UNTOUCHED track has a bad candidate: on the planted route a standing bad track outside the
                    planting (the 3-view tracks of the images placement), elsewhere behind the filter.
      completed     a completed bad track: every bad slot holds what nf.bad_slot_class says and nothing else; n_views = the bytes,
                    none of them on a bad observation; every float field of every record finite.  (These three per call:
                    nf.completion_routes, which tests/test_gpu_nonfinite.py applies to the device's calls.)
      routes        on the planted route EVERY standing bad 8-view track is completed, with a rejected bad candidate beside the
                    admitted one, and on the robust session all of them stand; behind the filter at least one of the two pairs
                    completes a bad track.
      fixed point   the second call admits nothing and changes no byte, NaN slots included (bytes compared, not values).
      scope         one call from the planted route's filtered state with the list {REG}: the candidates are the byte-0 elements in
                    image 7 of the eligible tracks, fewer than without a list, the bad ones among them rejected; equal to the twin
                    scene's call."""
    o = sc.tracks[0]
    T = len(sc.lengths)
    per_slot = np.repeat(np.arange(T), np.diff(o))
    loose = loose_tracks("refine2", sc, a, mh, robust)
    tight, tight_slot = ~loose, ~loose[per_slot]
    badt = np.zeros(T, bool)
    badt[sc.bad_tracks()] = True
    lst = a["poses"][2]
    posed = np.isin(sc.tracks[1], [i for i, p in ptw.poses_dict(*lst).items() if p is not None])
    fa, fb = a["complete_planted"]["filter"], b["complete_planted"]["filter"]
    assert fa[0][tight].tobytes() == fb[0][tight].tobytes() and fa[2][tight_slot].tobytes() == fb[2][tight_slot].tobytes(), case[0]
    assert fa[4][tight].tobytes() == fb[4][tight].tobytes() and (loose.any() or fa[3] == fb[3]), (case[0], fa[3], fb[3])
    where = np.zeros(T, bool)
    where[a["complete_planted"]["where"]] = True
    moved = where & tight & (fa[4]["kind"] != ftw.KIND_NOT_ELIGIBLE)      # (the filter dropped the moved observation of every track it read)
    assert np.all(fa[4]["dropped_by_error"][moved] >= 1) and not fa[2][o[:-1][moved] + nf.PLANT_AT].any(), case[0]
    completed_bad, untouched_bad = {}, {}
    for (name, before, first, again), (_, _, gfirst, gagain) in zip(completion_steps(a), completion_steps(b)):
        what = (case[0], name, mh, robust)
        p0, r0, m0 = before
        for (pa, sa, ma, ca, ta), (pb, sb, mb, cb, tb) in ((first, gfirst), (again, gagain)):
            assert not ma[sc.bad & tight_slot].any(), (what, np.nonzero(ma.astype(bool) & sc.bad & tight_slot)[0][:8])
            assert pa[tight].tobytes() == pb[tight].tobytes(), (what, np.nonzero(pa != pb)[0][:8])
            assert sa[tight_slot & ~sc.bad].tobytes() == sb[tight_slot & ~sc.bad].tobytes(), what
            assert ma[tight_slot].tobytes() == mb[tight_slot].tobytes() and ta[tight].tobytes() == tb[tight].tobytes(), what
            assert ca["rejected_by_depth"] == cb["rejected_by_depth"] == 0, (what, ca, cb)
            if not loose.any():
                assert ca == cb, (what, ca, cb)
            float_fields_finite(pa)
            assert not np.isnan(sa[~sc.bad]).any() and nan_bits(sa) <= {CANONICAL}, (what, [hex(v) for v in nan_bits(sa)])
        pa, sa, ma, ca, ta = first
        completed_bad[name], untouched_bad[name] = nf.completion_routes(sc, case, CAMS[cam], posed, before, first, tight, what)
        # the fixed point
        pb, sb, mb, cb, tb = again
        assert pb.tobytes() == pa.tobytes() and sb.tobytes() == sa.tobytes() and mb.tobytes() == ma.tobytes(), what
        assert cb["admitted"] == cb["completed"] == 0 and cb["candidates"] == ca["candidates"] - ca["admitted"], (what, ca, cb)
        assert all(cb[k] == ca[k] for k in ("eligible", "succeeded", "observations_used", "rejected_by_depth")), (what, ca, cb)
    # one scoped call: the candidates in REG alone
    reg = int(sc.ids[nf.REG]) if nf.REG < len(sc.ids) else -1
    if posed[sc.tracks[1] == reg].any():
        state = fa[:3]
        full = a["complete_planted"]["first"]
        got, _ = nf.completed_twice(host, sc, sc.kps, lst, CAMS[cam], state, scope=[reg])
        want, _ = nf.completed_twice(host, gr, gr.kps, b["poses"][2], CAMS[cam], fb[:3], scope=[reg])
        eligible = full[4]["kind"] != ctw.KIND_NOT_ELIGIBLE
        in_reg = (sc.tracks[1] == reg) & (state[2] == 0) & eligible[per_slot]
        assert got[3]["candidates"] == int(in_reg.sum()) < full[3]["candidates"], (case[0], got[3], full[3])
        assert np.array_equal(got[4]["candidates"], np.add.reduceat(in_reg.astype(np.int64), o[:-1])), case[0]
        rose = (got[2] != 0) & (state[2] == 0)
        assert np.all(sc.tracks[1][rose] == reg) and not got[2][sc.bad & tight_slot].any(), case[0]
        assert got[3]["rejected_by_error"] >= int((in_reg & sc.bad).sum()) and got[3]["rejected_by_depth"] == 0, (case[0], got[3])
        assert got[0][tight].tobytes() == want[0][tight].tobytes() and got[2][tight_slot].tobytes() == want[2][tight_slot].tobytes(), case[0]
        assert got[4][tight].tobytes() == want[4][tight].tobytes() and (loose.any() or got[3] == want[3]), (case[0], got[3], want[3])
        assert got[1][tight_slot & ~sc.bad].tobytes() == want[1][tight_slot & ~sc.bad].tobytes() and nan_bits(got[1]) <= {CANONICAL}, case[0]
    if not routes or not (badt & tight).any():
        return None
    # the routes
    stands = _lib.succeeded(fa[0]) & (sc.tracks[3] != 0)
    long_bad = badt & tight & (np.asarray(sc.lengths) == 8)
    assert where[long_bad].all() and (stands & long_bad).any(), (case[0], mh, robust)
    assert not robust or stands[long_bad].all(), (case[0], mh, np.nonzero(long_bad & ~stands)[0])
    assert np.array_equal(completed_bad["planted"][long_bad], stands[long_bad]), (case[0], mh, robust)   # EVERY standing one
    assert completed_bad["mix"].any() or completed_bad["trim"].any(), (case[0], mh, robust)
    outside = badt & tight & ~where & stands
    if outside.any():
        assert untouched_bad["planted"][outside].all(), (case[0], mh, robust, np.nonzero(outside & ~untouched_bad["planted"])[0])
    else:
        assert untouched_bad["mix"].any() or untouched_bad["trim"].any(), (case[0], mh, robust)
    return {k: int(v.sum()) for k, v in completed_bad.items()}, {k: int(v.sum()) for k, v in untouched_bad.items()}


@pytest.mark.parametrize("case", nf.CASES, ids=nf.CASE_IDS)
@pytest.mark.parametrize("cam", sorted(CAMS))
@pytest.mark.parametrize("place", sorted(PLACEMENTS))
def test_the_chain_equals_the_gross_outlier_scene(host, place, cam, case):
    """robust and plain session, the extension with max_hypotheses 8 and 0: the module docstring says what is compared which way; then
    the filter steps at the end of every one of these chains (compare_filter) and the completion steps beside them (compare_complete)"""
    sc, _, gr = PLACEMENTS[place](case)
    for robust in (True, False):
        for mh in (8, 0):
            a = nf.chain(host, sc, CAMS[cam], mh=mh, robust=robust)
            compare(sc, case, a, gross_chain(host, place, case, cam, mh, robust), mh, robust)
            compare_filter(host, sc, case, CAMS[cam], a, gross_chain(host, place, case, cam, mh, robust), mh, robust,
                           mix_trims_bad=(place, cam) != ("lanes", "cam"))
            reached = compare_complete(host, sc, gr, case, cam, a, gross_chain(host, place, case, cam, mh, robust), mh, robust)
            print(place, cam, case[0], "robust" if robust else "plain", mh, "bad tracks completed, untouched with a bad candidate:", reached)


@pytest.mark.parametrize("case", nf.CASES, ids=nf.CASE_IDS)
@pytest.mark.parametrize("cam", sorted(CAMS))
@pytest.mark.parametrize("place", sorted(PLACEMENTS))
def test_the_cure(host, place, cam, case):
    """A bad keypoint that is later replaced by a good one: from the state behind the planted route's completion the TRUE keypoints
    are uploaded in place of the bad ones (the clean scene of the same seed) and the completion runs again, on the robust and on the
    plain session (max_hypotheses 8).  What must be admitted comes from tests/complete_ref.py on the cured scene, not from the twin:
    every formerly bad observation of a standing track whose depth is positive and whose error under the current pose is within
    max_error -- no such error lies within 1e-6 px of the threshold, the reference module's guard.  The twin's bytes, kinds and view
    counts equal the reference's on every bad track; an admitted observation's slot goes from a number that fails `<= max_error` (a
    NaN under a NaN) to a finite one within it; a completed track holds no NaN any more, and NaNs stand only in the bad slots of the
    tracks that were not completed; every clean track is untouched."""
    import complete_ref as cr
    import test_complete_points_reference as xc
    sc = PLACEMENTS[place](case)[0]
    clean = PLACEMENTS[place](None)[0]
    o, img, idx, cons = sc.tracks[:4]
    kd = clean.kd()
    badt = sc.bad_tracks()
    for robust in (True, False):
        a = nf.chain(host, sc, CAMS[cam], mh=8, robust=robust)
        lst = a["poses"][2]
        poses = ptw.poses_dict(*lst)
        p0, r0, m0 = a["complete_planted"]["first"][:3]
        pts, res, mask, cnt, tr = ctw.run(host, sc.tracks, sc.ids, clean.kps, lst, CAMS[cam], p0, r0, m0, nf.THR[:2], trace=True)
        cured = 0
        for t in badt:
            b, e = int(o[t]), int(o[t + 1])
            w = cr.track(img[b:e], idx[b:e], bool(cons[t]), kd, poses, CAMS[cam], p0[t], r0[b:e], m0[b:e], nf.THR[:2], nf.THR[0])
            what = (case[0], robust, int(t), tr[t], w["kind"], w["mask"])
            assert w["error_margin"] > xc.GUARD_ERR and w["angle_margin"] > xc.GUARD_ANGLE, what
            assert tr[t]["kind"] == w["kind"] and np.array_equal(mask[b:e], w["mask"]), what
            assert (tr[t]["candidates"], tr[t]["admitted"], tr[t]["rejected_by_depth"]) == (w["candidates"], w["admitted"], w["rejected_by_depth"]), what
            assert pts[t]["status"] == w["status"] and pts[t]["n_views"] == w["n_views"], what
            if w["kind"] != cr.NOT_ELIGIBLE:
                assert w["candidates"] >= sc.bad[b:e].sum() and w["rejected_by_depth"] == 0, what   # every formerly bad observation is tested
            for k in np.nonzero(sc.bad[b:e] & (w["mask"] != 0))[0]:
                assert m0[b + k] == 0 and not r0[b + k] <= nf.THR[0] and np.isnan(r0[b + k]) == (nf.bad_slot_class(case, CAMS[cam]) == "nan"), (what, r0[b + k])
                assert np.isfinite(res[b + k]) and 0.0 <= res[b + k] <= nf.THR[0], (what, res[b + k])
                assert abs(res[b + k] - w["residuals"][k]) <= xc.TOL["residual"], (what, res[b + k], w["residuals"][k])
                cured += 1
            if w["kind"] == cr.COMPLETED:
                assert not np.isnan(res[b:e]).any(), what
        done = np.repeat(tr["kind"] == ctw.KIND_COMPLETED, np.diff(o))
        assert not np.isnan(res[~sc.bad | done]).any() and nan_bits(res) <= {CANONICAL}, case[0]
        rest = np.setdiff1d(np.arange(len(sc.lengths)), badt)
        assert np.all(tr["kind"][rest] != ctw.KIND_COMPLETED) and pts[rest].tobytes() == p0[rest].tobytes(), case[0]
        assert cured == cnt["admitted"] and cured >= len(badt), (case[0], robust, cured, cnt)      # (more than one per bad track)
        float_fields_finite(pts)
        print(place, cam, case[0], "robust" if robust else "plain", "formerly bad observations admitted:", cured, "of", int(sc.bad.sum()), cnt)


def test_completion_call_parameters(host):
    """max_error as a NaN, +inf, -inf and a negative number: the twin's export refuses them as the entry point does
    (tests/test_gpu_complete_points.py::test_errors_leave_the_session_alone).  -0.0 is accepted by both -- it is not below zero --
    and admits only an observation whose error is exactly 0: on the planted route under a bad value, every candidate is rejected by
    error, nothing is written, and the result is that of +0.0."""
    case = next(c for c in nf.CASES if c[0] == "nan_signed_xy")
    sc = nf.lanes(case)[0]
    a = nf.chain(host, sc, nf.CAM_D)
    lst, state = a["poses"][2], a["complete_planted"]["filter"][:3]
    for refused in (np.nan, -np.nan, np.inf, -np.inf, -1.0, np.nextafter(nf.THR[0], np.inf)):
        with pytest.raises(AssertionError):
            nf.completed_twice(host, sc, sc.kps, lst, nf.CAM_D, state, max_error=refused)      # host_complete_points returns 3
    outs = [nf.completed_twice(host, sc, sc.kps, lst, nf.CAM_D, state, max_error=z)[0] for z in (-0.0, 0.0)]
    for pts, res, mask, cnt, tr in outs:
        assert cnt["candidates"] == cnt["rejected_by_error"] == a["complete_planted"]["first"][3]["candidates"] > 0 and cnt["admitted"] == 0, cnt
        assert pts.tobytes() == state[0].tobytes() and res.tobytes() == state[1].tobytes() and mask.tobytes() == state[2].tobytes()
        assert np.all(tr["kind"] != ctw.KIND_COMPLETED)
    assert outs[0][3] == outs[1][3] and outs[0][4].tobytes() == outs[1][4].tobytes()


@pytest.mark.parametrize("case", nf.CASES, ids=nf.CASE_IDS)
@pytest.mark.parametrize("cam", sorted(CAMS))
def test_tile_elements_equal_the_gross_outlier_scene(host, cam, case):
    """the elements placement (tracks of 2 .. 130 views, the bad observation at element 0, 63, 64 and last) through the plain and the
    robust triangulation and the point refinement: the robust session in the first form -- but for the 2-view tracks, which are not
    retried (m < 3) and keep the plain record: second form -- the plain session in the second"""
    sc, bad, gr = nf.elements(case)
    poses = sc.poses
    o = sc.tracks[0]
    per_slot = np.repeat(np.arange(len(sc.lengths)), np.diff(o))
    badt = np.zeros(len(sc.lengths), bool)
    badt[sc.bad_tracks()] = True
    two = badt & (np.asarray(sc.lengths) == 2)
    outs = []
    for s in (sc, gr):
        pp, pr = tw.run(host, s.tracks, s.ids, s.kps, poses, CAMS[cam], nf.THR)
        rp, rr, rm, rc, tr = nf.robtw.run(host, s.tracks, s.ids, s.kps, poses, CAMS[cam], nf.THR + (64,), trace=True)
        fp, fr, fc = nf.rtw.run(host, s.tracks, s.ids, s.kps, poses, CAMS[cam], rp, rr, rm, nf.THR[:2])
        qp, qr, qc = nf.rtw.run(host, s.tracks, s.ids, s.kps, poses, CAMS[cam], pp, pr, None, nf.THR[:2])
        outs.append(dict(plain=(pp, pr), robust=(rp, rr, rm, rc), refined=(fp, fr, fc), plain_refined=(qp, qr, qc), trace=tr))
    a, b = outs
    tight = ~two
    for step in ("robust", "refined"):
        assert a[step][0][tight].tobytes() == b[step][0][tight].tobytes(), (case[0], step)
        ok = tight[per_slot] & ~bad
        assert a[step][1][ok].tobytes() == b[step][1][ok].tobytes(), (case[0], step)
        assert not np.isnan(a[step][1][~bad]).any() and nan_bits(a[step][1]) <= {CANONICAL}, (case[0], step)
        float_fields_finite(a[step][0][tight])
    assert a["robust"][2].tobytes() == b["robust"][2].tobytes() and a["robust"][3] == b["robust"][3]
    assert not a["robust"][2][bad & tight[per_slot]].any()
    # (the refinement's counters and cost sums follow the 2-view tracks' plain records and are not compared here)
    # every bad track of 3 and more views went through the hypotheses; those of 64 and more lost the bad observation and nothing else
    # and kept a point; a 3-view track is left with two views 1.2 degrees apart (elements 1, 2 or 0, 1: below min_angle, no consensus)
    # or 2.4 degrees apart (elements 0, 2)
    lengths = np.asarray(sc.lengths)
    tr = a["trace"]
    assert np.all(tr["retried"][badt & ~two] == 1)
    long_bad = badt & (lengths >= 64)
    assert long_bad.sum() == 9 and np.all(tr["mask1"][long_bad] == lengths[long_bad] - 1) and np.all(_lib.succeeded(a["robust"][0])[long_bad])
    three = np.nonzero(badt & (lengths == 3))[0]
    assert [int(tr["mask1"][t]) for t in three] == [-1, -1] and np.all(a["robust"][0]["status"][three] == _lib.TRI_ATTEMPTED | _lib.TRI_ROBUST)
    # the plain records: clean tracks equal, bad ones in the second form
    for step in ("plain", "plain_refined"):
        assert a[step][0][~badt].tobytes() == b[step][0][~badt].tobytes()
        assert a[step][1][~badt[per_slot]].tobytes() == b[step][1][~badt[per_slot]].tobytes()
        float_fields_finite(a[step][0][~badt])
        assert not any(np.isnan(a[step][0][n]).any() for n in ("X", "mean_residual", "tri_angle"))
        assert not np.isnan(a[step][1][~bad]).any() and nan_bits(a[step][1]) <= {CANONICAL}
        for t in np.nonzero(badt)[0]:
            s = int(a[step][0][t]["status"])
            assert s & _lib.TRI_ATTEMPTED and not s & _lib.TRI_ERROR_OK
            if nf.non_finite(case):
                assert s == _lib.TRI_ATTEMPTED and a[step][0][t]["n_views"] == sc.lengths[t] and np.all(a[step][1][o[t]:o[t + 1]] == -1.0)
    for t in np.nonzero(two)[0]:                                  # never retried: the plain record stands in the robust call
        assert a["robust"][0][t].tobytes() == a["plain"][0][t].tobytes()


# ---- the filter on the plain session --------------------------------------------------------------------------------------------------------
PLAIN_PLACEMENTS = {"lanes": nf.lanes, "images": nf.images, "elements": nf.elements}


def plain_session(host, sc, cam, place):
    """plain triangulation, point refinement, the filter under the session's thresholds WITHOUT inlier bytes (the call creates them),
    point refinement -> (poses, the posed mask per slot, the first refinement's outputs, the filter's with its trace, the second
    refinement's).  lanes and images: the chain's own steps under the OLD images' poses; elements: every image posed."""
    if place == "elements":
        poses = sc.poses
        pp, pr = tw.run(host, sc.tracks, sc.ids, sc.kps, poses, cam, nf.THR)
        before = nf.rtw.run(host, sc.tracks, sc.ids, sc.kps, poses, cam, pp, pr, None, nf.THR[:2])
        flt = ftw.run(host, sc.tracks, sc.ids, sc.kps, poses, cam, before[0], before[1], None, nf.THR[:2], trace=True)
    else:
        poses = sc.some(nf.OLD)
        a = nf.chain(host, sc, cam, mh=0, robust=False)
        before, flt = a["refine1"][:3], a["filter0"]
    after = nf.rtw.run(host, sc.tracks, sc.ids, sc.kps, poses, cam, flt[0], flt[1], flt[2], nf.THR[:2])
    return poses, np.isin(sc.tracks[1], [int(i) for i in poses]), before, flt, after


@pytest.mark.parametrize("case", nf.CASES, ids=nf.CASE_IDS)
@pytest.mark.parametrize("cam", sorted(CAMS))
@pytest.mark.parametrize("place", sorted(PLAIN_PLACEMENTS))
def test_the_plain_session_filter(host, place, cam, case):
    """The filter behind the plain triangulation and its point refinement, where a bad track's record is a DLT over the bad observation
    (second form: nothing here is held to the 1e6 scene).  The call creates the inlier bytes: 1 on the posed elements of an ATTEMPTED
    track (msfm_extend.h, plain_byte), whatever the observation holds.
      a non-finite value   the bad tracks are ATTEMPTED alone: not eligible, record, slots and (created) bytes as they were -- 1 on
                           the bad observation too.
      a finite value       (+-3e38, 1e30, the pixel 0) a bad track that has a point lacks ERROR_OK: eligible, trimmed or removed; one
                           without a point stays as under a non-finite value.  Before the call the records of +-3e38 in x hold
                           +inf (mean_residual) and the refinement's cost sums are +inf on the lane and image placements;
                           after it every float field of every record is finite and the next refinement's sums are finite: the
                           filter is the call that cures the only non-finite record fields the library hands out.
    Always: NaNs only in bad slots and only THE NaN, a second call that changes no byte."""
    sc = PLAIN_PLACEMENTS[place](case)[0]
    poses, posed, (qp, qr, qc), (fp, fr, fm, fc, ft), (ap, ar, ac) = plain_session(host, sc, CAMS[cam], place)
    o = sc.tracks[0]
    per_slot = np.repeat(np.arange(len(sc.lengths)), np.diff(o))
    attempted = (qp["status"] & _lib.TRI_ATTEMPTED) != 0
    bad_posed = np.add.reduceat((sc.bad & posed).astype(np.int64), o[:-1]) > 0
    assert bad_posed.sum() >= 5
    created = (posed & attempted[per_slot]).astype(np.uint8)
    same = ft["kind"] <= ftw.KIND_UNTOUCHED
    assert fm[same[per_slot]].tobytes() == created[same[per_slot]].tobytes() and np.all(fm <= created), case[0]
    assert fp[same].tobytes() == qp[same].tobytes() and fr[same[per_slot]].tobytes() == qr[same[per_slot]].tobytes(), case[0]
    has_point = (qp["status"] & _lib.TRI_POINT) != 0
    assert not (qp["status"][bad_posed] & _lib.TRI_ERROR_OK).any()
    assert np.all(ft["kind"][bad_posed & has_point] >= ftw.KIND_TRIMMED) and np.all(ft["kind"][bad_posed & ~has_point] == ftw.KIND_NOT_ELIGIBLE)
    if nf.non_finite(case):
        assert np.all(qp["status"][bad_posed] == _lib.TRI_ATTEMPTED) and np.all(ft["kind"][bad_posed] == ftw.KIND_NOT_ELIGIBLE)
        assert fm[sc.bad & posed].all()                                   # plain_byte's definition: the bad observation included
    else:
        # (+-3e38 in y on the 5-view tracks: the DLT ends without a point, as under a non-finite value; on the elements placement
        # its long tracks give a point whose errors stay below 1e308)
        no_point = case[0] in ("3e38_y", "minus_3e38_y") and place != "elements"
        assert has_point[bad_posed].any() != no_point, case[0]
        if case[0] in ("3e38_x", "minus_3e38_x") and place != "elements":
            assert np.isposinf(qp["mean_residual"][bad_posed & has_point]).any() and qc["cost_before"] == qc["cost_after"] == np.inf, (case[0], qc)
        float_fields_finite(fp)
        assert all(np.isfinite(ac[k]) for k in nf.rtw.COST_KEYS), (case[0], ac)
        float_fields_finite(ap)
    assert not np.isnan(fr[~sc.bad]).any() and nan_bits(fr) <= {CANONICAL} and nan_bits(ar) <= {CANONICAL}, case[0]
    assert not any(np.isnan(fp[n]).any() for n in ("X", "mean_residual", "tri_angle"))
    again = ftw.run(host, sc.tracks, sc.ids, sc.kps, poses, CAMS[cam], fp, fr, fm, nf.THR[:2])
    assert again[0].tobytes() == fp.tobytes() and again[1].tobytes() == fr.tobytes() and again[2].tobytes() == fm.tobytes(), case[0]
    print(place, cam, case[0], "bad tracks by kind", np.bincount(ft["kind"][bad_posed], minlength=5).tolist(), fc)


def test_the_plain_session_filter_reaches_every_kind_on_the_tile_elements(host):
    """over the finite values, on the elements placement (bad tracks of 2 .. 130 views): a bad track is trimmed under one value at
    least, removed by views under one, removed by angle under one"""
    kinds = {}
    for case in nf.CASES:
        if nf.non_finite(case):
            continue
        sc = nf.elements(case)[0]
        _, posed, _, flt, _ = plain_session(host, sc, nf.CAM, "elements")
        bad_posed = np.add.reduceat((sc.bad & posed).astype(np.int64), sc.tracks[0][:-1]) > 0
        kinds[case[0]] = set(int(k) for k in flt[4]["kind"][bad_posed])
    print(kinds)
    for k in (ftw.KIND_TRIMMED, ftw.KIND_REMOVED_BY_VIEWS, ftw.KIND_REMOVED_BY_ANGLE):
        assert any(k in v for v in kinds.values()), (k, kinds)


@pytest.mark.parametrize("case", [c for c in nf.CASES if c[2] == "x" or c[0] == "nan_xy"], ids=lambda c: c[0])
def test_the_routes_are_reached(host, case):
    """On the twins' traces, under CAM, on the images placement: a fixture that quietly misses a route proves nothing."""
    sc = nf.images(case)[0]
    ids, o = sc.ids, sc.tracks[0]
    a = nf.chain(host, sc, nf.CAM, mh=8, robust=True)
    lengths = np.asarray(sc.lengths)
    badt = np.zeros(len(lengths), bool)
    badt[sc.bad_tracks()] = True
    long_bad, short_bad = np.nonzero(badt & (lengths == 8))[0], np.nonzero(badt & (lengths == 3))[0]
    assert len(long_bad) >= 16 and len(short_bad) >= 8
    # the consensus rejected the bad observation of the OLD image: retried, mask 0 there, rescued
    rp, rr, rm, rc, tr = a["robust"]
    assert np.all(tr["retried"][long_bad] == 1) and not rm[o[long_bad] + 4].any() and np.all(rm[o[long_bad] + 3] == 1)
    assert np.all(_lib.succeeded(rp)[long_bad]) and np.all(rp["status"][long_bad] & _lib.TRI_ROBUST)
    assert rc["retried"] == rc["rescued"] == rc["observations_rejected"] == len(long_bad)
    plain = a["plain"][0]
    assert not (plain["status"][long_bad] & _lib.TRI_ERROR_OK).any()
    if nf.non_finite(case):
        assert np.all(plain["status"][long_bad] == _lib.TRI_ATTEMPTED) and not np.isfinite(rr[o[long_bad] + 4]).any()
    # a continued track rejected its bad new observations (images 1 and REG), accepted the clean one (image 0)
    ep, er, em, ec, el, et = a["extend"]
    assert np.all(et["kind"][long_bad] == etw.KIND_CONTINUE) and np.all(et["new_observations"][long_bad] == 3)
    assert np.all(et["accepted"][long_bad] == 1) and not em[o[long_bad] + 1].any() and not em[o[long_bad] + 7].any()
    if nf.non_finite(case):
        assert not np.isfinite(er[o[long_bad] + 1]).any() and not np.isfinite(er[o[long_bad] + 7]).any()
    # a created track: the plain DLT over its three views fails, it is retried, and rescued from the two clean views
    assert np.all(et["kind"][short_bad] == etw.KIND_CREATE) and np.all(et["route"][short_bad] == etw.ROUTE_ROBUST)
    assert np.all(_lib.succeeded(ep)[short_bad]) and np.all(ep["n_views"][short_bad] == 2) and not em[o[short_bad] + 1].any()
    full = tw.run(host, sc.tracks, ids, sc.kps, el, nf.CAM, nf.THR, select=short_bad)[0]
    assert not (full["status"][short_bad] & _lib.TRI_ERROR_OK).any()
    if nf.non_finite(case):
        assert np.all(full["status"][short_bad] == _lib.TRI_ATTEMPTED)
    # the registration drew samples with bad correspondences and succeeded all the same
    reg = a["register"]
    drew = nf.samples_with_bad(host, sc, reg)
    assert drew >= 1 and _lib.registered(reg[0]).all() and nf.registration_bad(sc, reg).sum() >= 16
    # the pose refinement of the images with bad observations stood
    pid, tab = a["poses"][2]
    rec, trc = a["poses"][3], a["poses"][5]
    for pos in nf.BAD_AT:
        k = pid.tolist().index(int(ids[pos]))
        assert trc[k]["verdict"] == 0 and trc[k]["accepted"] >= 1, (pos, trc[k])
    print("%s: retried %d, samples with a bad correspondence %d of %d" % (case[0], rc["retried"], drew, int(reg[0][0]["hypotheses"])))


# ---- the verification stage ---------------------------------------------------------------------------------------------------------------
N_MATCHES, N_BAD = 300, 20


def verify_pair(kind, case):
    """300 matches of a general (or planar) two-view scene with 0.5 px of noise; the value sits in 20 of them, alternately in image 1
    and in image 2 -> (p1, p2, bad [300], the twin pair with 1e6 there)"""
    from monocularsfm_amd import synth
    make = synth.planar_view_pair if kind == "planar" else synth.general_view_pair
    k1, k2, _, _ = make(N_MATCHES, 0, seed=11, noise_px=0.5)
    p = [np.array(k1[:, :2], np.float32), np.array(k2[:, :2], np.float32)]
    g = [a.copy() for a in p]
    bad = np.zeros(N_MATCHES, bool)
    for n, row in enumerate(range(7, N_MATCHES, N_MATCHES // N_BAD)[:N_BAD]):
        bad[row] = True
        if case is not None:
            for ax in case[2]:
                p[n % 2][row, "xy".index(ax)] = nf.value(case[1])
                g[n % 2][row, "xy".index(ax)] = nf.GROSS
    return p[0], p[1], bad, (g[0], g[1])


def verify_all(vhost, phost, p1, p2, cam):
    """every verification twin on one pair -> {name: (kept mask, record or None, schedule or None)}"""
    import pose_twin
    import verify_twin as vt
    camv = np.asarray(tuple(cam) + (0.0,) * (8 - len(cam)), np.float64)
    out = {}
    m = np.zeros(len(p1), np.uint8)
    a, b = np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32)
    k = vhost.host_fundamental_ransac_ex(a.ctypes.data_as(vt.FP), b.ctypes.data_as(vt.FP), len(a), 3.0, 0.99, 1000, 0x5eed5eed,
                                         m.ctypes.data_as(vt.UP))
    out["F"] = (m[:k].astype(bool) if k else np.zeros(len(a), bool), None, None)
    for name, model, select in (("E", 1, False), ("H", 2, False), ("select_F", 0, True), ("select_E", 1, True)):
        out[name] = vt._pair(vhost, model, select, camv, 0.7, 3.0, 0.99, 1000, 0x5eed5eed, a, b)
    mask, rec = pose_twin.geometry(phost, a, b, cam)
    out["pose"] = (mask, rec, None)
    return out


@pytest.fixture(scope="module")
def vhosts():
    import ctypes as C

    import pose_twin
    import verify_twin as vt
    v = vt.load_host()
    v.host_fundamental_ransac_ex.argtypes = [vt.FP, vt.FP, C.c_int, C.c_double, C.c_double, C.c_int, C.c_ulonglong, vt.UP]
    return v, pose_twin.load_host()


@pytest.mark.parametrize("case", nf.CASES, ids=nf.CASE_IDS)
@pytest.mark.parametrize("cam", sorted(CAMS))
@pytest.mark.parametrize("kind", ["general", "planar"])
def test_verification_twins(vhosts, kind, cam, case):
    """The F, E and H RANSAC twins, the model selection under both epipolar models and pose_twin.geometry on a 300-match pair with
    the value planted in 20 matches (10 in either image).  The gross-outlier equivalence holds here as well and is asserted: kept
    lists, selection records, staged schedules and the two-view record are those of the pair with 1e6 in the same coordinates.  A
    sample that draws a bad match gives a model that is not finite or that nothing agrees with; a bad match fails every error test.
    THE DENORMAL AND -0.0 ARE COMPARED ANOTHER WAY: they are the pixel coordinate 0, a place inside the image, and an epipolar test
    has one degree of freedom -- on the planar pair the F twin keeps match 67 with x = 0 px, as it must (0 px lies within 3 px of
    its epipolar line), and does not keep it with 1e6.  What the code owes these two values is that they count as the number they
    are: every output equals, byte for byte, that of the pair with +0.0 in the same coordinates (x - cx is the same double for all
    three)."""
    p1, p2, bad, gross = verify_pair(kind, case)
    zero_like = case[0].startswith(("denormal", "minus_zero"))
    if zero_like:                                           # the twin pair: +0.0 there
        gross = tuple(np.where(g == nf.GROSS, np.float32(0.0), g) for g in gross)
    got = verify_all(*vhosts, p1, p2, CAMS[cam])
    want = verify_all(*vhosts, *gross, CAMS[cam])
    for name, (keep, rec, sched) in got.items():
        if not zero_like:
            assert not keep[bad].any(), (name, np.nonzero(keep & bad)[0])                   # no bad match is kept
        if (name == "H") == (kind == "planar") or name.startswith("select"):
            assert keep.sum() >= 250, (name, int(keep.sum()))                               # ... and the pair is not lost to them
        gk, grec, gsched = want[name]
        assert np.array_equal(keep, gk), (name, np.nonzero(keep != gk)[0])                  # the equivalence
        if name == "pose":
            assert rec["valid"] == 1 and rec["n_kept"] == keep.sum() and rec.tobytes() == grec.tobytes(), (rec, grec)
            assert all(np.all(np.isfinite(rec[f])) for f in ("R", "t", "median_tri_angle", "mean_tri_angle", "mean_residual"))
        else:
            assert rec == grec and sched == gsched, (name, rec, grec, sched, gsched)
            assert sched is None or all(0 < s <= 1000 and 0 < r <= 32 for s, r in sched), sched   # (solved, rounds): finite, in range


# ---- the oracle's anchor: the 1e6 scene against the independent references -----------------------------------------------------------------
@pytest.mark.parametrize("axes", ["x", "y", "xy"])
@pytest.mark.parametrize("cam", sorted(CAMS))
def test_the_gross_scene_against_the_references(host, cam, axes):
    """The twin scene (1e6 in the bad coordinates) of the images placement is finite, so the independent numpy references process it:
    every twin of the chain against its reference, fed the same state, with the comparison functions, guards and tolerances of that
    twin's own reference test (tests/test_*_reference.py); the point and pose refinements with those modules' step_tol 1e-4.  Then
    the filter steps of nf.chain on this scene against tests/filter_ref.py and its completion steps against tests/complete_ref.py."""
    import extend_ref
    import refine_points_ref
    import refine_poses_ref
    import registration_ref
    import robust_triangulation_ref
    import test_extend_points_reference as xe
    import test_refine_points_reference as xr
    import test_refine_poses_reference as xp
    import test_registration_reference as xg
    import test_robust_triangulation_reference as xb
    import test_triangulation_reference as xt
    import triangulation_ref
    case = next(c for c in nf.CASES if c[0] == "nan_" + axes)
    gr = nf.images(case)[2]
    o = gr.tracks[0]

    def bad_slots_apart(res, want, tol):
        """The bad observations' errors are ~1e6 px, where one ulp (1.2e-10) is of the size of the modules' ABSOLUTE tolerances, which
        were measured on errors of a few px: they are held to `tol` RELATIVE to the error here and then handed to the module's
        comparison as the reference's own numbers.  Under CAM_D not even that: 1e6 px lies 400 focal lengths off the axis, where the
        undistortion's fixed-point iteration does not converge and its result depends on the number of steps (the twin's
        kUndistortIters, the references' own): there both must call the observation gross (> 100 x max_error), and every decision
        that the modules' comparisons check -- statuses, inlier bytes, counters -- must still agree.  -> a copy of res"""
        res = np.array(res, copy=True)
        for t, r in enumerate(want):
            for k in np.nonzero(gr.bad[o[t]:o[t + 1]])[0]:
                e = r["residuals"][k]
                if e >= 0:
                    if any(c_[4:]):
                        assert min(res[o[t] + k], e) > 100 * thr[0], (t, k, res[o[t] + k], e)
                    else:
                        assert abs(res[o[t] + k] - e) <= tol * e, (t, k, res[o[t] + k], e)
                        rel.append(abs(res[o[t] + k] - e) / e)
                    res[o[t] + k] = e
        return res

    def clean_only(want, pts, res):
        """the plain call's bad tracks are second-form tracks (their oracle is not this scene): the clean tracks alone"""
        badt = set(int(t) for t in gr.bad_tracks())
        sel = [t for t in range(len(want)) if t not in badt or not (want[t]["status"] & triangulation_ref.ATTEMPTED)]
        return [want[t] for t in sel], pts[sel], np.concatenate([res[o[t]:o[t + 1]] for t in sel])

    c_, thr, H = CAMS[cam], nf.THR, 8
    rel = []                                   # what bad_slots_apart measured
    ids, kps, tracks, kd = gr.ids, gr.kps, gr.tracks, gr.kd()
    first = gr.some(nf.OLD)
    # plain and robust triangulation
    want = triangulation_ref.run(tracks, kd, first, c_, *thr)
    xt.margins_hold(want)
    got = tw.run(host, tracks, ids, kps, first, c_, thr)
    sel_want, sel_pts, sel_res = clean_only(want, *got)
    assert len(sel_want) >= 48
    w = xt.worst(sel_want, (sel_pts, sel_res))
    print("plain:", w)
    xt.within(w)
    want = robust_triangulation_ref.run(tracks, kd, first, c_, *thr, max_hypotheses=H)
    xb.guards_hold(want)
    rob = nf.robtw.run(host, tracks, ids, kps, first, c_, thr + (H,))
    w = xb.worst(want, (rob[0], bad_slots_apart(rob[1], want, xb.TOL_RES), rob[2]))
    print("robust:", w)
    xb.within(w)
    assert rob[3] == xb.counts_of(want) and rob[3]["retried"] >= 16
    # point refinement after the robust call
    pp, pr, pm = rob[:3]
    want = refine_points_ref.run(tracks, kd, first, c_, robust_triangulation_ref.run(tracks, kd, first, c_, *thr, max_hypotheses=H), True,
                                 thr[0], thr[1], *xr.PARAMS)
    xr.guards_hold(want)
    ref1 = nf.rtw.run(host, tracks, ids, kps, first, c_, pp, pr, pm, thr[:2], xr.PARAMS, trace=True)
    w = xr.worst(want, (ref1[0], bad_slots_apart(ref1[1], want, xr.TOL_RES)) + ref1[2:], tracks[0])
    print("refine:", w)
    xr.within(w)
    pp, pr = ref1[:2]
    # registration of REG
    image_id = int(ids[nf.REG])
    reg = nf.regtw.run(host, tracks, pp, [image_id], kd, c_, **nf.REG_PARAMS)
    tids, cu, cv, X = registration_ref.correspondences(tracks, pp, image_id, kd[image_id], c_)
    f = (c_[0] + c_[1]) / 2
    want = registration_ref.register(image_id, cu, cv, X, f, lambda it: nf.regtw.sample3(host, image_id, it, len(cu)), **nf.REG_PARAMS)
    assert want["margin"] > 16 * xg.TOL_RES
    rec, offs, tid, flags, res = reg
    assert np.array_equal(tid, tids) and int(rec[0]["status"]) == want["status"] == 15 and np.array_equal(flags.astype(bool), want["flags"])
    assert int(rec[0]["n_inliers"]) == want["n_inliers"] and int(rec[0]["hypotheses"]) == want["hypotheses"]
    badc = nf.registration_bad(gr, reg)
    wr = dict(R=np.abs(rec[0]["R"].reshape(3, 3) - want["R"]).max(), t=np.abs(rec[0]["t"] - want["t"]).max(),
              res=np.abs(res - want["residuals"])[~badc].max(), res_bad_rel=(np.abs(res - want["residuals"]) / want["residuals"])[badc].max())
    print("register:", wr)
    assert wr["R"] <= xg.TOL_R and wr["t"] <= xg.TOL_T and wr["res"] <= xg.TOL_RES
    assert any(c_[4:]) or wr["res_bad_rel"] <= xg.TOL_RES                          # (see bad_slots_apart)
    # extension by NEW and REG's pose
    new = _lib.registered_poses(rec, gr.some(nf.NEW))
    ext = etw.run(host, tracks, ids, kps, first, new, c_, pp, pr, pm, thr, H, trace=True)
    want = extend_ref.run(tracks, kd, first, new, c_, pp, pr, pm, thr[0], thr[1], thr[2], H)
    c = dict(name="gross", cam=c_, thr=thr, mh=H, tracks=tracks, ids=ids, kps=kps, before=(pp, pr, pm), lst=first, new=new, want=want,
             got=(ext[0], bad_slots_apart(ext[1], want, xe.TOL["new_residual"])) + ext[2:])
    worst, touched, left, margins = xe.compare(c)
    print("extend:", worst, touched, left, margins)
    assert not left and touched == len(gr.lengths) and all(worst[q] <= xe.TOL[q] for q in xe.TOL), worst
    # pose refinement
    pp, pr, pm, _, lst = ext[:5]
    poses = ptw.poses_dict(*lst)
    # (REG is held as well: the registration has just left it at its own optimum, where the reference's first decision -- does the
    # cost drop? -- sits 1e-16 from its threshold, inside that module's guard; left out, it would take every 8-view track's re-verdict
    # out of the comparison with it)
    fixed = [int(ids[nf.OLD[0]]), int(ids[nf.REG])]
    params = (10, 1e-4, 15)
    want = refine_poses_ref.run(tracks, kd, poses, c_, xp.records_of(pp, pr, tracks[0]), pm, thr[0], thr[1], *params, fixed=set(fixed))
    got = ptw.run(host, tracks, ids, kps, poses, c_, pp, pr, pm, thr[:2], params, fixed, trace=True)   # (both by ascending id)
    got = (got[0], bad_slots_apart(got[1], want[2], xp.TOL["res"])) + got[2:]
    w, compared, left_out, n_tracks = xp.compare(dict(want=want, got=got, tracks=tracks), xp.TOL)
    print("poses:", w, compared, left_out, n_tracks)
    assert compared == 6 and not left_out and n_tracks == len(gr.lengths) and all(w[k] <= xp.TOL[k] for k in xp.TOL), w
    # the filter at the end of the twin scene's chain, under every pair, after the extension with max_hypotheses 8 and 0 (with 0 the bad
    # 3-view tracks are plain records over the 1e6 observation: eligible, the observation FITTING, dropped by error on both sides);
    # the comparison and the tolerances of tests/test_filter_points_reference.py
    import complete_ref
    import filter_ref
    import test_complete_points_reference as xc
    import test_filter_points_reference as xf
    rel.clear()
    for mh in (8, 0):
        g = nf.chain(host, gr, c_, mh=mh)
        pp, pr, pm, lst = g["refine2"][0], g["refine2"][1], g["extend"][2], g["poses"][2]
        for name, pair in nf.FILTER_PAIRS:
            want = filter_ref.run(tracks, kd, ptw.poses_dict(*lst), c_, pp, pr, pm, thr[:2], pair)
            got = g["filter"][name]
            got = (got[0], bad_slots_apart(got[1], want, xf.TOL["residual"])) + got[2:]
            w, eligible, left, margins = xf.compare(dict(name=(name, mh), tracks=tracks, before=(pp, pr, pm), got=got, want=want))
            print("filter %s, max_hypotheses %d:" % (name, mh), w, eligible, left, margins, got[3])
            assert eligible == len(gr.lengths) and not left and all(w[q] <= xf.TOL[q] for q in xf.TOL), (name, mh, w, left)
        # the completion steps of the same chain against tests/complete_ref.py, fed the twin's state before each call (on the planted
        # route: the filter's outputs under the moved keypoints); the comparison and the tolerances of
        # tests/test_complete_points_reference.py -- DESIGN.md section 22's bounds -- and no track left out by its guards
        for name, before, first, _ in completion_steps(g):
            want = complete_ref.run(tracks, kd, ptw.poses_dict(*lst), c_, before[0], before[1], before[2], thr[:2])
            got = (first[0], bad_slots_apart(first[1], want, xc.TOL["residual"])) + first[2:]
            w, eligible, left, margins = xc.compare(dict(name=(name, mh), tracks=tracks, before=before, got=got, want=want))
            print("completion %s, max_hypotheses %d:" % (name, mh), w, eligible, left, margins, got[3])
            assert eligible >= 48 and got[3]["completed"] > 0 and not left and all(w[q] <= xc.TOL[q] for q in xc.TOL), (name, mh, w, left)
    print("filter: the bad observations' errors, worst difference relative to their size: %.3g over %d slots" % (max(rel, default=0.0), len(rel)))
    assert any(c_[4:]) or len(rel) > 0


# ---- the other fixtures of tests/test_gpu_nonfinite.py, on the twins first ------------------------------------------------------------------
@pytest.mark.parametrize("T", [257, 256, 255, 65, 64, 63, 1])
def test_track_count_prefixes_on_the_twins(host, T):
    for case in nf.drawn(seed=11, k=4):
        sc, _, gr = nf.lanes(case)
        sc, gr = sc.prefix(T), gr.prefix(T)
        assert len(sc.bad_tracks()) == sum(t < T for t in nf.LANES)
        for mh in (8, 0):
            a, b = nf.chain(host, sc, nf.CAM, mh=mh), nf.chain(host, gr, nf.CAM, mh=mh)
            compare(sc, case, a, b, mh, True)
            compare_filter(host, sc, case, nf.CAM, a, b, mh, True, routes=False)     # (one track has no clean neighbour to leave untouched)
            compare_complete(host, sc, gr, case, "cam", a, b, mh, True, routes=False)
            pl = a["complete_planted"]                                               # every bad track of the prefix: planted, completed
            assert np.all(pl["first"][4]["kind"][sc.bad_tracks()] == ctw.KIND_COMPLETED), (T, case[0], mh, pl["first"][4][sc.bad_tracks()])


@pytest.mark.parametrize("case", nf.CASES, ids=nf.CASE_IDS)
def test_replaced_keypoints_on_the_twins(host, case):
    """The records and inlier bytes come from clean keypoints (every byte 1), then the keypoints are replaced: the bad observations are
    IN the fitting sets of the point refinement.  It ends; no record takes a NaN; a track whose fitting set holds a non-finite
    observation is not refined (its cost is not a number: no step is accepted); the registration and the extension that follow treat
    the value as on any other session; the filter drops exactly the replaced observations."""
    clean = nf.lanes(None)[0]
    sc, _, gr = nf.lanes(case)
    first = sc.some(nf.OLD)
    pp, pr, pm, _ = nf.robtw.run(host, clean.tracks, clean.ids, clean.kps, first, nf.CAM, nf.THR + (8,))
    assert pm.sum() == len(nf.OLD) * len(sc.lengths)                       # every observation of a posed image supports its point
    outs = []
    for s in (sc, gr):
        fp, fr, fc, tr = nf.rtw.run(host, s.tracks, s.ids, s.kps, first, nf.CAM, pp, pr, pm, nf.THR[:2], trace=True)
        reg = nf.regtw.run(host, s.tracks, fp, [int(s.ids[nf.REG])], s.kd(), nf.CAM, **nf.REG_PARAMS)
        new = _lib.registered_poses(reg[0], s.some(nf.NEW))
        ext = etw.run(host, s.tracks, s.ids, s.kps, first, new, nf.CAM, fp, fr, pm, nf.THR, 8, trace=True)
        outs.append((fp, fr, fc, tr, reg, ext))
    (fp, fr, fc, tr, reg, ext), g = outs
    badt = sc.bad_tracks()
    clean_t = np.setdiff1d(np.arange(len(sc.lengths)), badt)
    per_slot = np.repeat(np.isin(np.arange(len(sc.lengths)), badt), np.diff(sc.tracks[0]))
    float_fields_finite(fp[clean_t])
    assert not any(np.isnan(fp[n]).any() for n in ("X", "mean_residual", "tri_angle"))
    assert fp[clean_t].tobytes() == g[0][clean_t].tobytes() and fr[~per_slot].tobytes() == g[1][~per_slot].tobytes()
    assert nan_bits(fr) <= {CANONICAL} and not np.isnan(fr[~sc.bad]).any()
    if nf.non_finite(case):
        assert not _lib.refined(fp)[badt].any() and fp[badt].tobytes() == pp[badt].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(reg[:4], g[4][:4])) and _lib.registered(reg[0]).all()
    assert nan_bits(reg[4]) <= {CANONICAL} and nan_bits(ext[1]) <= {CANONICAL}
    assert ext[0][clean_t].tobytes() == g[5][0][clean_t].tobytes() and ext[2].tobytes() == g[5][2].tobytes() and ext[3] == g[5][3]
    print(case[0], fc, tr[badt]["verdict"], tr[badt]["accepted"])
    # the filter right behind the upload, under the session's thresholds: the observations dropped are exactly the bad observations in
    # posed images (each by error: their tracks are trimmed, every other track is untouched), the trimmed tracks' slots are rewritten
    # (a NaN's with THE NaN), and everything equals the twin scene's
    posed = np.isin(sc.tracks[1], [int(i) for i in first])
    (qp, qr, qm, qc, qt), w = [ftw.run(host, s.tracks, s.ids, s.kps, first, nf.CAM, pp, pr, pm, nf.THR[:2], trace=True) for s in (sc, gr)]
    assert qm.tobytes() == np.where(sc.bad & posed, 0, pm).astype(np.uint8).tobytes() and (sc.bad & posed).sum() == len(badt)
    assert (qc["dropped_by_error"], qc["dropped_by_depth"], qc["trimmed"]) == (len(badt), 0, len(badt)), qc
    assert np.all(qt["kind"][badt] == ftw.KIND_TRIMMED) and np.all(qt["kind"][clean_t] == ftw.KIND_UNTOUCHED)
    assert qp.tobytes() == w[0].tobytes() and qm.tobytes() == w[2].tobytes() and qc == w[3] and qt.tobytes() == w[4].tobytes()
    assert qr[~sc.bad].tobytes() == w[1][~sc.bad].tobytes() and qr[~per_slot].tobytes() == pr[~per_slot].tobytes()
    assert nan_bits(qr) <= {CANONICAL} and not np.isnan(qr[~sc.bad]).any()
    assert np.isnan(qr[sc.bad & posed]).all() == case[0].startswith("nan") and not (qr[sc.bad & posed] <= nf.THR[0]).any()
    float_fields_finite(qp)
