"""Inputs shared by the CPU and GPU tests of non-finite and huge keypoint coordinates: msfm_upload_keypoints does
not validate coordinates, so a NaN, an infinity, 3e38 or a denormal reaches every kernel that reads a keypoint.  The scenes are the
ring jobs of tests/test_gpu_robust_triangulation.ring_job with BAD OBSERVATIONS planted in them; every scene comes with its TWIN SCENE,
in which every bad coordinate is 1e6 instead: a finite gross outlier that the independent numpy references can process and that the
library must treat exactly as it treats the bad value (only the bad observations' own residual slots may differ).  chain() runs the
host twins through the whole reconstruction stage on such a scene.  Test infrastructure only.

The layout of every chain scene: tracks of 8 views through the images 0 .. 7 and tracks of 3 views through 0, 1, 2; the images
2 .. 6 are posed at the triangulation (OLD), 0 and 1 arrive by msfm_extend_points (NEW), 7 is registered (REG) and arrives with them.
A bad 8-view track carries the bad value in an OLD image (4), a NEW one (1) and REG (7): the consensus rejects the first, the
continuation the second, the registration meets the third.  A bad 3-view track carries it in image 1: not attempted at the
triangulation (one posed view), created by the extension from the views 0, 1, 2, of which 0 and 2 (2.4 degrees apart) agree."""
import numpy as np

import complete_twin as ctw
import extend_twin as etw
import filter_twin as ftw
import refine_points_twin as rtw
import refine_poses_twin as ptw
import registration_twin as regtw
import robust_triangulation_twin as robtw
import triangulation_twin as tw
import twin_host
from monocularsfm_amd import _lib
from refine_points_fixtures import tracks_of
from test_gpu_robust_triangulation import ring_job

CAM = (2500.0, 2500.0, 1536.0, 1152.0)
CAM_D = CAM + (-0.1, 0.02, 1e-3, -5e-4)
THR = (2.0, 1.5, 2)                  # the reference's Triangulator::Parameters
GROSS = np.float32(1e6)              # the twin scene's coordinate
# msfm_filter_points at the end of the chain: under the session's own thresholds it drops nothing there (every track untouched: the
# no-op path alone), so the filter steps pass explicit (max_error px, min_angle degrees) -- the three pairs that reach its routes on
# the 0.3 px ring jobs (tests/test_nonfinite_reference.py asserts that they do)
FILTER_MIX = (0.45, 1.5)             # a mix of untouched and trimmed tracks
FILTER_ANGLE = (2.0, 12.0)           # every track removed by angle, nothing dropped
FILTER_VIEWS = (0.3, 20.0)           # removed by views and by angle
# ... and a fourth.  Under FILTER_MIX the five bad tracks of the lane placement under CAM end untouched (3) or removed by views (2):
# none is TRIMMED, the one route that rewrites a bad observation's slot.  0.6 px is two sigma of the ring jobs' 0.3 px of noise per
# axis: an error passes it with probability 1 - exp(-2) = 0.86, a track with five fitting observations loses at least one with
# probability 0.5 and four of them with 1e-3 -- about half the tracks are trimmed, hardly any is removed.
FILTER_TRIM = (0.6, 1.5)
FILTER_PAIRS = (("mix", FILTER_MIX), ("angle", FILTER_ANGLE), ("views", FILTER_VIEWS), ("trim", FILTER_TRIM))

# float32 bit patterns
VALUES = (("nan", 0x7fc00000), ("nan_signed", 0xffc00000), ("nan_payload", 0x7fc00001), ("inf", 0x7f800000), ("minus_inf", 0xff800000),
          ("3e38", int(np.float32(3e38).view(np.uint32))), ("minus_3e38", int(np.float32(-3e38).view(np.uint32))),
          ("1e30", int(np.float32(1e30).view(np.uint32))), ("denormal", 0x00000001), ("minus_zero", 0x80000000))
# (name, bits, the coordinates that get the value): x alone, y alone, and for a NaN both
CASES = tuple((n + "_" + ax, b, ax) for n, b in VALUES for ax in (("x", "y", "xy") if n.startswith("nan") else ("x", "y")))
CASE_IDS = [c[0] for c in CASES]
NON_FINITE = frozenset(n for n, b in VALUES if (b & 0x7f800000) == 0x7f800000)


def non_finite(case):
    return case[0].rsplit("_", 1)[0] in NON_FINITE


def drawn(seed, k=4):
    """k cases from a fixed seed (the GPU tests; the full product is the CPU tests' job), always with one signed-NaN and one infinity
    among them: the values whose NaNs the two sides generate or propagate differently"""
    rng = np.random.default_rng(seed)
    pick = [int(rng.choice([i for i, c in enumerate(CASES) if c[0].startswith("nan_signed")])),
            int(rng.choice([i for i, c in enumerate(CASES) if "inf" in c[0]]))]
    rest = [i for i in range(len(CASES)) if i not in pick]
    pick += [int(i) for i in rng.choice(rest, k - 2, replace=False)]
    return [CASES[i] for i in pick]


def value(bits):
    return np.asarray([bits], np.uint32).view(np.float32)[0]


OLD, NEW, REG = (2, 3, 4, 5, 6), (0, 1), 7
BAD_AT = (1, 4, 7)                   # the elements of a bad 8-view track that carry the value
BAD_AT_SHORT = (1,)                  # of a bad 3-view track


class Scene:
    """ids, kps (list by image position), poses (the true ones, dict by id), lst (for tracks_add), tracks (the finished result),
    lengths, bad (bool per observation slot), clean (the keypoints without any bad value: what the cure uploads; None: kps)"""
    def __init__(self, ids, kps, poses, lst, lengths, bad, clean=None):
        self.ids, self.kps, self.poses, self.lst, self.lengths, self.bad = ids, kps, poses, lst, list(lengths), bad
        self.clean = kps if clean is None else clean
        self.tracks = tracks_of(self.lengths, ids)
        self.rows = len(kps[0])

    def some(self, positions):
        return {int(self.ids[p]): self.poses[int(self.ids[p])] for p in positions}

    def kd(self):
        return {int(i): k for i, k in zip(self.ids, self.kps)}

    def bad_tracks(self):
        return np.nonzero(np.add.reduceat(self.bad.astype(np.int64), self.tracks[0][:-1]) > 0)[0]

    def prefix(self, T):
        """the scene of the first T tracks (keypoint rows beyond them stay: nothing reads them)"""
        lengths = self.lengths[:T]
        n_img = max(lengths)
        full = ring_list(lengths, self.ids)
        return Scene(self.ids[:n_img], self.kps[:n_img], {int(i): self.poses[int(i)] for i in self.ids[:n_img]}, full, lengths,
                     self.bad[:int(np.sum(lengths))], self.clean[:n_img])


def ring_list(lengths, ids):
    from refine_points_fixtures import ring_list as rl
    return rl(lengths, ids)


def placed(lengths, where, case=None, seed=3, noise_px=0.3):
    """lengths: the ring job's track lengths; where: {track: element positions that carry the bad value}; case: an entry of CASES, or
    None for the clean scene (the mask still marks `where`).
    -> (the scene, its bad mask [observation slots], the twin scene with 1e6 in every bad coordinate)"""
    ids, kps, poses, lst = ring_job(lengths, noise_px=noise_px, seed=seed)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    bad = np.zeros(int(offs[-1]), bool)
    gross = [k.copy() for k in kps]
    clean = [k.copy() for k in kps]
    for t, positions in where.items():
        for pos in positions:
            assert pos < lengths[t]
            bad[offs[t] + pos] = True
            if case is None:
                continue
            for ax in case[2]:
                kps[pos][t, "xy".index(ax)] = value(case[1])
                gross[pos][t, "xy".index(ax)] = GROSS
    return Scene(ids, kps, poses, lst, lengths, bad, clean), bad, Scene(ids, gross, poses, lst, lengths, bad, clean)


# ---- the placements -----------------------------------------------------------------------------------------------------------------------
LANES = (0, 63, 64, 255, 256)


def lanes(case=None):
    """257 tracks of 8 views; the bad ones at the lanes 0, 63 | 64, 255 | 256: the wave and block edges of every one-lane-per-track kernel"""
    return placed([8] * 257, {t: BAD_AT for t in LANES}, case)


def whole_wave(case=None):
    """192 tracks of 8 views, every track of the middle wave (64 .. 127) bad, in ONE of the elements 1, 4, 7 by turns: that wave's
    reductions carry nothing else.  (One bad observation per track: with all three in every track of the wave, the denormal and -0.0
    -- the pixel 0, a place inside the image -- and 1e6 part under CAM_D on a few tracks, whose consensus differs between the two;
    that is the fixture's doing, not the code's, and the lane and image placements keep three per track.)"""
    return placed([8] * 192, {t: (BAD_AT[t % 3],) for t in range(64, 128)}, case)


IMAGES_T = 72
IMAGES_SHORT = tuple(range(5, IMAGES_T, 9))      # the 3-view tracks
IMAGES_BAD = tuple(range(2, IMAGES_T, 3))        # every third track is bad (the 3-view tracks 5, 14, .. among them)


def images(case=None):
    """72 tracks, every ninth of 3 views (created by the extension), every third one bad: a third of the registered image's
    correspondences are bad, so its RANSAC samples meet them"""
    lengths = [3 if t in IMAGES_SHORT else 8 for t in range(IMAGES_T)]
    return placed(lengths, {t: (BAD_AT_SHORT if t in IMAGES_SHORT else BAD_AT) for t in IMAGES_BAD}, case)


ELEMENT_LENGTHS = (2, 3, 64, 65, 130)


def elements(case=None):
    """tracks of 2, 3, 64, 65 and 130 views with the bad observation at element 0, 63, 64 and last (where the track has it): the
    64-observation LDS tiles of trr_retry_kernel; a clean track of every length between them"""
    lengths, where = [], {}
    for m in ELEMENT_LENGTHS:
        for pos in sorted({0, 63, 64, m - 1}):
            if pos < m:
                where[len(lengths)] = (pos,)
                lengths.append(m)
        lengths.append(m)
    return placed(lengths, where, case)


# ---- the chain of host twins --------------------------------------------------------------------------------------------------------------
REG_PARAMS = dict(min_inliers=15)
POSE_PARAMS = (10, 1e-6, 15)


# msfm_complete_points behind the filter: the pairs whose trimmed tracks hold candidates again (behind FILTER_ANGLE and FILTER_VIEWS
# nearly every track is removed and no longer stands)
COMPLETE_BEHIND = ("mix", "trim")
PLANT_AT = 3                         # the element of an 8-view track that the planted step moves: an OLD image, not in BAD_AT
PLANT_PX = np.float32(40.0)


def completed_twice(host, sc, kps, lst, cam, state, thr=THR, max_error=None, scope=()):
    """complete_twin.run from `state` = (records, residuals, inlier bytes) at max_error (None: the session's), then once more from its
    own outputs: the fixed point on the twin.  -> (first, again), each (records, residuals, bytes, counters, trace)"""
    first = ctw.run(host, sc.tracks, sc.ids, kps, lst, cam, state[0], state[1], state[2], thr[:2], max_error, scope, trace=True)
    again = ctw.run(host, sc.tracks, sc.ids, kps, lst, cam, first[0], first[1], first[2], thr[:2], max_error, scope, trace=True)
    return first, again


def planted_tracks(sc):
    """the tracks of the planted step: every third 8-view track and every bad 8-view track.  The bad 3-view tracks of the images
    placement are left out: they have no element PLANT_AT, and with two fitting views (0 and 2) they cannot lose one -- the filter
    would remove them by views and nothing would stand to be completed."""
    bad = set(int(t) for t in sc.bad_tracks())
    return np.asarray([t for t, n in enumerate(sc.lengths) if n == 8 and (t % 3 == 0 or t in bad)], np.int64)


def moved_keypoints(sc):
    """the scene's keypoints with the clean observation at element PLANT_AT of every planted track moved by 40 px in y"""
    kps = list(sc.kps)
    k = np.array(kps[PLANT_AT], copy=True)
    k[planted_tracks(sc), 1] += PLANT_PX
    kps[PLANT_AT] = k
    return kps


def complete_planted(host, sc, lst, cam, state, thr=THR):
    """The deterministic route into a completed bad track (tests/test_gpu_complete_points.plant on the twins): under
    moved_keypoints(sc) the filter twin runs from `state` (the chain's state behind refine2) with the session's thresholds and drops
    the moved observations; then the completion runs twice under the scene's ORIGINAL keypoints.  X did not move and the observation
    fitted before, so it is admitted again: every planted track that stands is COMPLETED, and in a bad one the bad observations --
    byte 0 and USED -- are the candidates rejected beside it.  -> dict(where = planted_tracks, filter, first, again)"""
    flt = ftw.run(host, sc.tracks, sc.ids, moved_keypoints(sc), lst, cam, state[0], state[1], state[2], thr[:2], None, trace=True)
    first, again = completed_twice(host, sc, sc.kps, lst, cam, flt[:3], thr)
    return dict(where=planted_tracks(sc), filter=flt, first=first, again=again)


# ---- what a completion call owes a bad observation (tests/test_nonfinite_reference.py and tests/test_gpu_nonfinite.py) ------------------
CANONICAL = 0x7ff8000000000000


def bad_slot_class(case, cam):
    """What a REWRITTEN bad slot of a completed track holds (point_verdict writes canonical(err) into the slot of every USED
    observation; err = f * |projection - undistorted observation|):
      a NaN coordinate        the difference is a NaN under either camera: THE NaN.
      an infinite coordinate  CAM: (inf - cx) / fx = inf, its square inf, the root inf, times f: +inf for either sign.  CAM_D: the
                              undistortion's first step multiplies inf by a factor built from inf (inf - inf, or inf * 0 in the
                              tangential term): a NaN, so THE NaN.
      3e38, -3e38, 1e30       CAM: the distance in px from the projection to the value, about |value|: finite (3e38 / fx squared is
                              1.4e70) and beyond 1e29.  CAM_D: the fixed-point undistortion leaves a finite number that depends on
                              the step count; what is owed is "finite or +inf, never a NaN -- or THE NaN --
                              and never within max_error": asserted as `not (slot <= max_error)` and THE NaN alone.  (Measured on
                              the chain scenes: finite, about |value|, as under CAM.)
      the denormal, -0.0      the pixel 0: a finite error of hundreds of px or more under both cameras.
    -> "nan", "inf", "huge", "gross" (finite, beyond max_error) or "any" (CAM_D under a huge finite value)"""
    name = case[0].rsplit("_", 1)[0]
    distorted = any(cam[4:])
    if name.startswith("nan"):
        return "nan"
    if name in ("inf", "minus_inf"):
        return "nan" if distorted else "inf"
    if name in ("3e38", "minus_3e38", "1e30"):
        return "any" if distorted else "huge"
    return "gross"


def holds_class(slots, kind, max_error):
    slots = np.ascontiguousarray(slots, np.float64)
    if kind == "nan":
        return bool(np.all(slots.view(np.uint64) == CANONICAL))
    if kind == "inf":
        return bool(np.all(np.isposinf(slots)))
    if kind == "huge":
        return bool(np.all(np.isfinite(slots) & (slots > 1e29)))
    if kind == "gross":
        return bool(np.all(np.isfinite(slots) & (slots > 100 * max_error)))
    return not bool(np.any(slots <= max_error)) and bool(np.all(slots.view(np.uint64)[np.isnan(slots)] == CANONICAL))


def completion_routes(sc, case, cam, posed, before, out, tight=None, what=None, scope=None):
    """One completion call: `before` = (records, residuals, bytes) it started from, `out` = (records, residuals, bytes, counters, the
    twin's trace) behind it; posed: bool per slot, the elements in an image with a pose; tight: bool per track, None = every track
    (the second-form tracks are left out: tests/test_nonfinite_reference.py); scope: the call's image list, None = every image.
    Asserted:
      rejection   no bad observation gets byte 1; every bad observation of an eligible track in a posed (and listed) image is a
                  candidate and is rejected by its error: the track's rejections by depth are 0, those by error at least its bad observations.
      untouched   a track that is not COMPLETED is bit for bit what it was, its bad slots included; the bytes only rise.
      completed   a completed bad track: every bad slot holds what bad_slot_class says and nothing else, the clean ones an error;
                  n_views = the bytes = those before + admitted, none on a bad observation; mean_residual finite, within max_error.
    -> (the completed bad tracks, the UNTOUCHED bad tracks with a rejected bad candidate): bool per track"""
    o = sc.tracks[0]
    T = len(sc.lengths)
    per_slot = np.repeat(np.arange(T), np.diff(o))
    tight = np.ones(T, bool) if tight is None else tight
    badt = np.zeros(T, bool)
    badt[sc.bad_tracks()] = True
    listed = np.ones(len(posed), bool) if scope is None else np.isin(sc.tracks[1], [int(i) for i in scope])
    # the bad candidates per track (a one-track scene registers no image: REG stays without a pose and its element is not USED)
    n_bad = np.add.reduceat((sc.bad & posed & listed).astype(np.int64), o[:-1])
    p0, r0, m0 = before
    pa, sa, ma, ca, ta = out
    max_error = THR[0]
    assert not ma[sc.bad & tight[per_slot]].any(), (what, np.nonzero((ma != 0) & sc.bad & tight[per_slot])[0][:8])
    kind = ta["kind"]
    by_error = ta["candidates"] - ta["admitted"] - ta["rejected_by_depth"]
    sel = (kind != ctw.KIND_NOT_ELIGIBLE) & tight & badt
    assert np.all(ta["rejected_by_depth"][sel] == 0) and np.all(by_error[sel] >= n_bad[sel]), (what, ta[sel], n_bad[sel])
    same = kind != ctw.KIND_COMPLETED
    assert pa[same].tobytes() == p0[same].tobytes() and sa[same[per_slot]].tobytes() == r0[same[per_slot]].tobytes(), what
    assert ma[same[per_slot]].tobytes() == m0[same[per_slot]].tobytes() and np.all(ma >= m0), what
    untouched = (kind == ctw.KIND_UNTOUCHED) & tight & badt & (by_error >= np.maximum(n_bad, 1))
    done = (kind == ctw.KIND_COMPLETED) & tight & badt
    slot_class = bad_slot_class(case, cam)
    for t in np.nonzero(done)[0]:
        sl = slice(int(o[t]), int(o[t + 1]))
        bad_used = (sc.bad & posed)[sl]                                    # (the slot of an element in an image without a pose: -1)
        assert holds_class(sa[sl][bad_used], slot_class, max_error), (what, t, slot_class, sa[sl][bad_used])
        assert not (sa[sl][bad_used] <= max_error).any() and np.all(sa[sl][posed[sl] & ~bad_used] >= 0.0), (what, t, sa[sl])
        assert pa[t]["n_views"] == ma[sl].sum() == m0[sl].sum() + ta[t]["admitted"] and not ma[sl][sc.bad[sl]].any(), (what, t, pa[t])
        assert np.isfinite(pa[t]["mean_residual"]) and pa[t]["mean_residual"] <= max_error, (what, t, pa[t])
        assert ta[t]["admitted"] >= 1 and by_error[t] >= n_bad[t] >= (scope is None), (what, t, ta[t])
    return done, untouched


def chain(host, sc, cam=CAM, thr=THR, H=8, mh=8, robust=True, trace=True):
    """The reconstruction stage's twins over one scene, each fed the previous one's outputs: triangulation (plain, or robust with H
    hypotheses), point refinement, registration of REG, extension by NEW + REG's registered pose with max_hypotheses mh, pose refinement
    (image OLD[0] fixed), point refinement again; then the filter once per pair of FILTER_PAIRS, each from that same state, and a
    point refinement behind the first of them.  On the plain session (robust=False) the filter also runs behind the first point
    refinement, under the session's thresholds and without inlier bytes (it creates them) -- a side step: the steps after it start from
    the refinement's outputs, as they always did.  -> dict step -> that twin's outputs (tuples as the twins return them; "filter" is a
    dict by pair name; None for a step that did not run: REG is absent from scenes with fewer than 8 images, "filter0" from the
    robust session)"""
    ids, kps, tracks = sc.ids, sc.kps, sc.tracks
    first = sc.some([p for p in OLD if p < len(ids)])
    out = {}
    out["plain"] = tw.run(host, tracks, ids, kps, first, cam, thr)
    if robust:
        r = robtw.run(host, tracks, ids, kps, first, cam, thr + (H,), trace=trace)
        out["robust"] = r
        pts, res, mask = r[0], r[1], r[2]
    else:
        (pts, res), mask = out["plain"], None
    out["refine1"] = rtw.run(host, tracks, ids, kps, first, cam, pts, res, mask, thr[:2], trace=trace)
    pts, res = out["refine1"][:2]
    out["filter0"] = None if robust else ftw.run(host, tracks, ids, kps, first, cam, pts, res, None, thr[:2], trace=True)
    new = sc.some([p for p in NEW if p < len(ids)])
    out["register"] = None
    if REG < len(ids):
        out["register"] = regtw.run(host, tracks, pts, [int(ids[REG])], sc.kd(), cam, **REG_PARAMS)
        new = _lib.registered_poses(out["register"][0], new)
    out["extend"] = etw.run(host, tracks, ids, kps, first, new, cam, pts, res, mask, thr, mh, trace=trace)
    pts, res, mask, _, lst = out["extend"][:5]
    fixed = [int(ids[OLD[0]])]
    out["poses"] = ptw.run(host, tracks, ids, kps, lst, cam, pts, res, mask, thr[:2], POSE_PARAMS, fixed, trace=trace)
    pts, res, lst = out["poses"][:3]
    out["refine2"] = rtw.run(host, tracks, ids, kps, lst, cam, pts, res, mask, thr[:2], trace=trace)
    pts, res = out["refine2"][:2]
    out["filter"] = {name: ftw.run(host, tracks, ids, kps, lst, cam, pts, res, mask, thr[:2], pair, trace=True) for name, pair in FILTER_PAIRS}
    out["complete"] = {name: completed_twice(host, sc, kps, lst, cam, out["filter"][name][:3], thr) for name in COMPLETE_BEHIND}
    out["complete_planted"] = complete_planted(host, sc, lst, cam, (pts, res, mask), thr)
    pts, res, mask = out["filter"]["mix"][:3]
    out["refine3"] = rtw.run(host, tracks, ids, kps, lst, cam, pts, res, mask, thr[:2], trace=trace)
    return out


load_host = twin_host.load


def registration_bad(sc, reg):
    """the bad mask of the registration's correspondence slots: the tracks whose observation in REG is bad"""
    o = sc.tracks[0]
    bad_reg = np.asarray([lengths > REG and bool(sc.bad[o[t] + REG]) for t, lengths in enumerate(sc.lengths)])
    return bad_reg[reg[2]]


def samples_with_bad(host, sc, reg):
    """how many of the hypotheses the registration of REG ran drew at least one bad correspondence"""
    rec, off, tid = reg[0], reg[1], reg[2]
    badc = registration_bad(sc, reg)
    n = int(off[1] - off[0])
    return sum(1 for it in range(int(rec[0]["hypotheses"])) if badc[regtw.sample3(host, int(sc.ids[REG]), it, n)].any())
