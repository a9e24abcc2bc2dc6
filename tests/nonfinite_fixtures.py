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

import extend_twin as etw
import filter_twin as ftw
import refine_points_twin as rtw
import refine_poses_twin as ptw
import registration_twin as regtw
import robust_triangulation_twin as robtw
import triangulation_twin as tw
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
    lengths, bad (bool per observation slot)"""
    def __init__(self, ids, kps, poses, lst, lengths, bad):
        self.ids, self.kps, self.poses, self.lst, self.lengths, self.bad = ids, kps, poses, lst, list(lengths), bad
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
                     self.bad[:int(np.sum(lengths))])


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
    for t, positions in where.items():
        for pos in positions:
            assert pos < lengths[t]
            bad[offs[t] + pos] = True
            if case is None:
                continue
            for ax in case[2]:
                kps[pos][t, "xy".index(ax)] = value(case[1])
                gross[pos][t, "xy".index(ax)] = GROSS
    return Scene(ids, kps, poses, lst, lengths, bad), bad, Scene(ids, gross, poses, lst, lengths, bad)


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
    pts, res, mask = out["filter"]["mix"][:3]
    out["refine3"] = rtw.run(host, tracks, ids, kps, lst, cam, pts, res, mask, thr[:2], trace=trace)
    return out


def load_host():
    L = ftw.load_host()                  # (etw.load_host()'s exports and host_filter_points)
    R = regtw.load_host()
    for name in ("host_register_counts", "host_register_images", "host_register_sample3", "host_p3p", "host_register_refine"):
        f = getattr(R, name)
        g = getattr(L, name)
        g.argtypes, g.restype = f.argtypes, f.restype
    return L


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
