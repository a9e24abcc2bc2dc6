"""Scenes for the two-view pose refinement (csrc/msfm_pose_refine.h, tv_refine_kernel): every case is a two_view_fixtures.case built
on two_view(..., keypoints=) with 0.7 px of Gaussian noise and a fixed seed, so the device stages exactly the planted list and keeps
exactly the case's nk matches (tests/test_two_view_refine_reference.py asserts that of the twin for every case, without a GPU).

    sized(n)        n noisy inliers, no outliers: the kept sizes 15, 63, 64, 65, 255, 256, 257, 513 sit on both sides of the strides
                    of the 256 partial sums (an empty partial, one full stride, one match into the second and the third stride) and 14
                    is one short of min_matches.  The seeds are the first from 700 + n for which the RANSAC keeps all n.
    noise_free()    the pair starts at the minimum.
    short_baseline()  the baseline is 1e-4 of the depth: the translation block of the normal system is near-singular.
"""
import numpy as np

import two_view_fixtures as tvf
from monocularsfm_amd import synth

F32 = np.float32
CAM = tvf.CAM
NOISE = 0.7
SIZES = (15, 63, 64, 65, 255, 256, 257, 513)
SIZED_SEEDS = {14: 714, 15: 715, 63: 763, 64: 764, 65: 765, 255: 957, 256: 958, 257: 961, 513: 1213}


def sized(n, seed=None):
    seed = SIZED_SEEDS[n] if seed is None else seed
    k1, k2, _, _ = synth.general_view_pair(n, 0, seed=seed, noise_px=NOISE)
    return tvf.case("sized-%d" % n, k1, k2, seed, n)


def noise_free(n=120, seed=1301):
    k1, k2, _, _ = synth.general_view_pair(n, 0, seed=seed, noise_px=0.0)
    return tvf.case("noise-free", k1, k2, seed, n)


def short_baseline(n=120, seed=1302, ratio=1e-4):
    """camera 2 = camera 1 turned by 20 mrad about y and moved sideways by ratio x the scene's depth"""
    rng = np.random.default_rng(seed)
    f, cx, cy = CAM[0], CAM[2], CAM[3]
    depth = 6.0
    c, s = np.cos(0.02), np.sin(0.02)
    R2 = np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]])
    cams = [(np.eye(3), np.array([0.0, 0.0, depth]), f, cx, cy), (R2, np.array([ratio * depth, 0.0, depth]), f, cx, cy)]
    X = np.stack([rng.uniform(-1.6, 1.6, n), rng.uniform(-1.1, 1.1, n), rng.uniform(-1.0, 1.0, n)], 1)
    k1, k2 = synth.keypoints(n, seed=seed + 1), synth.keypoints(n, seed=seed + 2)
    for k, cam in ((k1, cams[0]), (k2, cams[1])):
        p, z = tvf.project(cam, X)
        assert z.min() > 0
        k[:, :2] = (p + rng.normal(0, NOISE, p.shape)).astype(F32)
    return tvf.case("short-baseline", k1, k2, seed, n, cams=cams)


def exact_pair(n=120, seed=1303, rotation_only=False):
    """A pair for the host twin alone, which takes normalised fp64 coordinates: the exact fp64 projections of n scene points through two
    synth.scene_cameras and a record at the TRUE relative pose with every match counted in front and triangulated -- a start AT the
    minimum (the residuals are rounding, ~1e-13 px).  rotation_only: both cameras share their centre, so every translation direction
    explains the matches, nothing triangulates and the cost is rounding noise: no step can stand.
    -> (record fields as a dict, q1, q2 [n x 2 float64])"""
    (R1, t1, _, _, _), (R2, t2, _, _, _) = synth.scene_cameras(2, seed=seed)
    if rotation_only:
        t2 = R2 @ R1.T @ t1
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-1.6, 1.6, n), rng.uniform(-1.1, 1.1, n), rng.uniform(-1.0, 1.0, n)], 1)
    Y1, Y2 = X @ R1.T + t1, X @ R2.T + t2
    R = R2 @ R1.T
    t = t2 - R @ t1
    t = np.array([1.0, 0.0, 0.0]) if rotation_only else t / np.linalg.norm(t)
    rec = dict(valid=1, R=R.reshape(9), t=t, n_kept=n, n_positive_depth=n, n_triangulated=n)
    return rec, Y1[:, :2] / Y1[:, 2:], Y2[:, :2] / Y2[:, 2:]


def edge_cases():
    return [sized(n) for n in (14,) + SIZES] + [noise_free(), short_baseline()]


def planted(case):
    """the case's planted correspondences as pixel points, in staged order -> (p1, p2), n x 2 float32 each"""
    dA, kA, dB, kB = case["scene"]
    qt = case["qt"]
    return kA[qt[:, 0], :2], kB[qt[:, 1], :2]
