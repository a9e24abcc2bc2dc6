"""The two-view geometry's host twin (csrc/msfm_pose.h through libmsfm_host.so, tests/pose_twin.py) against an independent fp64
numpy reference (tests/pose_ref.py: np.linalg.svd decomposition and DLT, math.acos, a sorted median, plain sums).  CPU only.

Tolerances of the doubles.  The reference is measured against ITSELF in np.longdouble on the same inputs (SCATTER below collects,
per quantity, the largest |fp64 reference - longdouble reference| the tests see: the reference's own rounding scatter, independent of
the code under test); the twin is allowed 16 x that (its operation order differs from LAPACK's, each within a few ulp of the
conditioning).  Measured on the seeds below (x86-64, longdouble = 80-bit): scatter R 5.5e-16, t 4.1e-16 -> bounds 8.8e-15, 6.6e-15;
the twin's largest differences were R 6.7e-16, t 3.3e-16.  The statistics' scatter is set by the near-zero baselines (0.02 and 0.002
of the scene's), where the DLT's two smallest singular values nearly coincide and the reference's own point moves with its
rounding: median angle 5.3e-2 deg, mean angle 8.0e-5 deg, mean residual 1.1e-3 px (bounds 16 x those); the twin differed from the
fp64 reference by 1.9e-11 deg, 1.2e-11 deg and 2.0e-14 px at most, i.e. far inside them.

Counts.  winner, n_positive_depth and n_triangulated must EQUAL the reference's after leaving out the matches whose reference error
lies within BAND (relative) of tri_max_error or whose reference depth within BAND of the depth threshold under any candidate; at most
0.1 % of a test's matches may be left out (the seeds below leave out none: asserted)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import emat_ref
import pose_ref
import pose_twin
from monocularsfm_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = (2500.0, 2500.0, 1536.0, 1152.0, 0.0, 0.0, 0.0, 0.0)
F = 2500.0
BAND = 1e-9
SCATTER = {}


@pytest.fixture(scope="module")
def host():
    return pose_twin.load_host()


def note(key, a, b):
    d = float(np.max(np.abs(np.asarray(a, np.longdouble) - np.asarray(b, np.longdouble))))
    SCATTER[key] = max(SCATTER.get(key, 0.0), d)
    return d


def true_pose(cams):
    (R1, t1, *_), (R2, t2, *_) = cams
    R = R2 @ R1.T
    t = t2 - R @ t1
    return R, t


def view_pair(n_in, n_out, seed, baseline=1.0, noise_px=0.5):
    """synth.general_view_pair with the second camera moved towards the first: baseline 1 is general_view_pair itself, 0 the
    same centre and orientation blended alike (a near-zero baseline)."""
    cams = synth.scene_cameras(2, seed=seed)
    if baseline != 1.0:
        (R1, t1, f, cx, cy), (R2, t2, _, _, _) = cams
        c1, c2 = -R1.T @ t1, -R2.T @ t2
        c = c1 + baseline * (c2 - c1)
        cams = [cams[0], (R2, -R2 @ c, f, cx, cy)]
    ids = np.r_[np.arange(n_in), np.full(n_out, -1)]
    k1, k2 = synth.scene_keypoints([ids, ids], cams, max(n_in, 1), seed=seed, noise_px=noise_px)
    return k1, k2, cams


def normalised(p):
    return np.array([emat_ref.undistort(CAM, float(u), float(v)) for u, v in p]).reshape(-1, 2)


def as_set(cands):
    return sorted((tuple(np.round(np.r_[R.ravel(), t], 9)) for R, t in cands))


def rotation_angle(Ra, Rb):
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(Ra.T @ Rb) - 1) / 2))))


def test_acos(host):
    x = np.r_[np.linspace(-1.0, 1.0, 400001), [-1.0, 1.0, 0.5, -0.5, np.nextafter(0.5, 1), np.nextafter(-0.5, -1),
                                               np.nextafter(1.0, 0), np.nextafter(-1.0, 0), 0.0, 1e-300, -1e-300]]
    got = pose_twin.acos(host, x)
    worst = max(abs(float(g) - math.acos(float(v))) for g, v in zip(got, x))
    print("acos: largest absolute error %.3g rad" % worst)
    assert worst <= 1e-12
    out = pose_twin.acos(host, np.array([1.0000000000000002, -1.0000000000000002, 2.0, float("nan")]))
    assert np.all(np.isnan(out))   # outside [-1, 1]: NaN, as std::acos (the angle becomes 0)


def test_decomposition_candidates(host):
    rng = np.random.default_rng(7)
    Es = []
    for _ in range(40):
        R = synth._rotation(rng, rng.uniform(0.05, 1.5))
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        E = emat_ref.essential_from_pose(R, t) * rng.choice([-1.0, 1.0])
        Es.append((E / np.linalg.norm(E), R, t))
    for E, R, t in Es:
        got, want, ext = pose_twin.decompose(host, E), pose_ref.decompose(E), pose_ref.decompose(E, np.longdouble)
        assert as_set(got) == as_set(want)
        for (Rg, tg), (Rw, tw), (Rx, tx) in zip(got, want, ext):      # and in the stated order
            sr, st = note("R", Rw, Rx), note("t", tw, tx)
            assert np.abs(Rg - Rw).max() <= 16 * max(SCATTER["R"], sr) and np.abs(tg - tw).max() <= 16 * max(SCATTER["t"], st)
            assert abs(np.linalg.det(Rg) - 1) < 1e-13 and abs(np.linalg.norm(tg) - 1) < 1e-13
        assert np.trace(got[0][0]) >= np.trace(got[2][0]) and got[0][1][np.argmax(np.abs(got[0][1]))] > 0
        # the true pose is one of the four
        assert min(rotation_angle(Rg, R) + np.degrees(np.arccos(np.clip(tg @ t, -1, 1))) for Rg, tg in got) < 1e-5


def ransac_winner(k1, k2):
    """The E the reference RANSAC (emat_ref.ransac) ends with: the hypothesis whose best solution gives the returned mask,
    re-solved.  -> (E, mask as bool)"""
    rmask = emat_ref.ransac(CAM, k1[:, :2], k2[:, :2])
    assert rmask is not None
    q1, q2 = normalised(k1[:, :2]), normalised(k2[:, :2])
    score = emat_ref.scorer(CAM, k1[:, :2], k2[:, :2])
    thr2 = (3.0 / F) ** 2
    for it in range(1000):
        c, m = score(it)
        if m is not None and np.array_equal(m.astype(np.uint8), rmask):
            idx = emat_ref.sample5(0x5EED5EED, it, len(q1))
            sols, _ = emat_ref.five_point(q1[idx], q2[idx])
            return max(sols, key=lambda E: sum(emat_ref.sampson(E, *q1[i], *q2[i]) <= thr2 for i in range(len(q1)))), rmask.astype(bool)
    raise AssertionError("the winner of emat_ref.ransac was not found again")


def test_decomposition_of_ransac_winners(host):
    for seed in (1, 2, 3, 4):
        k1, k2, _ = view_pair(60, 15, seed)
        E, _ = ransac_winner(k1, k2)
        got, want = pose_twin.decompose(host, E), pose_ref.decompose(E)
        assert got is not None and as_set(got) == as_set(want)


def test_median_rule_exactly(host):
    """The reference's median through the twin's record, compared exactly: an odd and an even kept list whose angles are all
    different, against the sorted per-match angles of the twin's own evaluate."""
    k1, k2, cams = view_pair(41, 0, 21, noise_px=0.2)
    R0, t0 = true_pose(cams)
    E = emat_ref.essential_from_pose(R0, t0 / np.linalg.norm(t0))
    E /= np.linalg.norm(E)
    q1, q2 = normalised(k1[:, :2]), normalised(k2[:, :2])
    for n in (41, 40, 7, 6, 5, 2, 1):
        rec, w = pose_twin.record(host, E, q1[:n], q2[:n], F)
        assert rec["valid"] == 1
        R, t = pose_twin.decompose(host, E)[w]
        ang = sorted(pose_twin.evaluate(host, R, t, F, *q1[i], *q2[i])[2] for i in range(n))
        assert len(set(ang)) == n
        want = ang[n // 2] if n % 2 else (ang[(n - 1) // 2] + ang[n // 2]) / 2
        assert rec["median_tri_angle"] == want
        ref = pose_ref.record(E, q1[:n], q2[:n], F)
        assert abs(ref["median_tri_angle"] - want) < 1e-9


CASES = [(seed, b) for seed in (11, 12, 13, 14) for b in (1.0, 0.3, 0.02, 0.002)]


def test_whole_record_against_the_reference(host):
    """Winner and counts equal, doubles within 16 x the reference's own scatter; both verdicts of the rule occur."""
    verdicts, left_out, total = set(), 0, 0
    worst = {}
    for seed, baseline in CASES:
        k1, k2, cams = view_pair(260, 50, seed, baseline)
        mask, rec = pose_twin.geometry(host, k1[:, :2], k2[:, :2], CAM[:4])
        assert mask.sum() >= 5
        q1, q2 = normalised(k1[mask, :2]), normalised(k2[mask, :2])
        # the twin's own winning E is not exported: the reference takes the E of the true pose's RANSAC-independent record below, and
        # the twin's record function is compared on the same E
        R0, t0 = true_pose(cams)
        E = emat_ref.essential_from_pose(R0, t0 / max(np.linalg.norm(t0), 1e-300))
        if not np.linalg.norm(E) > 1e-6:
            E = emat_ref.essential_from_pose(R0, np.array([1.0, 0.0, 0.0]))
        E /= np.linalg.norm(E)
        want = pose_ref.record(E, q1, q2, F)
        ext = pose_ref.record(E, q1, q2, F, dtype=np.longdouble)
        got, w = pose_twin.record(host, E, q1, q2, F)
        total += len(q1)
        assert want["valid"] == 1 and got["valid"] == 1
        # matches at a threshold, by the reference alone
        edge = np.zeros(len(q1), bool)
        for per in want["per_candidate"]:
            for i, (_, err, _, (z1, z2)) in enumerate(per):
                edge[i] |= abs(err - 2.0) <= BAND * 2.0 or abs(z1 - pose_ref.EPS) <= BAND * pose_ref.EPS or abs(z2 - pose_ref.EPS) <= BAND * pose_ref.EPS
        left_out += int(edge.sum())
        assert not edge.any()       # (these seeds: nothing at an edge, so the counts compare whole)
        assert w == want["winner"] == ext["winner"]
        assert got["n_kept"] == len(q1) and got["n_positive_depth"] == want["n_positive_depth"] and got["n_triangulated"] == want["n_triangulated"]
        assert got["is_initial_candidate"] == want["is_initial_candidate"]
        verdicts.add(int(got["is_initial_candidate"]))
        for key, g, a, b in (("R", got["R"].reshape(3, 3), want["R"], ext["R"]), ("t", got["t"], want["t"], ext["t"]),
                             ("median", got["median_tri_angle"], want["median_tri_angle"], ext["median_tri_angle"]),
                             ("mean_angle", got["mean_tri_angle"], want["mean_tri_angle"], ext["mean_tri_angle"]),
                             ("mean_residual", got["mean_residual"], want["mean_residual"], ext["mean_residual"])):
            note(key, a, b)
            worst[key] = max(worst.get(key, 0.0), float(np.max(np.abs(np.asarray(g) - np.asarray(a, np.float64)))))
    print("reference scatter (fp64 against longdouble):", SCATTER)
    print("twin against the reference:", worst)
    assert left_out <= 0.001 * total
    assert verdicts == {0, 1}
    for key in worst:
        assert worst[key] <= 16 * SCATTER[key], (key, worst[key], SCATTER[key])


def test_pose_against_the_truth(host):
    """The whole twin (its own RANSAC winner) against synth.scene_cameras' true relative pose: no worse than 2 x the reference's error
    on the same kept matches (both fit the same noisy data; this guards against a wrong candidate or a transposed R)."""
    for seed in (11, 12, 13, 14, 15):
        k1, k2, cams = view_pair(260, 50, seed)
        R0, t0 = true_pose(cams)
        t0 = t0 / np.linalg.norm(t0)
        mask, rec = pose_twin.geometry(host, k1[:, :2], k2[:, :2], CAM[:4])
        assert rec["valid"] == 1 and rec["n_kept"] == mask.sum()
        # the reference on the same data: its own RANSAC (tests/emat_ref.py), the winner re-solved, np.linalg.svd pose
        rmask = emat_ref.ransac(CAM, k1[:, :2], k2[:, :2])
        assert rmask is not None
        q1, q2 = normalised(k1[:, :2]), normalised(k2[:, :2])
        score = emat_ref.scorer(CAM, k1[:, :2], k2[:, :2])
        best = None
        for it in range(64):
            c, m = score(it)
            if m is not None and np.array_equal(m.astype(np.uint8), rmask):
                idx = emat_ref.sample5(0x5EED5EED, it, len(q1))
                sols, _ = emat_ref.five_point(q1[idx], q2[idx])
                thr2 = (3.0 / F) ** 2
                best = max(sols, key=lambda E: sum(emat_ref.sampson(E, *q1[i], *q2[i]) <= thr2 for i in range(len(q1))))
                break
        assert best is not None
        want = pose_ref.record(best, q1[rmask.astype(bool)], q2[rmask.astype(bool)], F)
        ref_rot, ref_dir = rotation_angle(want["R"], R0), math.degrees(math.acos(min(1.0, float(want["t"] @ t0))))
        got_rot = rotation_angle(rec["R"].reshape(3, 3), R0)
        got_dir = math.degrees(math.acos(max(-1.0, min(1.0, float(rec["t"] @ t0)))))
        print("seed %d: rotation error %.4f (reference %.4f) deg, direction error %.4f (reference %.4f) deg" % (seed, got_rot, ref_rot, got_dir, ref_dir))
        assert got_rot <= 2 * ref_rot and got_dir <= 2 * ref_dir


def finite_record(rec):
    return all(np.all(np.isfinite(rec[k])) for k in ("R", "t", "median_tri_angle", "mean_tri_angle", "mean_residual"))


def test_degenerate_inputs(host):
    zero = np.zeros(1, pose_twin.RECORD)[0]
    # nE < 5
    k1, k2, _ = view_pair(4, 0, 3)
    mask, rec = pose_twin.geometry(host, k1[:, :2], k2[:, :2], CAM[:4])
    assert not mask.any() and rec.tobytes() == zero.tobytes()
    # pure rotation: E is degenerate, whatever the RANSAC keeps gives a finite record
    k1, k2, _, _ = synth.rotation_view_pair(200, 40, seed=5)
    mask, rec = pose_twin.geometry(host, k1[:, :2], k2[:, :2], CAM[:4])
    assert finite_record(rec) and (rec["valid"] == 1 or rec.tobytes() == zero.tobytes())
    if rec["valid"]:
        assert rec["median_tri_angle"] < 4.0 and rec["is_initial_candidate"] == 0
    # all matches identical
    k = np.tile(np.array([[1000.0, 900.0, 1.0, 0.0]], np.float32), (30, 1))
    mask, rec = pose_twin.geometry(host, k[:, :2], k[:, :2], CAM[:4])
    assert finite_record(rec) and rec["is_initial_candidate"] == 0
    E = emat_ref.essential_from_pose(np.eye(3), np.array([1.0, 0.0, 0.0]))
    q = np.tile([[0.1, -0.2]], (30, 1))
    rec, w = pose_twin.record(host, E / np.linalg.norm(E), q, q, F)
    assert finite_record(rec) and rec["is_initial_candidate"] == 0
    # E = 0, NaN: no decomposition
    for bad in (np.zeros((3, 3)), np.full((3, 3), np.nan), np.outer([1.0, 0, 0], [0, 1.0, 0])):
        rec, w = pose_twin.record(host, bad, q, q, F)
        assert w == -1 and rec.tobytes() == zero.tobytes()
    # t along the optical axis
    rng = np.random.default_rng(9)
    X = np.c_[rng.uniform(-1, 1, 80), rng.uniform(-1, 1, 80), rng.uniform(4, 6, 80)]
    t = np.array([0.0, 0.0, 1.0])
    q1, q2 = X[:, :2] / X[:, 2:], (X + t)[:, :2] / (X + t)[:, 2:]
    E = emat_ref.essential_from_pose(np.eye(3), t)
    rec, w = pose_twin.record(host, E / np.linalg.norm(E), q1, q2, F)
    want = pose_ref.record(E / np.linalg.norm(E), q1, q2, F)
    assert rec["valid"] == 1 and finite_record(rec) and w == want["winner"] and rec["n_positive_depth"] == 80
    assert np.abs(rec["t"] - t).max() < 1e-12 and np.abs(rec["R"].reshape(3, 3) - np.eye(3)).max() < 1e-12


def test_rule_edges(tmp_path):
    """msfm_initial_candidate (csrc/msfm_hostutil.h) at its edges, through a g++-built program."""
    src = tmp_path / "rule.cpp"
    src.write_text(r'''
#include <cmath>
#include <cstdio>
#include "msfm_hostutil.h"
int main() {
    const double up = std::nextafter(4.0, 5.0), down = std::nextafter(4.0, 3.0), e_up = std::nextafter(2.0, 3.0);
    int bad = 0;
    bad += !msfm_initial_candidate(100, 4.0, 4.0, 2.0, 100, 2.0, 4.0);      // every test at equality passes
    bad += msfm_initial_candidate(99, 4.0, 4.0, 2.0, 100, 2.0, 4.0);
    bad += msfm_initial_candidate(100, down, 4.0, 2.0, 100, 2.0, 4.0);
    bad += msfm_initial_candidate(100, 4.0, down, 2.0, 100, 2.0, 4.0);
    bad += msfm_initial_candidate(100, 4.0, 4.0, e_up, 100, 2.0, 4.0);
    bad += !msfm_initial_candidate(101, up, up, 0.0, 100, 2.0, 4.0);
    bad += !msfm_initial_candidate(0, 0.0, 0.0, 0.0, 0, 0.0, 0.0);
    bad += msfm_initial_candidate(100, NAN, 4.0, 2.0, 100, 2.0, 4.0);       // NaN never passes (the records hold none)
    bad += msfm_initial_candidate(100, 4.0, 4.0, NAN, 100, 2.0, 4.0);
    bad += msfm_pair_two_view_bytes(0, 10) != 0 || msfm_pair_two_view_bytes(1000, 10) != 12148;
    bad += msfm_pair_scratch_bytes(700, 650, 1024, 1024, 6, 2, 1, true) - msfm_pair_scratch_bytes(700, 650, 1024, 1024, 6, 2, 1) != 12 * 700 + 148;
    bad += msfm_pair_scratch_bytes(700, 650, 1024, 1024, 6, 2, 1, false) != msfm_pair_scratch_bytes(700, 650, 1024, 1024, 6, 2, 1);
    std::printf("%d\n", bad);
    return bad;
}
''')
    exe = tmp_path / "rule"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "monocularsfm_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout.strip() == "0"


def test_host_rule_export(host):
    assert host.host_initial_candidate(100, 4.0, 4.0, 2.0, 100, 2.0, 4.0) == 1
    assert host.host_initial_candidate(99, 4.0, 4.0, 2.0, 100, 2.0, 4.0) == 0


def test_abi_lists_the_entry_points():
    from monocularsfm_amd import _lib
    assert "msfm_set_two_view_geometry" in _lib.EXPORTS and "msfm_fetch_two_view_geometry" in _lib.EXPORTS
    assert _lib.TWO_VIEW_RECORD.itemsize == 144 == pose_twin.RECORD.itemsize
    header = open(os.path.join(ROOT, "include", "msfm_match.h")).read()
    assert "msfm_set_two_view_geometry" in header and "msfm_fetch_two_view_geometry" in header
