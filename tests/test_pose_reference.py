"""The two-view geometry's host twin (csrc/msfm_pose.h through libmsfm_host.so, tests/pose_twin.py) against an independent fp64
numpy reference (tests/pose_ref.py: np.linalg.svd decomposition and DLT, math.acos, a sorted median, plain sums).  CPU only.

Tolerances of the doubles.  The reference is measured against ITSELF in np.longdouble on the same inputs (SCATTER below collects,
per quantity, the largest |fp64 reference - longdouble reference| the tests see: the reference's own rounding scatter, independent of
the code under test); the twin is allowed 16 x that (its operation order differs from LAPACK's, each within a few ulp of the
conditioning).  Measured on the seeds below (x86-64, longdouble = 80-bit): scatter R 5.5e-16, t 4.1e-16 -> bounds 8.8e-15, 6.6e-15;
the twin's largest differences were R 6.7e-16, t 3.3e-16.  The statistics' scatter is largest at the near-zero baselines (0.02 and
0.002 of the scene's), where the DLT's two smallest singular values nearly coincide: median angle 2.6e-11 deg, mean angle 7.3e-12
deg, mean residual 1.7e-14 px (bounds 16 x those); the twin differed from the fp64 reference by 1.9e-11 deg, 1.2e-11 deg and
2.0e-14 px at most.  (Until the longdouble DLT refinement of pose_ref.py learnt to step past a shifted matrix that is singular to
working precision, the matches it gave up on set these scatters: 5.3e-2 deg, 8.0e-5 deg, 1.1e-3 px, a thousand million times wider.)

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
import two_view_fixtures as tvf
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


# ---- the scenes of tests/two_view_fixtures.py: the edges of tv_pose_kernel (tests/test_gpu_two_view_geometry.py runs them on the
# device; here, without a GPU, that every scene reaches the edge it is named for, and the twin against the reference on them) ------

@pytest.fixture(scope="module")
def edge_cases():
    cases = tvf.exact_sizes() + tvf.staged_vs_kept() + tvf.tied_angles() + [tvf.depth_spread()]
    return {c["name"]: c for c in cases}


def planted_points(c):
    (_, kA, _, kB), qt = c["scene"], c["qt"]
    return kA[qt[:, 0], :2], kB[qt[:, 1], :2]


def test_edge_fixtures_reach_their_edges(host, oracle, edge_cases):
    """Every case of two_view_fixtures: the CPU oracle's match list is the planted one (ascending query row), the twin keeps the
    stated nk and rejects the stated positions, the record is valid; the tie cases' middle ranks are equal or distinct as intended;
    the spread case's keys differ in their upper bytes."""
    assert [edge_cases["exact-%d" % n]["nk"] for n in tvf.EXACT_SIZES] == list(tvf.EXACT_SIZES)
    assert sorted((c["n"], c["nk"]) for c in edge_cases.values() if c["name"].startswith("staged")) == \
        [(65, 63), (129, 64), (300, 256), (300, 257), (600, 512), (600, 513)]
    angles = {}
    for name, c in edge_cases.items():
        dA, _, dB, _ = c["scene"]
        q, t, _ = oracle.match_pair(dA, dB)
        assert np.array_equal(np.stack([q, t], 1), c["qt"]) and np.all(np.diff(q) > 0), name
        p1, p2 = planted_points(c)
        mask, rec = pose_twin.geometry(host, p1, p2, tvf.CAM)
        assert len(mask) == c["n"] and int(mask.sum()) == c["nk"] == rec["n_kept"], (name, int(mask.sum()))
        assert np.array_equal(np.nonzero(~mask)[0], c["rejected"]), name
        assert rec["valid"] == 1, name
        if not name.startswith("depth"):
            assert rec["n_triangulated"] == c["nk"], name
        angles[name] = pose_twin.kept_angles(host, rec, p1[mask], p2[mask], tvf.CAM)
        assert rec["median_tri_angle"] == pose_twin.median_rule(angles[name]), name
    # the rejected positions the kept list's ballot needs: both sides of a 64-boundary, a whole 64-chunk, the last staged match
    rej = {name: set(c["rejected"].tolist()) for name, c in edge_cases.items()}
    assert any({63, 64} <= r for r in rej.values())
    assert any(set(range(64 * k, 64 * k + 64)) <= r and 0 < 64 * k < c["n"] - 64
               for c in edge_cases.values() for r in [rej[c["name"]]] for k in range(c["n"] // 64))
    assert any(c["n"] - 1 in rej[c["name"]] for c in edge_cases.values())
    # ties: D runs of c equal angles; the two middle ranks of the even cases
    middle = {}
    for d, k in tvf.TIED:
        a = sorted(angles["tied-%dx%d" % (d, k)])
        values, counts = np.unique(a, return_counts=True)
        assert len(values) == d and set(counts.tolist()) == {k}
        n = d * k
        if n % 2 == 0:
            middle[(d, k)] = a[(n - 1) // 2] == a[n // 2]
    assert middle == {(8, 40): False, (6, 43): False, (16, 16): False, (7, 40): True}
    # spread: angles over more than five decades, the keys' two upper bytes take many values, the median well inside the range
    a = np.sort(np.asarray(angles["depth-spread"]))
    assert a[0] > 0 and a[-1] > 10.0 and a[-1] / a[0] > 1e5
    assert len(set((a.view(np.uint64) >> np.uint64(48)).tolist())) >= 16
    assert 100 * a[0] < pose_twin.median_rule(a) < a[-1] / 100


def test_walk_job_layout(host, oracle):
    """two_view_fixtures.walk_job for a grid of 256 workgroups: the own-scene pairs lie in every third of the list, the twin finds
    them valid and the cross pairs invalid, and workgroups walk valid / invalid / valid as well as invalid / valid / invalid."""
    cu = 256
    job = tvf.walk_job(cu)
    pairs, own = job["pairs"], job["own"]
    assert len(pairs) == 3 * cu + 7 and len(own) == 48
    images, kps = {}, {}
    for s, (dA, kA, dB, kB, _) in enumerate(job["scenes"]):
        images[2 * s], images[2 * s + 1], kps[2 * s], kps[2 * s + 1] = dA, dB, kA, kB
        assert max(len(dA), len(dB)) < 400
    offs, q, t, _ = oracle.match_pairs(images, pairs)
    valid = np.zeros(len(pairs), bool)
    for p, (i, j) in enumerate(pairs):
        s, e = offs[p], offs[p + 1]
        valid[p] = pose_twin.geometry(host, kps[i][q[s:e], :2], kps[j][t[s:e], :2], tvf.CAM)[1]["valid"] == 1
    is_own = np.zeros(len(pairs), bool)
    is_own[own] = True
    cross = ~is_own
    cross[job["staged_only"]] = False
    assert np.array_equal(pairs[is_own, 0] // 2, pairs[is_own, 1] // 2) and not np.any(pairs[cross, 0] // 2 == pairs[cross, 1] // 2)
    assert sorted(set(np.diff(offs)[job["staged_only"]].tolist())) == [3, 4] and len(job["staged_only"]) == 16
    assert len({tuple(p) for p in pairs[is_own]}) == 48
    assert np.array_equal(valid, is_own)
    assert all(valid[k * cu:(k + 1) * cu].sum() >= 8 for k in range(3))
    walks = {tuple(valid[b::cu][:3]) for b in range(cu)}
    assert {(True, False, True), (False, True, False), (False, False, False)} <= walks


EDGE_REFERENCE = ["tied-%dx%d" % dc for dc in tvf.TIED] + ["exact-63", "exact-256", "exact-769"], ["depth-spread"]


def reference_on(host, c, params=pose_twin.DEFAULTS):
    """The twin's record function and the reference (fp64 and longdouble) on the case's kept matches and the E of its true pose."""
    p1, p2 = planted_points(c)
    mask, _ = pose_twin.geometry(host, p1, p2, tvf.CAM)
    q1, q2 = normalised(p1[mask]), normalised(p2[mask])
    R0, t0 = true_pose(c["cams"])
    E = emat_ref.essential_from_pose(R0, t0 / np.linalg.norm(t0))
    E /= np.linalg.norm(E)
    kw = dict(min_num_inliers=params[0], tri_max_error=params[1], tri_min_angle=params[2])
    got, w = pose_twin.record(host, E, q1, q2, F, params)
    return got, w, pose_ref.record(E, q1, q2, F, **kw), pose_ref.record(E, q1, q2, F, dtype=np.longdouble, **kw), (E, q1, q2)


DOUBLES = (("R", "R"), ("t", "t"), ("median", "median_tri_angle"), ("mean_angle", "mean_tri_angle"), ("mean_residual", "mean_residual"))


def compare_with_reference(got, w, want, ext, scatter, worst, tri_max_error=2.0):
    """Winner, counts and verdict equal (nothing at a threshold: asserted, so no match is left out); the doubles' differences and
    the reference's own scatter are collected."""
    assert want["valid"] == 1 and got["valid"] == 1
    for per in want["per_candidate"]:
        for _, err, _, (z1, z2) in per:
            assert not (abs(err - tri_max_error) <= BAND * tri_max_error or abs(z1 - pose_ref.EPS) <= BAND * pose_ref.EPS or
                        abs(z2 - pose_ref.EPS) <= BAND * pose_ref.EPS)
    assert w == want["winner"] == ext["winner"]
    for key in ("n_kept", "n_positive_depth", "n_triangulated", "is_initial_candidate"):
        assert got[key] == want[key] == ext[key], key
    for key, field in DOUBLES:
        g = got[field].reshape(3, 3) if key == "R" else got[field]
        d = float(np.max(np.abs(np.asarray(want[field], np.longdouble) - np.asarray(ext[field], np.longdouble))))
        scatter[key] = max(scatter.get(key, 0.0), d)
        worst[key] = max(worst.get(key, 0.0), float(np.max(np.abs(np.asarray(g) - np.asarray(want[field], np.float64)))))


def test_edge_scenes_against_the_reference(host, edge_cases):
    """The twin against pose_ref on the tie scenes, three of the exact sizes and the depth spread: winner, counts and verdict equal
    with no match left out, the doubles within 16 x the reference's own longdouble scatter on the same inputs.  Two groups, each with
    its own scatter: the well-conditioned scenes together, and the depth spread alone (its far points are ill-conditioned and would
    widen the others' bounds).  Measured (x86-64, longdouble = 80-bit): well-conditioned scenes, scatter R 5.1e-16, t 1.7e-16, median
    1.5e-13 deg, mean angle 3.6e-14 deg, mean residual 4.0e-14 px; the twin's largest differences R 5.6e-16, t 2.2e-16, median
    1.3e-13, mean angle 5.3e-14, mean residual 5.0e-14.  Depth spread: scatter R 3.2e-16, t 1.4e-16, median 6.2e-12 deg, mean angle
    3.9e-11 deg, mean residual 7.4e-15 px; twin R 3.3e-16, t 2.2e-16, median 0, mean angle 8.6e-11, mean residual 5.3e-15.
    The tie scenes' medians are also compared exactly with the sorted per-match angles of the twin's own evaluate."""
    for group in EDGE_REFERENCE:
        scatter, worst = {}, {}
        for name in group:
            got, w, want, ext, (E, q1, q2) = reference_on(host, edge_cases[name])
            compare_with_reference(got, w, want, ext, scatter, worst)
            if name.startswith("tied"):
                R, t = pose_twin.decompose(host, E)[w]
                ang = [pose_twin.evaluate(host, R, t, F, *a, *b)[2] for a, b in zip(q1, q2)]
                assert len(set(ang)) == edge_cases[name]["distinct"]
                assert got["median_tri_angle"] == pose_twin.median_rule(ang)
                assert abs(want["median_tri_angle"] - got["median_tri_angle"]) < 1e-9
        print(group[0], "...: reference scatter", scatter, "twin against the reference", worst)
        for key in worst:
            assert worst[key] <= 16 * scatter[key], (group, key, worst[key], scatter[key])


def test_no_match_triangulated(host):
    """tri_max_error = 0: no match counts as triangulated, both means are exactly 0 and the median is computed all the same."""
    k1, k2, cams = view_pair(100, 0, 31, noise_px=0.3)
    c = dict(scene=(None, k1, None, k2), qt=np.stack([np.arange(100)] * 2, 1), cams=cams)
    scatter, worst = {}, {}
    got, w, want, ext, _ = reference_on(host, c, params=(100, 0.0, 4.0))
    assert got["n_kept"] == 100
    # (no error lies within BAND of 0: every match's error is positive)
    assert min(m[1] for m in want["per_match"]) > 0
    compare_with_reference(got, w, want, ext, scatter, worst, tri_max_error=0.0)
    assert got["n_triangulated"] == 0 and got["n_positive_depth"] > 0 and got["is_initial_candidate"] == 0
    assert got["mean_tri_angle"] == 0.0 == want["mean_tri_angle"] and got["mean_residual"] == 0.0 == want["mean_residual"]
    assert got["median_tri_angle"] > 1.0
    for key in worst:
        assert worst[key] <= 16 * scatter[key], (key, worst[key], scatter[key])
    # the whole twin: the same verdict, and apart from the triangulated statistics the record of the default parameters
    mask, rec0 = pose_twin.geometry(host, k1[:, :2], k2[:, :2], CAM[:4], params=(100, 0.0, 4.0))
    _, rec = pose_twin.geometry(host, k1[:, :2], k2[:, :2], CAM[:4])
    assert rec0["valid"] == 1 and rec0["n_triangulated"] == 0 and rec0["mean_tri_angle"] == 0.0 and rec0["mean_residual"] == 0.0
    assert rec0["median_tri_angle"] == rec["median_tri_angle"] != 0.0 and rec["n_triangulated"] > 0
    assert rec0["is_initial_candidate"] == 0 and rec0["R"].tobytes() == rec["R"].tobytes()
