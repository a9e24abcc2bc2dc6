"""The staging schedule of the staged E / H RANSAC on the CPU (no GPU): host_staged_schedule (host/HostTestApi.cpp) predicts, for
one pair, how many rounds the device runs it (the first round r whose replay over the counts min((r + 1) * kRound, max_iters) is
decided) and how many hypotheses it solves there (min(rounds * kRound, max_iters)).  tests/test_gpu_verify_scale.py predicts
verification_stats() from it, so here it is checked against the independent numpy references (tests/emat_ref.py,
tests/hmat_ref.py): their sequential loop over their own per-hypothesis counts reads hypotheses 0 .. L - 1, and a staged replay is
decided exactly when it has all of those -- rounds = ceil(L / kRound).  Small pairs at 90 %, 50 % and 25 % inliers, max_iters at
one below / at / one above each round size."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emat_ref  # noqa: E402
import hmat_ref  # noqa: E402

from monocularsfm_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "monocularsfm_amd", "host")
FP, DP = C.POINTER(C.c_float), C.POINTER(C.c_double)
CAM = (2500.0, 2500.0, 1536.0, 1152.0, 0.0, 0.0, 0.0, 0.0)   # synth's camera
ROUND = {1: 32, 2: 64}    # kVeRound (csrc/msfm_verify_e.hip.h), kVhRound (csrc/msfm_verify_h.hip.h)
SAMPLE = {1: 5, 2: 4}
MAX_ITERS = (1, 31, 32, 33, 63, 64, 65, 200)
INLIERS = {"90": (36, 4), "50": (20, 20), "25": (10, 30)}


@pytest.fixture(scope="module")
def host():
    subprocess.check_call(["make", "-C", HOST, "-s", "libmsfm_host.so"])
    L = C.CDLL(os.path.join(HOST, "libmsfm_host.so"))
    L.host_staged_schedule.argtypes = [C.c_int, FP, FP, C.c_int, DP, C.c_double, C.c_double, C.c_int, C.c_ulonglong,
                                       C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
    return L


def schedule(host, model, p1, p2, threshold=3.0, confidence=0.99, max_iters=1000, seed=0x5eed5eed):
    p1 = np.ascontiguousarray(p1, np.float32)
    p2 = np.ascontiguousarray(p2, np.float32)
    cam = np.asarray(CAM, np.float64)
    rounds, solved = C.c_int(), C.c_longlong()
    rc = host.host_staged_schedule(model, p1.ctypes.data_as(FP), p2.ctypes.data_as(FP), len(p1), cam.ctypes.data_as(DP), threshold,
                                   confidence, max_iters, seed, C.byref(rounds), C.byref(solved))
    assert rc == 0
    return rounds.value, solved.value


class LazyCounts:
    """The reference's count of hypothesis it, computed on first use and kept; `read` is one past the largest index read."""

    def __init__(self, count_at):
        self.count_at, self.memo, self.read = count_at, {}, 0

    def __getitem__(self, it):
        if it not in self.memo:
            self.memo[it] = self.count_at(it)[0]
        self.read = max(self.read, it + 1)
        return self.memo[it]


def reference_schedule(model, lazy, n, max_iters, confidence=0.99):
    if n < SAMPLE[model]:
        return 0, 0
    lazy.read = 0
    if model == 1:
        emat_ref.replay(lazy, n, max_iters, confidence)
    else:
        hmat_ref.sequential_replay(lazy, n, max_iters, confidence)
    rounds = max(1, -(-lazy.read // ROUND[model]))
    return rounds, min(rounds * ROUND[model], max_iters)


def view_pair(model, level, seed):
    n_in, n_out = INLIERS[level]
    gen = synth.general_view_pair if model == 1 else synth.planar_view_pair
    k1, k2, _, _ = gen(n_in, n_out, seed=seed, noise_px=0.5)
    return k1[:, :2], k2[:, :2]


@pytest.mark.parametrize("model", [1, 2])
@pytest.mark.parametrize("level", ["90", "50", "25"])
def test_schedule_equals_the_reference_loop(host, model, level):
    p1, p2 = view_pair(model, level, seed=400 + 10 * model + len(level) + int(level))
    n = len(p1)
    if model == 1:
        lazy = LazyCounts(emat_ref.scorer(CAM, p1.astype(np.float64), p2.astype(np.float64)))
    else:
        lazy = LazyCounts(hmat_ref.counter(p1, p2))
    seen = set()
    for max_iters in MAX_ITERS:
        got = schedule(host, model, p1, p2, max_iters=max_iters)
        want = reference_schedule(model, lazy, n, max_iters)
        assert got == want, (model, level, max_iters, got, want)
        assert got[0] == -(-got[1] // ROUND[model]) and 1 <= got[0] <= -(-max_iters // ROUND[model])
        seen.add(got[0])
    if level == "90":   # decided in round 0 whatever the bound
        assert seen == {1}, seen
    if level == "25":   # runs to max_iters: every round, the last one partial where max_iters is not a multiple of kRound
        assert all(schedule(host, model, p1, p2, max_iters=m) == (-(-m // ROUND[model]), m) for m in MAX_ITERS)


@pytest.mark.parametrize("model", [1, 2])
def test_schedule_of_tiny_pairs_and_other_models(host, model):
    """n below the sample size: nothing runs (0, 0); at the sample size the pair runs.  Models other than 1 and 2 are refused."""
    k1, k2, _, _ = synth.planar_view_pair(8, 0, seed=77, noise_px=0.3)
    for n in range(0, 8):
        got = schedule(host, model, k1[:n, :2], k2[:n, :2], max_iters=100)
        if n < SAMPLE[model]:
            assert got == (0, 0), (n, got)
        else:
            assert got[0] >= 1 and got[1] == min(got[0] * ROUND[model], 100), (n, got)
    cam = np.asarray(CAM, np.float64)
    r, s = C.c_int(7), C.c_longlong(7)
    p = np.ascontiguousarray(k1[:, :2], np.float32)
    for bad in (0, 3, -1):
        assert host.host_staged_schedule(bad, p.ctypes.data_as(FP), p.ctypes.data_as(FP), len(p), cam.ctypes.data_as(DP), 3.0, 0.99,
                                         100, 1, C.byref(r), C.byref(s)) == -1


@pytest.mark.parametrize("model", [1, 2])
def test_schedule_edges_of_the_parameters(host, model):
    """Seeds 0 and 2^64 - 1, threshold 0 (no hypothesis reaches the sample size: every round runs), a near-1 confidence."""
    p1, p2 = view_pair(model, "50", seed=500 + model)
    n = len(p1)
    for seed in (0, (1 << 64) - 1):
        if model == 1:
            lazy = LazyCounts(emat_ref.scorer(CAM, p1.astype(np.float64), p2.astype(np.float64), seed=seed))
        else:
            lazy = LazyCounts(hmat_ref.counter(p1, p2, seed=seed))
        for max_iters in (33, 65):
            assert schedule(host, model, p1, p2, max_iters=max_iters, seed=seed) == reference_schedule(model, lazy, n, max_iters)
    assert schedule(host, model, p1, p2, threshold=0.0, max_iters=65) == (-(-65 // ROUND[model]), 65)
    lazy = LazyCounts(emat_ref.scorer(CAM, p1.astype(np.float64), p2.astype(np.float64), threshold=1.0) if model == 1
                      else hmat_ref.counter(p1, p2, threshold=1.0))
    assert schedule(host, model, p1, p2, threshold=1.0, confidence=0.999999, max_iters=65) == \
        reference_schedule(model, lazy, n, 65, confidence=0.999999)
