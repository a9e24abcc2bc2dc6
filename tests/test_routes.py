"""The matching route of a sub-batch (msfm_route / msfm_scratch_route in monocularsfm_amd/csrc/msfm_hostutil.h), compiled here with g++.

Every route gives the same bits, so the GPU tests only see a wrong route decision when a profile counter happens to move.  This table
pins the decision itself at each of its edges: the compact / dense switch at ratio 0.95f, the fine-twin level 0.625, the quarter rule of
a mixed twin sub-batch, the mean of 2048 rows per twin pair, every knob value.  Each row gives the route, the pairs on the twins' sweep,
the `demoted_pairs` count and the scratch route code (0 - 4) MatchJob::build charges each pair with.  The expected values were worked
out by hand from the decision as it stood before it moved into one function (PrefilterLaunch::choose_routes, prepare_batch_images and
MatchJob::start / build), known oddities included:
  * `demoted_pairs` tests each pair's own n1 + n2 >= 2048, while the route takes the mean over the twin pairs;
  * with coarse twins every prefiltered non-byte pair is charged as scratch route 4, even one without twins.
MatchJob always prunes (flag 1); with the flag off a pair is charged as on the dense route, like the ratio above 0.95.
"""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "monocularsfm_amd", "csrc")

DRIVER = r"""
#include "msfm_hostutil.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
// one scenario per line: prefilter q8_route q8_direct q8_level prune ratio n_pairs, then per pair valid use a_u8 b_u8 a_twin b_twin n1 n2
// -> kind, the pairs on the twins' sweep, demoted_pairs, the scratch route code of each pair
int main() {
    const char* kinds[] = {"dense", "fp16", "i8", "q8_direct", "q8_mixed", "q8_refine"};
    std::string level, ratio;
    MsfmRouteKnobs k;
    int prune, n;
    while (std::cin >> k.prefilter >> k.q8_route >> k.q8_direct >> level >> prune >> ratio >> n) {
        k.q8_level = std::strtof(level.c_str(), nullptr);
        const float r = std::strtof(ratio.c_str(), nullptr);
        std::vector<MsfmRoutePair> pairs((size_t)n);
        for (MsfmRoutePair& q : pairs) {
            int v[6];
            for (int& x : v) std::cin >> x;
            std::cin >> q.n1 >> q.n2;
            q = MsfmRoutePair{v[0] != 0, v[1] != 0, v[2] != 0, v[3] != 0, v[4] != 0, v[5] != 0, q.n1, q.n2};
        }
        const MsfmRoute route = msfm_route(k, prune, r, pairs);
        if (route.twin.size() != pairs.size()) return 1;
        std::printf("%s ", kinds[route.kind]);
        for (char t : route.twin) std::printf("%d", (int)t);
        std::printf(" %lld", route.demoted_pairs);
        for (const MsfmRoutePair& q : pairs) std::printf(" %d", msfm_scratch_route(k, prune, r, q.use, q.a_is_u8, q.b_is_u8));
        std::printf("\n");
    }
    return 0;
}
"""


def f32(x):
    return float(np.float32(x))


def next_up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


R95 = f32(0.95)


# pairs: (valid, use, a_u8, b_u8, a_twin, b_twin, n1, n2)
def B(n1, n2, valid=1, use=1):   # two byte images
    return (valid, use, 1, 1, 0, 0, n1, n2)


def T(n1, n2, valid=1, use=1):   # two float images with twins
    return (valid, use, 0, 0, 1, 1, n1, n2)


def F(n1, n2, valid=1, use=1):   # two float images without twins
    return (valid, use, 0, 0, 0, 0, n1, n2)


def H(n1, n2):                   # a twin on one side only
    return (1, 1, 0, 0, 1, 0, n1, n2)


# name: (knobs (prefilter, q8_route, q8_direct, q8_level), (prune, ratio), pairs, (kind, twins, demoted, scratch codes))
K = (1, 1, 1, 0.5)          # the defaults, twins at level 0.5 (fine)
KC = (1, 1, 1, 0.75)        # coarse twins
P8 = (1, 0.8)
SCENARIOS = {
    # byte stores, and what one float pair does to them
    "bytes_all": (K, P8, [B(1000, 1000), B(500, 600)], ("i8", "00", 0, [3, 3])),
    "bytes_plus_float": (K, P8, [B(1000, 1000), F(1000, 1000)], ("fp16", "00", 1, [3, 1])),
    "bytes_plus_float_coarse_level": (KC, P8, [B(1000, 1000), F(1000, 1000)], ("fp16", "00", 1, [3, 4])),
    "no_prefiltered_pairs": (K, P8, [B(1000, 1000, use=0), F(800, 900, use=0)], ("i8", "00", 0, [0, 0])),
    # the compact / dense switch, the prune flag
    "ratio_095_bytes": (K, (1, R95), [B(1000, 1000)], ("i8", "0", 0, [3])),
    "ratio_above_095_bytes": (K, (1, next_up(R95)), [B(1000, 1000)], ("dense", "0", 0, [2])),
    "ratio_095_twins": (K, (1, R95), [T(1500, 1500)], ("q8_direct", "1", 0, [1])),
    "ratio_above_095_twins": (K, (1, next_up(R95)), [T(1500, 1500)], ("dense", "0", 0, [2])),
    "ratio_zero": (K, (1, 0.0), [B(1000, 1000)], ("dense", "0", 0, [2])),
    "prune_off": (K, (0, 0.8), [B(1000, 1000), T(1500, 1500)], ("dense", "00", 0, [2, 2])),
    # fine and coarse twins: the level edge 0.625, the q8_direct knob
    "fine_twins_all": (K, P8, [T(1500, 1500), T(1200, 1000)], ("q8_direct", "11", 0, [1, 1])),
    "coarse_twins_all": (KC, P8, [T(1500, 1500), T(1200, 1000)], ("q8_refine", "11", 0, [4, 4])),
    "level_0625": ((1, 1, 1, 0.625), P8, [T(1500, 1500)], ("q8_direct", "1", 0, [1])),
    "level_above_0625": ((1, 1, 1, next_up(0.625)), P8, [T(1500, 1500)], ("q8_refine", "1", 0, [4])),
    "q8_direct_0": ((1, 1, 0, 0.5), P8, [T(1500, 1500)], ("q8_refine", "1", 0, [4])),
    "q8_direct_2": ((1, 1, 2, 1.0), P8, [T(1500, 1500)], ("q8_direct", "1", 0, [1])),
    "level_zero": ((1, 1, 1, 0.0), P8, [F(1000, 1000)], ("fp16", "0", 0, [1])),
    "level_zero_q8_direct_0": ((1, 1, 0, 0.0), P8, [F(1000, 1000)], ("fp16", "0", 0, [1])),
    # mixed twin sub-batches: the quarter rule (mean rule satisfied), coarse twins, a twin on one side only
    "quarter_exact": (K, P8, [T(2048, 2048), F(6144, 6144)], ("q8_mixed", "10", 0, [1, 1])),
    "quarter_minus_one_row": (K, P8, [T(2048, 2047), F(6144, 6144)], ("fp16", "00", 1, [1, 1])),
    "mixed_coarse": (KC, P8, [T(1500, 1500), F(1000, 1000)], ("fp16", "00", 1, [4, 4])),
    "mixed_one_sided_twin": (K, P8, [T(1500, 1500), H(1500, 1500)], ("q8_mixed", "10", 0, [1, 1])),
    "mixed_no_twin_pair": (K, P8, [F(1500, 1500), H(1500, 1500)], ("fp16", "00", 0, [1, 1])),
    # the mean of 2048 rows per twin pair (q8_route 1), lifted by q8_route 2; demoted_pairs tests each pair on its own
    "mean_2048_one_pair": (K, P8, [T(1024, 1024)], ("q8_direct", "1", 0, [1])),
    "mean_2047_one_pair": (K, P8, [T(1024, 1023)], ("fp16", "0", 0, [1])),
    "mean_2048_two_pairs": (K, P8, [T(1500, 1500), T(548, 548)], ("q8_direct", "11", 0, [1, 1])),
    "mean_2048_minus_one_two_pairs": (K, P8, [T(1500, 1500), T(548, 547)], ("fp16", "00", 1, [1, 1])),
    "mean_2048_minus_one_coarse": (KC, P8, [T(1500, 1500), T(548, 547)], ("fp16", "00", 1, [4, 4])),
    "q8_route_2_mean_2048": ((1, 2, 1, 0.5), P8, [T(1500, 1500), T(548, 548)], ("q8_direct", "11", 0, [1, 1])),
    "q8_route_2_mean_2047": ((1, 2, 1, 0.5), P8, [T(1024, 1023)], ("q8_direct", "1", 0, [1])),
    "q8_route_2_small_images": ((1, 2, 1, 0.5), P8, [T(50, 50), T(100, 60)], ("q8_direct", "11", 0, [1, 1])),
    "q8_route_1_small_images": (K, P8, [T(50, 50), T(100, 60)], ("fp16", "00", 0, [1, 1])),
    "q8_route_2_small_coarse_mixed": ((1, 2, 1, 0.75), P8, [T(50, 50), F(100, 100)], ("fp16", "00", 1, [4, 4])),
    "q8_route_1_small_coarse_mixed": (KC, P8, [T(50, 50), F(100, 100)], ("fp16", "00", 0, [4, 4])),
    # the knobs' other values
    "q8_route_0": ((1, 0, 1, 0.5), P8, [T(1500, 1500), B(1000, 1000)], ("fp16", "00", 1, [1, 3])),
    "q8_route_0_coarse_level": ((1, 0, 1, 0.75), P8, [T(1500, 1500)], ("fp16", "0", 0, [1])),
    "prefilter_0": ((0, 1, 1, 0.5), P8, [B(1000, 1000, use=0), T(1500, 1500, use=0)], ("fp16", "00", 0, [0, 0])),
    "prefilter_2_bytes": ((2, 1, 1, 0.5), P8, [B(1000, 1000)], ("fp16", "0", 0, [1])),
    "prefilter_2_coarse_twins": ((2, 1, 1, 0.75), P8, [T(1500, 1500)], ("fp16", "0", 0, [1])),
    "prefilter_2_dense": ((2, 1, 1, 0.5), (1, 0.96), [B(1000, 1000)], ("dense", "0", 0, [2])),
    # invalid and unused pairs are ignored
    "bytes_with_invalid_and_unused_float": (K, P8, [B(1000, 1000), F(0, 500, valid=0), F(1000, 1000, use=0)], ("i8", "000", 0, [3, 1, 0])),
    "twins_with_unused_float": (K, P8, [T(1500, 1500), F(1000, 1000, use=0)], ("q8_direct", "10", 0, [1, 0])),
    "twins_with_invalid_small_twin": (K, P8, [T(0, 100, valid=0), T(1500, 1500)], ("q8_direct", "01", 0, [1, 1])),
    "twins_with_unused_bytes": (KC, P8, [B(1000, 1000, use=0), T(1500, 1500)], ("q8_refine", "01", 0, [0, 4])),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("routes")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    cc = subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", str(exe), str(src)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return str(exe)


def run(driver, knobs, prune, pairs):
    prefilter, q8_route, q8_direct, level = knobs
    line = [prefilter, q8_route, q8_direct, f32(level).hex(), prune[0], f32(prune[1]).hex(), len(pairs)]
    for p in pairs:
        line += list(p)
    out = subprocess.run([driver], input=" ".join(str(x) for x in line) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    f = out.stdout.split()
    return f[0], f[1], int(f[2]), [int(x) for x in f[3:]]


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_route_table(driver, name):
    knobs, prune, pairs, want = SCENARIOS[name]
    assert run(driver, knobs, prune, pairs) == want


def test_table_covers_every_knob_value():
    seen = {(i, k[i]) for k, _, _, _ in SCENARIOS.values() for i in range(3)}
    assert {(i, v) for i in range(3) for v in (0, 1, 2)} <= seen
    assert {0.0, 0.625, next_up(0.625)} <= {f32(k[3]) for k, _, _, _ in SCENARIOS.values()}
    assert {R95, next_up(R95)} <= {f32(p[1]) for _, p, _, _ in SCENARIOS.values()}
