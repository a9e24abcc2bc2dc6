"""The pure policy of vocabulary retrieval (monocularsfm_amd/csrc/msfm_retrieval.h), compiled here with g++, against hand-worked values
and the numpy reference (tests/retrieval_ref.py); and the reference's own recall on a planted co-visibility scene.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import retrieval_ref as ref  # noqa: E402

CSRC = os.path.join(HERE, "..", "monocularsfm_amd", "csrc")

DRIVER = r"""
#include "msfm_retrieval.h"
#include <cstdio>
#include <iostream>
#include <string>
int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "sample") {
            long long r, m;
            std::cin >> r >> m;
            const MsfmRetSample s = msfm_ret_sample(r, m);
            std::printf("%lld %lld\n", (long long)s.step, (long long)s.count);
        } else if (cmd == "vocab") {
            long long v, ms;
            std::cin >> v >> ms;
            std::printf("%d\n", msfm_ret_vocab_size((int)v, ms));
        } else if (cmd == "init") {
            long long ms;
            int vp;
            std::cin >> ms >> vp;
            for (int k = 0; k < vp; ++k) std::printf("%lld ", (long long)msfm_ret_initial_row(k, ms, vp));
            std::printf("\n");
        } else if (cmd == "centroid") {
            unsigned long long s, c;
            std::cin >> s >> c;
            std::printf("%u\n", msfm_ret_centroid(s, c));
        } else if (cmd == "topk") {
            int n, self, k;
            std::cin >> n >> self >> k;
            std::vector<float> s(n);
            std::vector<int32_t> ids(n);
            for (float& x : s) { std::string t; std::cin >> t; x = std::stof(t); }
            for (int32_t& x : ids) std::cin >> x;
            for (int p : msfm_ret_topk(s.data(), ids.data(), n, self, k)) std::printf("%d ", p);
            std::printf("\n");
        } else if (cmd == "union" || cmd == "groups") {
            int m, per = 0;
            std::cin >> m;
            if (cmd == "groups") std::cin >> per;
            std::vector<std::pair<int, int>> p(m);
            for (auto& x : p) std::cin >> x.first >> x.second;
            if (cmd == "union") {
                for (auto& x : msfm_ret_union(p)) std::printf("%d,%d ", x.first, x.second);
            } else {
                for (size_t e : msfm_ret_group_ends(p, per)) std::printf("%zu ", e);
            }
            std::printf("\n");
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def policy(tmp_path_factory):
    d = tmp_path_factory.mktemp("retrieval_policy")
    src = d / "drv.cpp"
    src.write_text(DRIVER)
    exe = d / "drv"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        return out.strip("\n").split("\n")
    return run


@pytest.mark.parametrize("rows,max_rows,step,count", [
    (100, 1000, 1, 100),     # R < M: every row
    (1000, 1000, 1, 1000),   # R == M
    (1001, 1000, 1, 1000),   # R / M = 1: the first M rows
    (2999, 1000, 2, 1000),   # R not a multiple of M: s = 2, capped at M
    (2000, 1000, 2, 1000),
    (3001, 1000, 3, 1000),
    (7, 3, 2, 3),            # rows 0, 2, 4
    (0, 10, 1, 0),
])
def test_sample_plan(policy, rows, max_rows, step, count):
    assert ref.sample_plan(rows, max_rows) == (step, count)
    assert policy(["sample %d %d" % (rows, max_rows)]) == ["%d %d" % (step, count)]


@pytest.mark.parametrize("v,ms,want", [(16384, 1000, 125), (16384, 7, 1), (16384, 0, 1), (10, 1000, 10), (33, 264, 33), (33, 263, 32)])
def test_vocab_size(policy, v, ms, want):
    assert ref.vocab_size(v, ms) == want
    assert policy(["vocab %d %d" % (v, ms)]) == [str(want)]


def test_initial_rows(policy):
    for ms, vp in [(100, 12), (8, 1), (1000, 125), (17, 2)]:
        got = [int(x) for x in policy(["init %d %d" % (ms, vp)])[0].split()]
        assert got == ref.initial_rows(vp, ms)
    assert [int(x) for x in policy(["init 17 2"])[0].split()] == [0, 8]


@pytest.mark.parametrize("total,cnt,want", [(3, 2, 2), (1, 2, 1), (5, 2, 3), (0, 1, 0), (255 * 7, 7, 255), (10, 4, 3), (9, 4, 2),
                                            (2 ** 31 + 1, 2, 2 ** 30 + 1)])
def test_centroid_rounding(policy, total, cnt, want):
    # floor((2 sum + cnt) / (2 cnt)): a mean at .5 rounds up (1.5 -> 2, 0.5 -> 1, 2.5 -> 3)
    assert ref.centroid(total, cnt) == want
    assert policy(["centroid %d %d" % (total, cnt)]) == [str(want)]


def _topk_line(s, ids, self_pos, k):
    return "topk %d %d %d %s %s" % (len(s), self_pos, k, " ".join(repr(float(np.float32(x))) for x in s), " ".join(map(str, ids)))


@pytest.mark.parametrize("s,ids,self_pos,k", [
    ([0.0, 0.5, 0.5, 0.25, 0.5], [4, 9, 2, 7, 5], 0, 2),      # three-way tie at the top: the lower ids 2, 5
    ([0.0, 0.5, 0.5, 0.25, 0.5], [4, 9, 2, 7, 5], 0, 3),      # the K boundary inside the tie
    ([0.3, 0.0, 0.2, -0.1, 0.2], [0, 1, 2, 3, 4], 1, 10),     # K >= N - 1: every s > 0, no zero, no negative
    ([0.9, 0.9, 0.9], [3, 1, 2], 1, 5),                       # self excluded even at the top score
    ([0.0, 0.0], [0, 1], 0, 1),                               # nobody
])
def test_topk_ties(policy, s, ids, self_pos, k):
    s32 = np.asarray(s, np.float32)
    want = ref.topk(s32, ids, self_pos, k)
    got = policy([_topk_line(s32, ids, self_pos, k)])[0].split()
    assert [int(x) for x in got] == want
    if s == [0.0, 0.5, 0.5, 0.25, 0.5] and k == 2:
        assert want == [2, 4]


def test_union_orientation_and_order(policy):
    sel = [(3, 1), (1, 3), (0, 5), (5, 0), (2, 4), (4, 2), (9, 1), (2, 2)]
    got = policy(["union %d %s" % (len(sel), " ".join("%d %d" % p for p in sel))])[0].split()
    assert got == ["3,1", "4,2", "5,0", "9,1"]


def test_groups_like_brute_mode(policy):
    # row 5 has 250 pairs: groups of 100, 100, 50; rows 6 and 7 end their own groups
    pairs = [(5, j) for j in range(250)] + [(6, 0), (6, 3)] + [(7, j) for j in range(100)]
    got = policy(["groups %d 100 %s" % (len(pairs), " ".join("%d %d" % p for p in pairs))])[0].split()
    assert [int(x) for x in got] == [100, 200, 250, 252, 352]


def test_reference_selection_k_ge_n_minus_1():
    s = np.array([[0, .2, 0, .4], [.2, 0, .1, 0], [0, .1, 0, .3], [.4, 0, .3, 0]])
    assert ref.select(s, [10, 11, 12, 13], 3) == [(11, 10), (12, 11), (13, 10), (13, 12)]


def test_reference_recall_on_planted_scene():
    images, overlap = ref.covis_scene(24, window=8, stride=2, seed=3)
    ids = list(images)
    words, _ = ref.train(images, ids, num_words=64, iters=8)
    order, s, _ = ref.scores(images, ids, words)
    k = 6
    for a, i in enumerate(order):
        top = {order[j] for j in ref.topk(s[a], order, a, k)}
        need = {j for j in order if j != i and overlap(i, j) >= 0.5}
        assert need <= top, (i, sorted(need - top))


def test_reference_assign_ties_and_quantisation():
    # equidistant rows go to the lower word; x 255 at .5 rounds half to even
    words = np.full((2, 128), 100, np.uint8)
    words[1, 0] = 102
    q = np.full((1, 128), 100, np.int64)
    q[0, 0] = 101
    assert ref.assign(q, words).tolist() == [0]
    x = np.array([[0.5 / 255 * 1] * 128], np.float32)
    qq = ref.quantize(x)
    assert qq[0, 0] == np.rint(np.float32(x[0, 0]) * np.float32(255))
    with pytest.raises(ValueError):
        ref.quantize(np.full((2, 128), 1.5, np.float32))


def _small_scenes():
    rng = np.random.default_rng(41)
    images, _ = ref.covis_scene(24, window=8, stride=2, seed=3)
    yield images, 64
    fimages, _ = ref.covis_scene(12, window=6, stride=3, seed=4, as_float=True)
    fimages[12] = np.zeros((0, 128), np.float32)                          # an empty image between non-empty ones
    fimages[13] = rng.integers(0, 2, size=(30, 128)).astype(np.float32)   # 0.0 / 1.0 only: q = x
    yield fimages, 40


def test_reference_helpers_equal_scores_and_assign():
    for images, v in _small_scenes():
        ids = list(images)
        words, _ = ref.train(images, ids, num_words=v, iters=4)
        order, s, nnz = ref.scores(images, ids, words)
        wl = []
        for i in order:
            q = ref.quantize(images[i])
            w = ref.assign(q, words)
            # any chunking gives the same words: one row, a few rows, everything at once
            for block in (8 * len(words), 8 * len(words) * 7, 1 << 40):
                assert np.array_equal(ref.assign(q, words, block_bytes=block), w)
            wl.append(w)
        s2, nnz2 = ref.scores_from_words(wl, len(words))
        assert np.array_equal(nnz2, nnz)
        assert np.array_equal(s2, s)
        rows = [0, 5, len(order) - 1, 3]
        s3, _ = ref.scores_from_words(wl, len(words), rows=rows)
        assert np.allclose(s3, s[rows], rtol=0, atol=1e-15)
        assert all(s3[r, p] == 0 for r, p in enumerate(rows))
        for k in (1, 3, 6, len(order)):
            assert ref.select_fast(s, order, k) == ref.select(s, order, k)
            top = ref.select_rows(s3, order, k, rows=rows)
            assert [t.tolist() for t in top] == [ref.topk(s3[r], order, p, k) for r, p in enumerate(rows)]


def test_select_rows_equals_topk_under_heavy_ties():
    rng = np.random.default_rng(42)
    for n, k in [(50, 1), (50, 7), (120, 119), (200, 40)]:
        s = rng.choice(np.array([-0.5, 0.0, 0.25, 0.5, 0.75], np.float32), size=(n, n))
        s = np.triu(s, 1) + np.triu(s, 1).T
        ids = rng.permutation(10 * n)[:n].tolist()
        got = ref.select_rows(s, ids, k)
        for i in range(n):
            assert got[i].tolist() == ref.topk(s[i], ids, i, k)
        assert ref.select_fast(s, ids, k) == ref.select(s, ids, k)


def test_group_ends_twin(policy):
    rng = np.random.default_rng(43)
    pairs = sorted({(int(i), int(j)) for i, j in rng.integers(0, 300, size=(2000, 2)) if i > j})
    for per in (1, 7, 100):
        line = "groups %d %d %s" % (len(pairs), per, " ".join("%d %d" % p for p in pairs))
        assert [int(x) for x in policy([line])[0].split()] == ref.group_ends(pairs, per)


@pytest.mark.parametrize("n,k,seed", [(1329, 50, 0), (2000, 1024, 1), (10000, 1, 2), (10000, 1024, 3), (10000, 513, 4), (300, 1024, 5)])
def test_topk_policy_at_scale(policy, n, k, seed):
    # a handful of levels: hundreds of exact ties, zeros and negatives (never candidates), ids not in position order
    rng = np.random.default_rng(50 + seed)
    levels = np.array([-1.0, -2.0 ** -20, 0.0, 2.0 ** -24, 0.125, 0.5, 0.5000001, 0.9], np.float32)
    ids = rng.permutation(10000)[:n].astype(np.int32)
    lines, want = [], []
    for self_pos in (0, n // 2, n - 1):
        s = levels[rng.integers(0, len(levels), size=n)]
        if seed == 5:
            s[:] = np.float32(0.5)                     # every candidate tied, K >= N - 1
        lines.append(_topk_line(s, ids.tolist(), self_pos, k))
        want.append(ref.topk(s, ids.tolist(), self_pos, k))
    got = policy(lines)
    for g, w in zip(got, want):
        assert [int(x) for x in g.split()] == w
        assert len(w) == min(k, len(w)) and len(w) > 0
