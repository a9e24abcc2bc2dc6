"""The cut of the sweeps' work-item list into the eight XCDs' chunks (msfm_item_chunks, monocularsfm_amd/csrc/msfm_hostutil.h),
compiled here with g++ around a driver:

  * every item appears exactly once: the chunks are contiguous, in list order, start at 0 and end at the item count, and
    msfm_item_position sends the items of chunk x, in order, to the positions x, 8 + x, 16 + x, ... of a list 8 x the longest chunk long;
  * chunk costs differ by at most one item's cost (the most expensive item's) on the lists named below: no item, 1 item, 7 items,
    8 k + 1 items, all-equal costs, one very expensive item -- and on the two lists of a mixed sub-batch (all pairs with the pairs
    of the other sweep at the skipped items' cost; those pairs alone), built from pair sizes as build_items builds them;
  * on random run lists the bound that holds by construction: every boundary starts at most half an item's cost from its mark
    x / 8 of the total, so any two chunks differ by at most two items' cost, and the second step only ever narrows that.
The bounds are the function's own reasoning (the comment above it), not what it was seen to return."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "monocularsfm_amd", "csrc")

DRIVER = r"""
#include "msfm_hostutil.h"
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>
static std::vector<long long> expand(const std::vector<MsfmItemRun>& runs) {
    std::vector<long long> c;
    for (const MsfmItemRun& r : runs)
        for (long long k = 0; k < r.count; ++k) c.push_back(r.cost > 1 ? r.cost : 1);
    return c;
}
// -> false with a message; strict: the chunks' costs differ pairwise by at most the most expensive item's cost
static bool check(const char* what, const std::vector<MsfmItemRun>& runs, bool strict) {
    const std::vector<long long> c = expand(runs);
    const MsfmItemChunks ch = msfm_item_chunks(runs);
    const long long n = (long long)c.size();
    if (ch.start[0] != 0 || ch.items() != n) { std::printf("%s: ends %d .. %d of %lld\n", what, ch.start[0], ch.items(), n); return false; }
    for (int x = 0; x < kItemChunks; ++x)
        if (ch.start[x + 1] < ch.start[x]) { std::printf("%s: chunk %d runs backwards\n", what, x); return false; }
    long long total = 0, cmax = 0;
    for (long long v : c) total += v, cmax = std::max(cmax, v);
    long long lo = -1, hi = -1;
    const int per = ch.longest();
    std::vector<char> taken((size_t)per * kItemChunks, 0);
    for (int x = 0; x < kItemChunks; ++x) {
        long long cost = 0;
        for (int k = ch.start[x]; k < ch.start[x + 1]; ++k) {
            cost += c[(size_t)k];
            if (msfm_item_chunk_of(ch, k) != x) { std::printf("%s: item %d not in chunk %d\n", what, k, x); return false; }
            const long long pos = msfm_item_position(ch, k);
            if (pos != (long long)(k - ch.start[x]) * kItemChunks + x || pos < 0 || pos >= (long long)taken.size() || taken[(size_t)pos]) {
                std::printf("%s: item %d at position %lld\n", what, k, pos);
                return false;
            }
            taken[(size_t)pos] = 1;
        }
        lo = lo < 0 ? cost : std::min(lo, cost), hi = std::max(hi, cost);
    }
    if (std::count(taken.begin(), taken.end(), 1) != n) { std::printf("%s: %lld items placed\n", what, (long long)std::count(taken.begin(), taken.end(), 1)); return false; }
    if (hi - lo > (strict ? 1 : 2) * cmax) { std::printf("%s: chunk costs %lld .. %lld, largest item %lld\n", what, lo, hi, cmax); return false; }
    return true;
}
// the run list of a set of pairs as build_items makes it (integer sweep: 16 waves of 32 rows)
struct P { int n1, n2; bool twin; };
static std::vector<MsfmItemRun> pair_runs(const std::vector<P>& pairs, int list) {   // list 0: all, 1: all with the others idle, 2: the others alone
    std::vector<MsfmItemRun> runs;
    for (const P& p : pairs) {
        if (list == 2 && p.twin) continue;
        const int nab = (p.n1 + 511) / 512, tiles = 2 * ((p.n2 + 127) / 128);
        if (list == 1 && !p.twin) { runs.push_back(MsfmItemRun{nab, msfm_item_cost(0, 0, 32, 16)}); continue; }
        if (nab > 1) runs.push_back(MsfmItemRun{nab - 1, msfm_item_cost(tiles, 512, 32, 16)});
        runs.push_back(MsfmItemRun{1, msfm_item_cost(tiles, p.n1 - (nab - 1) * 512, 32, 16)});
    }
    return runs;
}
int main() {
    // the cost model: more tiles, more rows cost more; a block with one real row is cheaper than a full one but not free
    if (!(msfm_item_cost(80, 512, 32, 16) > msfm_item_cost(72, 512, 32, 16) && msfm_item_cost(80, 1, 32, 16) < msfm_item_cost(80, 512, 32, 16) &&
          msfm_item_cost(80, 1, 32, 16) > msfm_item_cost(0, 0, 32, 16) && msfm_item_cost(80, 512, 32, 16) == msfm_item_cost(80, 512, 64, 8) &&
          msfm_item_cost(80, 129, 32, 16) == msfm_item_cost(80, 256, 32, 16))) { std::printf("cost model\n"); return 1; }
    bool ok = true;
    ok = check("no item", {}, true) && ok;
    ok = check("1 item", {{1, 5000}}, true) && ok;
    ok = check("7 items", {{3, 4000}, {1, 1200}, {3, 4100}}, true) && ok;
    ok = check("7 equal items", {{7, 4000}}, true) && ok;
    for (long long k : {1LL, 2LL, 13LL, 1000LL, 10625LL}) {
        ok = check("8 k + 1 equal items", {{8 * k + 1, 5280}}, true) && ok;
        ok = check("8 k + 1 items, two costs", {{4 * k, 5280}, {1, 1500}, {4 * k, 4768}}, true) && ok;
        ok = check("8 k equal items", {{8 * k, 5280}}, true) && ok;
    }
    for (long long where : {0LL, 1LL, 40LL, 99LL, 100LL}) {   // one very expensive item among 100 cheap ones, at either end and inside
        std::vector<MsfmItemRun> runs;
        if (where > 0) runs.push_back({where, 176});
        runs.push_back({1, 1000000});
        if (where < 100) runs.push_back({100 - where, 176});
        ok = check("one very expensive item", runs, true) && ok;
    }
    ok = check("zero and negative costs count as 1", {{5, 0}, {4, -3}, {0, 100}, {-2, 100}, {8, 1}}, true) && ok;
    // a mixed sub-batch: pairs of 1 x 5400 and 5400 x 1 rows next to 600 x 600 ones and bench-sized ones
    std::mt19937 rng(7);
    std::vector<P> pairs;
    for (int k = 0; k < 300; ++k) {
        const int kind = (int)(rng() % 4);
        P p = {600, 600, (rng() & 1) != 0};
        if (kind == 1) p.n1 = 1, p.n2 = 5400;
        if (kind == 2) p.n1 = 5400, p.n2 = 1;
        if (kind == 3) p.n1 = 4600 + (int)(rng() % 801), p.n2 = 4600 + (int)(rng() % 801);
        pairs.push_back(p);
    }
    for (int list = 0; list < 3; ++list) ok = check(list == 0 ? "all pairs" : list == 1 ? "mixed, first list" : "mixed, second list", pair_runs(pairs, list), true) && ok;
    // random run lists: the bound by construction
    for (int t = 0; t < 2000; ++t) {
        std::vector<MsfmItemRun> runs;
        const int nr = (int)(rng() % 40);
        for (int r = 0; r < nr; ++r) runs.push_back({(long long)(rng() % (t & 1 ? 4 : 300)), (long long)(1 + rng() % (t & 2 ? 10 : 6000))});
        ok = check("random", runs, false) && ok;
    }
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
"""


def test_item_chunks(tmp_path):
    src = tmp_path / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip().endswith("OK"), res.stdout[-2000:]
