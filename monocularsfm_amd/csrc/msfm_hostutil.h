// msfm_hostutil.h -- small pure functions shared by device and host code, compilable on their own (tests/test_hostutil.py builds a
// g++ driver around them): the 4-byte packing of the integer sweeps' column partials, the cost marks of a call's sub-batches, the
// scratch memory one image pair of a sub-batch needs, the matching route of a sub-batch, the fold of a candidate's key into a slot's
// (best, second), the ratio cap of the reverse thresholds and the order-invariance certificate, the two-view model selection's rule.
#pragma once
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSFM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MSFM_HD inline
#endif

// Column partial of the integer sweeps -- per column and 512-row block the two largest accumulators (relative to the item's K:
// -S~/2, <= 1, > -2^23) -- in FOUR bytes instead of the float pipeline's float2: the largest exactly (24 bits; -2^23 = "no real
// row"), and an 8-bit code of how far below it the second largest is, rounded UP: code c stands for
// ((16 + (c & 15)) << (c >> 4)) - 16 (exact up to 15, then 1/16 steps; 255 = "no second").  The second value is only ever used as
// an upper bound of the column's second-smallest S^ -- a smaller accumulator is a larger S^ -- so rounding the gap up keeps every
// bound valid; it halves what sweep 1 writes and the thresholds / prune kernels read (3.3 GB -> 1.65 GB per 8128-pair job).
MSFM_HD int msfm_cp_pack(int hi, bool hi_valid, int lo, bool lo_valid) {
    unsigned c = 255u;
    if (lo_valid) {
        const unsigned x = (unsigned)(hi - lo) + 16u;          // gap + 16 >= 16
        int e = 27 - __builtin_clz(x);                         // floor(log2 x) - 4 >= 0
        unsigned m = (x + (1u << e) - 1u) >> e;                // 16 .. 32, rounded up
        e += (int)(m >> 5);                                    // (m == 32 -> 16 at the next exponent)
        m = (m >> 5) ? 16u : m;
        const unsigned code = ((unsigned)e << 4) | (m - 16u);
        c = code >= 255u ? 255u : code;                        // (e > 15 lands here as well)
    }
    return hi_valid ? (int)(((unsigned)hi << 8) | c) : (int)0x80000000;
}
constexpr int kCpNone = -(1 << 23);                                           // the "no real row" value of the 24-bit field
MSFM_HD int msfm_cp_hi(int code) { return code >> 8; }                        // kCpNone: no real row
MSFM_HD bool msfm_cp_has_second(int code) { return (code & 255) != 255; }
MSFM_HD int msfm_cp_gap(int code) { const int c = code & 255; return ((16 + (c & 15)) << (c >> 4)) - 16; }

// Cumulative-cost marks of the parts a large call is cut into (msfm_set_pipeline): n_sub parts whose size shrinks linearly towards
// the end of the call, the last one to `taper` of the average -- what follows the LAST sweep 1 of a call (that part's thresholds,
// plan, sweep 2, exact re-check, epilogue) has nothing left to hide behind, and it is proportional to the part's size.
// -> marks[0] = 0 < marks[1] < ... < marks[n_sub] = total.
inline std::vector<long long> msfm_pipeline_marks(long long total, long long n_sub, double taper) {
    std::vector<long long> marks;
    if (n_sub < 2) return marks;
    const double last = taper, first = 2.0 - last;
    double acc = 0.0;
    marks.push_back(0);
    for (long long k = 0; k < n_sub; ++k) {
        acc += first - (first - last) * (double)k / (double)(n_sub - 1);
        marks.push_back(k + 1 == n_sub ? total : (long long)((double)total * acc / (double)n_sub));
    }
    return marks;
}

// ---- The hand-out of the sweeps' work items to the 8 XCDs.  The linear item list -- pairs in the order of their
// streamed image, a pair's items in the order (range, A block) -- is cut into 8 CONTIGUOUS chunks of nearly equal COST, one per XCD;
// chunk x's items sit at positions (k - start[x]) * 8 + x of the device list, whose length is 8 x the longest chunk.  The workgroups
// of an XCD take the items of its chunk in order from a cursor (sweep kernels), so a chunk's cost is what its XCD has to do.
constexpr int kItemChunks = 8;
struct MsfmItemChunks {                      // (a kernel argument as it is)
    int start[kItemChunks + 1];              // chunk x = linear items start[x] .. start[x + 1] - 1; start[8] = all items
    int items() const { return start[kItemChunks]; }
    int longest() const {
        int m = 0;
        for (int x = 0; x < kItemChunks; ++x) m = start[x + 1] - start[x] > m ? start[x + 1] - start[x] : m;
        return m;
    }
};
MSFM_HD int msfm_item_chunk_of(const MsfmItemChunks& c, int k) {   // the chunk of linear item k
    int x = 0;
#pragma unroll
    for (int j = 1; j < kItemChunks; ++j) x += k >= c.start[j] ? 1 : 0;
    return x;
}
MSFM_HD long long msfm_item_position(const MsfmItemChunks& c, int k) {
    const int x = msfm_item_chunk_of(c, k);
    return (long long)(k - c.start[x]) * kItemChunks + x;
}

// Cost of one sweep-1 item, in arbitrary units (a full tile = 64): `b_tiles` 64-row tiles of the streamed image against one block of
// `wave_rows * waves` A rows of which `rows` are real.  This is a MODEL, not a measurement: a tile's time is taken as a fixed part
// (barrier, DMA issue, the slowest wave's wake-up: 16) plus the matrix and epilogue work of the busiest SIMD, proportional to the
// waves of the block that hold a real row there (waves w, w + 4, ... share a SIMD; a wave without a real row skips both halves);
// an item's own prologue and row transposition count as 2.5 full tiles.  Only the RATIO between an image's last block and a full
// one, and between items of different tile counts, matters -- and only across XCDs: within one the cursor evens out what is left.
constexpr int kItemCostTileFixed = 16, kItemCostTileWaves = 48, kItemCostFixed = 160;
inline long long msfm_item_cost(int b_tiles, int rows, int wave_rows, int waves) {
    const int active = rows <= 0 ? 0 : (rows >= wave_rows * waves ? waves : (rows + wave_rows - 1) / wave_rows);
    const int per_simd = (active + 3) / 4, full = (waves + 3) / 4;
    return kItemCostFixed + (long long)b_tiles * (kItemCostTileFixed + kItemCostTileWaves * per_simd / full);
}

// `count` consecutive items of the linear list, each of cost `cost` (a pair and range: its full A blocks, then its last block)
struct MsfmItemRun { long long count, cost; };
// The cut: boundary x is the item boundary whose cumulative cost is NEAREST to x / 8 of the total (ties: the earlier one).  Every
// boundary is then at most half an item's cost (the most expensive one's) from its mark, so every chunk's cost is within one item's
// cost of total / 8 and any two chunks within two; equal costs give chunk lengths that differ by at most one item.  A second step
// (below) narrows the spread between the chunks to one item's cost where moving boundaries by single items can.  Fewer than 8
// items leave chunks empty.
inline MsfmItemChunks msfm_item_chunks(const std::vector<MsfmItemRun>& runs) {
    MsfmItemChunks c = {};
    long long total = 0, n = 0;
    for (const MsfmItemRun& r : runs) total += (r.count > 0 ? r.count : 0) * (r.cost > 1 ? r.cost : 1), n += r.count > 0 ? r.count : 0;
    c.start[kItemChunks] = (int)n;
    std::size_t ri = 0;
    long long acc = 0, idx = 0;      // cost and items before run ri
    for (int x = 1; x < kItemChunks; ++x) {
        const long long mark = total * x;   // in units of 1 / 8 cost: compare with 8 x a cumulative cost
        // the run the mark falls into: the first whose end reaches it
        while (ri < runs.size()) {
            const long long cnt = runs[ri].count > 0 ? runs[ri].count : 0, cost = runs[ri].cost > 1 ? runs[ri].cost : 1;
            if (kItemChunks * (acc + cnt * cost) >= mark) break;
            acc += cnt * cost, idx += cnt, ++ri;
        }
        if (ri == runs.size()) { c.start[x] = (int)n; continue; }
        const long long cnt = runs[ri].count > 0 ? runs[ri].count : 0, cost = runs[ri].cost > 1 ? runs[ri].cost : 1;
        const long long num = mark - kItemChunks * acc, den = kItemChunks * cost;   // j items of the run: |j * den - num| smallest
        long long j = (2 * num + den - 1) / (2 * den);
        j = j < 0 ? 0 : (j > cnt ? cnt : j);
        c.start[x] = (int)(idx + j);
    }
    // Two boundaries may err in opposite directions, which leaves two chunks up to two items' cost apart: while the most and the
    // least expensive chunk differ by more than the most expensive item, the boundaries between them move one item towards the
    // expensive one -- it hands an item down the row, the cheap one receives one -- as long as that narrows the spread.
    std::vector<long long> items_end(runs.size()), cost_end(runs.size());
    long long cmax = 0;
    acc = 0, idx = 0;
    for (std::size_t r = 0; r < runs.size(); ++r) {
        const long long cnt = runs[r].count > 0 ? runs[r].count : 0, cost = runs[r].cost > 1 ? runs[r].cost : 1;
        acc += cnt * cost, idx += cnt, items_end[r] = idx, cost_end[r] = acc;
        if (cnt > 0 && cost > cmax) cmax = cost;
    }
    auto cum = [&](long long k) -> long long {   // cost of the first k items
        std::size_t lo = 0, hi = runs.size();
        while (lo < hi) {                        // the first run that ends at or behind item k
            const std::size_t mid = (lo + hi) / 2;
            if (items_end[mid] < k) lo = mid + 1; else hi = mid;
        }
        if (lo == runs.size()) return total;
        const long long cost = runs[lo].cost > 1 ? runs[lo].cost : 1;
        return cost_end[lo] - (items_end[lo] - k) * cost;
    };
    auto spread = [&](const MsfmItemChunks& t, int* most, int* least) -> long long {
        long long hi = -1, lo = -1;
        for (int x = 0; x < kItemChunks; ++x) {
            const long long v = cum(t.start[x + 1]) - cum(t.start[x]);
            if (hi < 0 || v > hi) hi = v, *most = x;
            if (lo < 0 || v < lo) lo = v, *least = x;
        }
        return hi - lo;
    };
    for (int pass = 0; pass < 8 * kItemChunks; ++pass) {
        int most = 0, least = 0;
        const long long s = spread(c, &most, &least);
        if (s <= cmax) break;
        MsfmItemChunks t = c;
        if (most < least) for (int x = most + 1; x <= least; ++x) t.start[x] -= 1;
        else for (int x = least + 1; x <= most; ++x) t.start[x] += 1;
        int m2 = 0, l2 = 0;
        if (spread(t, &m2, &l2) >= s) break;
        c = t;
    }
    return c;
}

// What the two-view geometry (msfm_set_two_view_geometry) adds to msfm_pair_scratch_bytes for one pair: per staged match (at most
// n1) the kept-index slot (4 B) and the angle slot (8 B) of tv_pose_kernel, per pair its record (144 B) and the saved winner (4 B).
inline long long msfm_pair_two_view_bytes(int n1, int n2) {
    if (n1 <= 0 || n2 <= 0) return 0;
    return 12LL * n1 + 148;
}

// Device scratch ONE image pair adds to a sub-batch, in bytes -- what MatchJob::build (msfm_job.hip.h) cuts a call by, and
// what the buffers of a scratch set really hold (round 3 charged 2 x a_blocks128 x n2pad 4-byte units per pair whatever the
// route: 2.6 - 3.4 x what the matrix-core route allocates, so a "48 GiB" budget produced 200 sub-batches of config 4 on a
// 58 GiB footprint).  n1pad / n2pad: rows padded to 512; blocks128 / blocks512: 128- / 512-row blocks of image 1.
//   route 1, matrix cores, match lists with ratio <= 0.95 (compacted sweep 2): row partials 2 x 4 B x n1pad | column partials
//     8 B (fp16 route: float2; the integer routes use 4 of them) per 512-row block and column | thresholds, block masks, best /
//     second keys, final kNN arrays: 36 B per padded row and column | staged + compact match lists 24 B per row | the plan of
//     sweep 2 and its candidate lists for ONE SIXTEENTH of the rows alive (measured: 1 - 3.3 %; buffers that turn out too small are
//     re-grown and the sub-batch re-run, this is only the cut): 20 B + 8 candidates x 8 B per compacted row, a column once per
//     512-row block group (at most 32);
//   route 3, INTEGER matrix cores (both images byte stores, match lists with ratio <= 0.95): as route 1 with 4-byte column partials and
//     without the final kNN arrays (the epilogue reads the reduce slots: 24 B per padded row and column), + 4 B per candidate and
//     compacted row for the exact-S hand-over of sweep 2;
//   route 4, route 1 for float stores whose byte twins are coarse (values beyond 0.625): one EIGHTH of the rows instead of a sixteenth;
//   route 2, matrix cores, dense sweep 2 (kNN-level API, ratio > 0.95): candidate lists of 16 entries per row and column instead;
//   route 0, brute force: three 4-byte row partials per padded row, three per 128-row block and column.
// (A mixed sub-batch -- byte pairs next to float pairs -- allocates by route 1's sizes for all of them: this is the cut, not a cap.)
// two_view: the call computes two-view geometry records (msfm_pair_two_view_bytes on top, whatever the route).
// two_view_refine: it also refines them (msfm_set_two_view_refinement): the pair's msfm_two_view_refinement, 40 B.
inline long long msfm_pair_scratch_bytes(int n1, int n2, int n1pad, int n2pad, int blocks128, int blocks512, int route,
                                         bool two_view = false, bool two_view_refine = false) {
    if (n1 <= 0 || n2 <= 0) return 0;
    const long long slots = (long long)n1pad + n2pad;
    const long long common = (route == 3 ? 24LL : 36LL) * slots + 24LL * n1 + 1024 + (two_view ? msfm_pair_two_view_bytes(n1, n2) : 0) +
                             (two_view_refine ? 40LL : 0);
    if (route == 0) return common + 12LL * n1pad + 12LL * (long long)blocks128 * n2pad;
    const long long partials = 8LL * n1pad + (route == 3 ? 4LL : 8LL) * (long long)blocks512 * n2pad;
    if (route == 2) return common + partials + 128LL * ((long long)n1 + n2) + 16384;
    const long long bits = blocks512 < 32 ? blocks512 : 32;
    // (route 4 = route 1 with COARSE byte twins, msfm_q8.hip.h: plan A holds every live column once per block group and the prune kernel
    // only knows live / dead -- twice the compacted rows of the direct route)
    const long long cmp_rows = ((long long)n1 + (long long)n2 * bits) / (route == 4 ? 8 : 16) + 1024;
    return common + partials + (route == 3 ? 120LL : 84LL) * cmp_rows;
}

// ---- The matching route of a sub-batch: the ONE statement of the policy (every route gives the same bits).  msfm_route
// runs once per sub-batch (prepare_batch_images), MatchJob::build cuts a call by msfm_scratch_route before any sub-batch exists.
// with twins at least this fine the twins' sweep yields thresholds tight enough to collect candidates with directly
// (~4.5 per live row on RootSIFT-like data against 2.5 after an fp16 sweep 1'; 12 at m = 1): no sweep 1' (msfm_q8.hip.h)
constexpr float kQ8DirectMaxLevel = 0.625f;
struct MsfmRouteKnobs { int prefilter, q8_route, q8_direct; float q8_level; };   // the context's (msfm_ctx.hip.h; q8_level 0: no twins yet)
// Sweep 2 on the compacted live rows, or on everything again?  The Lowe test kills ~94 % of the rows at ratio 0.8 on SIFT-like data; near
// or above 1 almost every row stays alive, and the compacted sweep (both directions separately) would do up to twice the dense one's work.
inline bool msfm_compact_sweep2(int prune, float ratio) { return prune != 0 && ratio > 0.f && ratio <= 0.95f; }
// route Q at all: twins are read on the integer-core prefilter only
inline bool msfm_twin_route_on(const MsfmRouteKnobs& k) { return k.prefilter == 1 && k.q8_route != 0; }
// fine twins: their sweep's bounds are the thresholds of sweep 2; coarse ones (a store with values near 1): an fp16 sweep 1' first
inline bool msfm_fine_twins(const MsfmRouteKnobs& k) { return k.q8_direct == 2 || (k.q8_direct == 1 && k.q8_level <= kQ8DirectMaxLevel); }
// both images byte stores (a store is bytes throughout or not at all)
inline bool msfm_byte_pair(bool a_is_u8, bool b_is_u8) { return a_is_u8 && b_is_u8; }

// Route of a sub-batch's prefiltered pairs (brute-force pairs run beside any of them):
enum MsfmRouteKind {
    kRouteDense,      // prune off or ratio > 0.95 (the kNN-level API): fp16 sweep 1, thresholds, dense sweep 2
    kRouteFp16,       // fp16 sweep 1, compacted sweep 2
    kRouteI8,         // every pair joins two byte images: both sweeps on the integer cores, exact S from the sweep itself
    kRouteQ8Direct,   // route Q, fine twins on every pair: the twins' sweep 1 on the integer cores gives sweep 2 its thresholds
    kRouteQ8Mixed,    // route Q, fine twins on some pairs: the twins' sweep 1 for them, the fp16 sweep 1 for the others
    kRouteQ8Refine,   // route Q, coarse twins on every pair: the twins' sweep 1, plan A, fp16 sweep 1' of the live rows
};
struct MsfmRoute {
    MsfmRouteKind kind = kRouteDense;
    std::vector<char> twin;          // per pair: swept on its twins (route Q; the others of a mixed sub-batch take the fp16 sweep 1)
    long long demoted_pairs = 0;     // pairs that could take an integer route alone but go to the fp16 cores with the rest
    bool compact() const { return kind != kRouteDense; }
    bool q8() const { return kind >= kRouteQ8Direct; }
};
struct MsfmRoutePair { bool valid, use, a_is_u8, b_is_u8, a_twin, b_twin; int n1, n2; };   // (a pair counts when valid and in use)

inline MsfmRoute msfm_route(const MsfmRouteKnobs& k, int prune, float ratio, const std::vector<MsfmRoutePair>& pairs) {
    MsfmRoute r;
    r.twin.assign(pairs.size(), 0);
    if (!msfm_compact_sweep2(prune, ratio)) return r;
    r.kind = kRouteFp16;
    if (k.prefilter != 1) return r;
    long long rows = 0, n_pairs = 0, twin_pairs = 0, twin_rows = 0;
    bool bytes = true;
    for (const MsfmRoutePair& q : pairs) {
        if (!q.valid || !q.use) continue;
        bytes = bytes && msfm_byte_pair(q.a_is_u8, q.b_is_u8);
        rows += q.n1 + q.n2;
        n_pairs += 1;
        if (q.a_twin && q.b_twin) twin_pairs += 1, twin_rows += q.n1 + q.n2;
    }
    if (bytes) {   // (also a sub-batch without prefiltered pairs: nothing is swept)
        r.kind = kRouteI8;
        return r;
    }
    // Route Q: a pair takes it when both its images have twins; a sub-batch in which only SOME pairs do runs two first sweeps (fine twins,
    // a quarter of the rows or more with twins) or keeps the fp16 route for all (coarse twins: plan A and sweep 1' cover whole sub-batches).
    // Two plans and three sweeps only pay on real images: small ones -- the pre-emptive filter's 100-row subsets -- need q8_route == 2.
    const bool fine = msfm_fine_twins(k), mixed = twin_pairs < n_pairs;
    bool q8 = msfm_twin_route_on(k) && (!mixed || (fine && twin_pairs > 0 && 4 * twin_rows >= rows));
    if (q8 && k.q8_route < 2 && (twin_pairs == 0 || twin_rows < 2 * 1024 * twin_pairs)) q8 = false;
    if (q8) {
        r.kind = mixed ? kRouteQ8Mixed : (fine ? kRouteQ8Direct : kRouteQ8Refine);
        for (std::size_t p = 0; p < pairs.size(); ++p) r.twin[p] = pairs[p].valid && pairs[p].use && pairs[p].a_twin && pairs[p].b_twin;
        return r;
    }
    // One pair that cannot take an integer route sends all of them to the fp16 kernels (~1.6 x the sweep time): counted, so that a mixed
    // store shows up in the profile.  (Each pair's own n1 + n2 >= 2048 here, while the decision above takes the mean over the twin pairs.)
    for (const MsfmRoutePair& q : pairs)
        if (q.valid && q.use && (msfm_byte_pair(q.a_is_u8, q.b_is_u8) ||
                                 (k.q8_route && q.a_twin && q.b_twin && (k.q8_route == 2 || q.n1 + q.n2 >= 2048))))
            r.demoted_pairs += 1;
    return r;
}

// What msfm_pair_scratch_bytes charges one pair for (route code 0 - 4), before the sub-batch -- and with it its route -- exists.
inline int msfm_scratch_route(const MsfmRouteKnobs& k, int prune, float ratio, bool use, bool a_is_u8, bool b_is_u8) {
    if (!use || k.prefilter == 0) return 0;
    if (!msfm_compact_sweep2(prune, ratio)) return 2;
    if (k.prefilter == 1 && msfm_byte_pair(a_is_u8, b_is_u8)) return 3;
    // (every prefiltered non-byte pair counts as route 4 when the context's twins are coarse, even a pair without twins)
    if (msfm_twin_route_on(k) && k.q8_level > 0.f && !msfm_fine_twins(k)) return 4;
    return 1;
}

// Room for the device-side plan of sweep 2 (compacted rows, candidate entries, work items) of a sub-batch that could compact `ub` rows at
// most, in `groups` groups of at most `max_ranges` ranges -- MatchJob sizes the buffers BEFORE the plan exists.  The prediction is what
// the previous sub-batch needed (hint_*), scaled by the ratio of the two upper bounds and void beyond a factor two: the parts of a call and
// the calls of a repeated job are alike, a call of another kind (the pre-emptive filter's 100-row subsets before the full images) says
// nothing.  Without one: `prior_16ths` / 16 of the rows (5 on the direct routes, 2.5 -> the caller passes rows_ub_all_bits * 5 / 32 as
// `ub_prior`), and all rows for a small sub-batch (up to 2 M rows = 0.25 GB of plan buffers: on 100-row subsets more than half stay alive).
// A buffer that EXISTS (have_*) is kept as long as it holds the prediction + 1/8, a fresh one gets 1.5 x the prediction: growing means
// replacing the buffer.  (Round 5, first half: absolute hints -- the buffers kept from the small call counted as large enough for the
// large call's first sub-batch, whose plan then overflowed: profiles/r05_cli_cold_call.txt.)
struct MsfmPlanRoom { long long rows, cand, items; bool hinted; };
inline MsfmPlanRoom msfm_plan_room(long long ub, long long ub_prior, long long groups, long long max_ranges, int wg_rows,
                                   long long hint_ub, long long hint_rows, long long hint_cand, long long hint_items,
                                   long long have_rows, long long have_cand, long long have_items) {
    auto mx = [](long long a, long long b) { return a > b ? a : b; };
    const long long slack = (long long)wg_rows * groups + wg_rows;
    const bool hinted = hint_rows > 0 && hint_ub > 0 && ub <= 2 * hint_ub && 2 * ub >= hint_ub;
    const double s = hinted ? (double)ub / (double)hint_ub : 0.0;
    const long long h_rows = (long long)((double)hint_rows * s), h_cand = (long long)((double)hint_cand * s), h_items = (long long)((double)hint_items * s);
    const long long prior = mx(ub_prior, ub < (1LL << 21) ? ub : (1LL << 21));
    const long long rows_min = (hinted ? h_rows + h_rows / 8 : prior) + slack;
    MsfmPlanRoom r;
    r.hinted = hinted;
    r.rows = have_rows >= rows_min ? have_rows : mx(h_rows + h_rows / 2, prior) + slack;
    // (per group: 8 entries per compacted row rounded up to 1024, + 1024 -- plan_group_cap_units)
    const long long cand_min = mx(8 * rows_min + 2048 * groups, h_cand);
    r.cand = have_cand >= cand_min ? have_cand : mx(8 * r.rows + 2048 * groups, h_cand);
    // (the list holds 8 x the longest per-XCD sub-list: twice the balanced size leaves room for skew)
    const long long items_min = mx(2 * ((rows_min / wg_rows + groups) * max_ranges + 64) / 8 * 8, (h_items + 64) / 8 * 8);
    r.items = have_items >= items_min ? have_items : mx(2 * ((r.rows / wg_rows + groups) * max_ranges + 64) / 8 * 8, (h_items + 64) / 8 * 8);
    return r;
}

// Where the page-locked piece of a call's result lists that holds byte `off` ends (GrowPinned, msfm_ctx.hip.h): the first 32 MiB are cut
// 1, 1, 2, 4, 8, 16 MiB, then 32-MiB pieces -- page-locking costs 0.2 ms per MiB, and a small call's lists should cost a small piece.
inline unsigned long long msfm_pinned_piece_end(unsigned long long off) {
    const unsigned long long piece = 32ull << 20;
    if (off >= piece) return (off / piece + 1) * piece;
    unsigned long long end = 1ull << 20;
    while (end <= off) end *= 2;
    return end;
}

// One key into a slot's (best, second) -- the reduction of the exact re-check (pf_exact_candidates_kernel).  best ends as the
// smallest key the slot ever saw, second as the second smallest DISTINCT key: every key but the final minimum loses exactly once
// against `best` (when it arrives, or when a smaller one displaces it) and is then offered to `second`; a key arriving twice meets
// itself and is dropped.  seen_best / seen_second: what a plain load saw in the two words some time BEFORE (any earlier state: the
// words only ever decrease, so a stale look is >= the truth): a key that does not beat what was seen cannot change the word and
// skips the atomic -- most candidates of a row do.  amin(word, key) = atomic minimum returning the old value.  ~0 = "nothing yet".
template <class AtomicMin>
MSFM_HD void msfm_fold_key(unsigned long long* best, unsigned long long* second, unsigned long long key, unsigned long long seen_best,
                           unsigned long long seen_second, AtomicMin amin) {
    if (key == seen_best) return;
    unsigned long long loser = key;
    if (key < seen_best) {
        const unsigned long long old = amin(best, key);
        if (old == key) return;
        loser = old > key ? old : key;
        if (loser == ~0ull) return;
    }
    if (loser < seen_second) (void)amin(second, loser);
}

// ---- The order-invariance certificate (msfm_kernels.hip.h states the bound): two conforming fp32 builds of the distance differ by at
// most a relative kOrderEps in any distance they report.
constexpr double kOrderEps = 1.0e-5;
constexpr float kNoNeighbour = 3.402823466e+38f;   // FLT_MAX: batchDistance's initial value -- "fewer than two neighbours"

// ---- The ratio cap of the REVERSE thresholds (match lists with 0 < ratio <= 0.9: msfm_ratio_cap_on).  A column's second neighbour is
// used for one thing only, the Lowe test d0 < ratio * d1; its value is never handed out.  The test -- and its certificate -- is decided
// as soon as every element that can VIOLATE it is known: an element t != best with
//        d0 (1 + e)  >=  ratio d_t (1 - e),      e = kOrderEps, d = the pinned fp32 distances.
// So the threshold that collects a column's candidates need not reach the second neighbour (today's bound), only d0 / ratio -- on real
// correspondences far less.  INVARIANT of the helpers below: every violator t has S~_t <= T (resp. a real distance <= the capped
// bound), and so has the best element itself.  What follows from it (msfm_order_sensitive): if a column ends WITHOUT a second candidate
// no violator exists -- the test passes under every conforming order; a second candidate that was found is >= the true second.
// Where it applies: match lists with 0 < ratio <= kRatioCapMax = 0.9 -- a SUBSET of the compacted sweep 2 (ratio <= 0.95), not all of it.
// The bound itself holds for every ratio < 1; the limit is one of scope.  With capped masks a live column is counted once per block
// that holds a row within d0 / ratio of it, i.e. about once, and the first plan of a fresh context (msfm_plan_room: every row once for
// a small sub-batch) then holds any data whose neighbours are unique.  tests/test_gpu_jobs.py reaches the re-run path of an outgrown
// plan with exactly such data at ratio 0.95, through the uncapped masks; as long as that test stands as it is, ratios in (0.9, 0.95]
// keep the uncapped thresholds (follow-ups).
constexpr float kRatioCapMax = 0.9f;
inline bool msfm_ratio_cap_on(int prune, float ratio) { return prune != 0 && ratio > 0.f && ratio <= kRatioCapMax; }

// Distance space (route Q, direct thresholds).  u0 / u1: upper bounds of the REAL distance of the twins' nearest / second-nearest
// element.  The pinned order is within g = 4e-6 relative of real arithmetic (msfm_kernels.hip.h), so the pinned d0 <= u0 (1 + g) and a
// violator's real distance is <= d_t / (1 - g) <= u0 / ratio * (1 + e)(1 + g) / ((1 - e)(1 - g)) < u0 / ratio * (1 + 2.9e-5): the factor
// 1 + 4 e leaves 1.1e-5 for the three roundings here (2e-7).  The best element: real distance <= u0 (1 + 2 g) < the cap (ratio < 1).
MSFM_HD float msfm_ratio_cap_distance(float u0, float u1, float ratio) {
    const float c = u0 / ratio * (1.f + 4.f * (float)kOrderEps);
    return c < u1 ? c : u1;   // (a NaN keeps u1)
}

// S~ space, fp16 sweep (pf_thresholds_kernel).  s0: the column's smallest S~; eps >= |S~ - S| for every element (S: the pinned order's);
// norms = the column's norm + the other image's largest (the scale of the roundings, as in today's slack).  The best element's
// S <= s0 + eps; a violator's S_t = d_t^2 (1 +- 2^-23: d is a rounded sqrtf) <= S0 / ratio^2 * ((1 + e) / (1 - e))^2 (1 + 3e-7)
// < S0 / ratio^2 * (1 + 4.1e-5) -- the factor 1 + 1e-4 covers it and the four roundings of c; its S~_t <= S_t + eps.
MSFM_HD float msfm_ratio_cap_sweep(float s0, float eps, float norms, float ratio) {
    const float tiny = 1e-5f * (fabsf(s0) + norms);
    const float s0ub = fmaxf(s0 + eps + tiny, 0.f);
    const float c = s0ub / (ratio * ratio) * (1.f + 1e-4f);
    return c + eps + 1e-5f * (fabsf(c) + norms);
}
// Integer sweeps (byte images): S~ <= S <= S~ + eps, all of them integers; the cap is one too.
MSFM_HD float msfm_ratio_cap_sweep_i8(float s0, float eps, float ratio) {
    return ceilf(fmaxf(s0 + eps, 0.f) / (ratio * ratio) * (1.f + 1e-4f)) + eps;
}

// Which rows could come out differently under another conforming evaluation order?  (i0, d0, d1): the row's neighbour and its two
// distances in the pinned order; the derivation is the comment block above order_sensitive (msfm_kernels.hip.h), which calls this.
// d1 == +inf: a capped column without a second candidate -- no element can violate the ratio test under any order (the invariant
// above), and the first neighbour is the same element under every order (a violator-free column has d0 (1 + e) < ratio d_t (1 - e)
// < d_t (1 - e) for all t); what is left is the forward distance cut on d0.
MSFM_HD bool msfm_order_sensitive(int i0, float d0, float d1, float ratio, double max_distance, bool forward) {
    const bool no_violator = d1 == __builtin_huge_valf();
    if (i0 < 0 || !(d1 < kNoNeighbour || no_violator)) return false;   // no match under any order (pruned with margin / < 2 neighbours)
    const double lo0 = (double)d0 * (1.0 - kOrderEps), hi0 = (double)d0 * (1.0 + kOrderEps);
    if (forward && lo0 > max_distance) return false;        // cut by FilterMatchesByDistance whatever the ratio test says
    const bool cut_certified = !forward || hi0 <= max_distance || lo0 > max_distance;
    if (no_violator) return !cut_certified;
    const double lo1 = (double)d1 * (1.0 - kOrderEps), hi1 = (double)d1 * (1.0 + kOrderEps);
    const bool pass = d0 < ratio * d1;
    bool certified;
    if (pass)
        certified = hi0 < (double)ratio * lo1 && hi0 < lo1 && cut_certified;
    else
        certified = lo0 >= (double)ratio * hi1;
    return !certified;
}

// The two-view model selection (msfm_set_model_selection): a pair keeps the homography's list iff the epipolar model (F or E) keeps
// something and nH >= h_ratio * nE -- the reference's Initializer takes F when num_inliers_H / num_inliers_F < 0.7
// (src/Reconstruction/Initializer.cpp:38-66).  One rounded product and an exact compare; nE = 0 keeps the (empty) epipolar list, so
// a pair of 4 .. 6 matches never keeps an unverified 4-point fit.  The device's two_view_select_kernel and the host twin
// (host/GeometricVerification.cpp) both call this.
MSFM_HD bool msfm_select_homography(int n_epipolar, int n_homography, double h_ratio) {
    return n_epipolar > 0 && (double)n_homography >= h_ratio * (double)n_epipolar;
}

// The two-view geometry's test for an initial pair (msfm_set_two_view_geometry): the reference's, in the positive
// (Initializer::RecoverPoseFromFundanmental fails a pair when num_inliers < rel_pose_min_num_inlier || median_tri_angle <
// init_tri_min_angle || ave_tri_angle < init_tri_min_angle || ave_residual > init_tri_max_error,
// src/Reconstruction/Initializer.cpp:400-405).  Exact compares only.  tv_pose_kernel and the host twin (TwoViewGeometry) both call this.
MSFM_HD bool msfm_initial_candidate(int n_triangulated, double median_tri_angle, double mean_tri_angle, double mean_residual,
                                    int min_num_inliers, double tri_max_error, double tri_min_angle) {
    return n_triangulated >= min_num_inliers && median_tri_angle >= tri_min_angle && mean_tri_angle >= tri_min_angle &&
           mean_residual <= tri_max_error;
}
