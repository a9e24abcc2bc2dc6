// msfm_retrieval.h -- the pure policy of vocabulary retrieval (matching mode 2, include/msfm_match.h "retrieval"), shared by the
// device code (csrc/msfm_retrieval.hip.h), the library's host side and the ComputeMatches executable, and compilable on its own
// (tests/test_retrieval_host.py builds a g++ driver around it): the training sample, the effective vocabulary size and the initial
// words, the centroid rounding, the selection key and the top-K of one image, the union of the selections into brute mode's pair
// orientation and order, and the groups the executable writes them in.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSFM_RET_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MSFM_RET_HD inline
#endif

// Training sample of R rows (the call's images by ascending id, rows concatenated) with at most M rows: every s-th row from row 0,
// s = max(1, R / M).  count = Ms, the rows at 0, s, 2s, ... below R, at most M of them.
struct MsfmRetSample {
    int64_t step, count;
};
inline MsfmRetSample msfm_ret_sample(int64_t rows, int64_t max_rows) {
    const int64_t s = std::max<int64_t>(1, max_rows > 0 ? rows / max_rows : 1);
    const int64_t n = rows > 0 ? std::min<int64_t>(max_rows, (rows + s - 1) / s) : 0;
    return MsfmRetSample{s, n};
}
// V' = min(V, max(1, Ms / 8)): at least eight sample rows per word, one word at least
inline int msfm_ret_vocab_size(int num_words, int64_t sample_rows) {
    return (int)std::min<int64_t>(num_words, std::max<int64_t>(1, sample_rows / 8));
}
// the sample row word k starts from: (k Ms) / V' in 64-bit integers
MSFM_RET_HD int64_t msfm_ret_initial_row(int k, int64_t sample_rows, int vocab) { return (int64_t)k * sample_rows / vocab; }
// one dimension of a word with cnt > 0 rows whose values sum to `sum`: the mean rounded half up, floor((2 sum + cnt) / (2 cnt))
MSFM_RET_HD unsigned msfm_ret_centroid(uint64_t sum, uint64_t cnt) { return (unsigned)((2 * sum + cnt) / (2 * cnt)); }

// Selection key of candidate image `id` at score s: larger = earlier.  Only s > 0 is a candidate (key 0 otherwise); equal scores go to
// the lower id.  The bits of a positive float order like the float.
MSFM_RET_HD uint64_t msfm_ret_key(float s, int id) {
    if (!(s > 0.f)) return 0ull;
    unsigned bits;
#if defined(__HIP_DEVICE_COMPILE__)
    bits = __float_as_uint(s);
#else
    std::memcpy(&bits, &s, 4);
#endif
    return ((uint64_t)bits << 32) | (uint64_t)(0xffffffffu - (unsigned)id);
}
MSFM_RET_HD int msfm_ret_key_id(uint64_t key) { return (int)(0xffffffffu - (unsigned)(key & 0xffffffffu)); }

// Image `self` (position in `ids`) takes the first K images j != self with s > 0, by key, highest first: the positions, in order.
inline std::vector<int> msfm_ret_topk(const float* scores_row, const int32_t* ids, int n, int self, int k) {
    std::vector<std::pair<uint64_t, int>> c;
    for (int j = 0; j < n; ++j) {
        const uint64_t key = j == self ? 0ull : msfm_ret_key(scores_row[j], ids[j]);
        if (key) c.emplace_back(key, j);
    }
    const size_t take = std::min(c.size(), (size_t)std::max(0, k));
    std::partial_sort(c.begin(), c.begin() + (long)take, c.end(), [](const std::pair<uint64_t, int>& a, const std::pair<uint64_t, int>& b) { return a.first > b.first; });
    std::vector<int> out;
    for (size_t t = 0; t < take; ++t) out.push_back(c[t].second);
    return out;
}

// The union of the selections (a, b) -- image a took image b -- as brute mode's rows (max id, min id), by first id, then second
inline std::vector<std::pair<int, int>> msfm_ret_union(const std::vector<std::pair<int, int>>& selected) {
    std::vector<std::pair<int, int>> p;
    p.reserve(selected.size());
    for (const auto& s : selected)
        if (s.first != s.second) p.emplace_back(std::max(s.first, s.second), std::min(s.first, s.second));
    std::sort(p.begin(), p.end());
    p.erase(std::unique(p.begin(), p.end()), p.end());
    return p;
}

// Brute mode's groups over the union (BruteFeatureMatcher::RunMatching): row i ascending, j < i ascending, a group ends after every
// `per_group` pairs of a row and at the end of every row.  Returns the end index of every group in `pairs` (sorted as above).
inline std::vector<size_t> msfm_ret_group_ends(const std::vector<std::pair<int, int>>& pairs, int per_group) {
    std::vector<size_t> ends;
    int in_group = 0;
    for (size_t t = 0; t < pairs.size(); ++t) {
        in_group += 1;
        const bool row_ends = t + 1 == pairs.size() || pairs[t + 1].first != pairs[t].first;
        if (in_group == per_group || row_ends) {
            ends.push_back(t + 1);
            in_group = 0;
        }
    }
    return ends;
}
