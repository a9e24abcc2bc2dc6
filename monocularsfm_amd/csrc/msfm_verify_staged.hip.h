// msfm_verify_staged.hip.h -- the staged RANSAC core the essential matrix (msfm_verify_e.hip.h) and the homography
// (msfm_verify_h.hip.h) share.  MatchJob::issue_verify launches, back to back with no host wait in between:
//   the model's points kernel       the coordinates of every staged match, once;
//   staged_decide_kernel, r = -1    every pair with >= kSample matches goes on the list of round 0 (no replay);
//   then for r = 0, 1, ..:
//     the model's round kernel      hypotheses r * kRound .. of every listed pair, one lane each, on a persistent grid that walks
//                                   the list (a round with nothing left costs one short dispatch); the count of hypothesis it of
//                                   pair p lands in hyp_counts[p * max_iters + it];
//     staged_decide_kernel, r       one thread per pair replays the sequential stopping rule (msfm_fmat::replay_adaptive<kSample>)
//                                   over the counts so far, marks the pair decided when the loop ended before it needed a count
//                                   not yet computed, and appends the undecided pairs to the list of the next round;
//   the model's mask kernel         re-solves the winner and compacts the pair's inliers in order (staged_compact_step) into the
//                                   second staging buffer.
// The replay never reads a count beyond its stopping point, so the result equals scoring all max_iters hypotheses; the last round
// reaches max_iters, where every pair is decided.
#pragma once
#include "msfm_fmat.h"
#include "msfm_kernels.hip.h"

namespace msfm {

struct StagedParams {
    double thr2;                // the model's squared threshold (E: normalised, H: pixels)
    double confidence;
    int max_iters;
    int round;
    unsigned long long seed;
};

struct StagedStats {            // per scratch set, zeroed per sub-batch
    unsigned long long solved;  // hypotheses solved
    int rounds;                 // rounds any pair of the sub-batch ran
    int pad;
};

// after round prm.round (-1: before round 0): the stopping rule over the counts so far, and the list of the next round.  One thread
// per pair.  kSample / kRound: 5 / kVeRound for the essential matrix, 4 / kVhRound for the homography.
template <int kSample, int kRound>
__global__ void staged_decide_kernel(const int* __restrict__ counts, const int* __restrict__ hyp_counts, int n_pairs, StagedParams prm,
                                     int* __restrict__ state, int* __restrict__ list, int* __restrict__ best_it, int* __restrict__ best_count,
                                     StagedStats* __restrict__ stats) {
    MSFM_TAIL_PRIO();
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs || state[p] != 0) return;
    const int n = counts[p];
    if (n < kSample) {
        state[p] = 1;
        best_it[p] = -1;
        best_count[p] = 0;
        return;
    }
    if (prm.round >= 0) {
        const int avail = min((prm.round + 1) * kRound, prm.max_iters);
        const int* hc = hyp_counts + (long long)p * prm.max_iters;
        int bc = 0;
        bool decided = false;
        const int bi = msfm_fmat::replay_adaptive<kSample>(n, prm.max_iters, prm.confidence, [&](int it) { return hc[it]; }, &bc, avail, &decided);
        if (decided) {
            state[p] = 1;
            best_it[p] = bi;
            best_count[p] = bc;
            atomicMax(&stats->rounds, prm.round + 1);
            return;
        }
    }
    const int nxt = (prm.round + 1) & 1;
    const int k = atomicAdd(&list[2 * n_pairs + nxt], 1);
    list[nxt * n_pairs + k] = p;
}

// one step of the ordered compaction of a pair's staged matches by a single wave (the one of vf_mask_compact_kernel): lane tid's
// match i goes behind the pos0 already kept and the kept lanes below it.  Returns the new pos0.
__device__ __forceinline__ int staged_compact_step(bool keep, int i, int pos0, long long base, int tid, const int2* st_qt,
                                                   const float* st_d, int2* out_qt, float* out_d) {
    const unsigned long long bal = __ballot(keep);
    const int pos = pos0 + __popcll(bal & ((1ull << tid) - 1ull));
    if (keep) {
        out_qt[base + pos] = st_qt[base + i];
        out_d[base + pos] = st_d[base + i];
    }
    return pos0 + __popcll(bal);
}

}  // namespace msfm
