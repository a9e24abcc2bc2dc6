// msfm_verify_h.hip.h -- the homography verification on the device (msfm_set_verification_model(.., 2, NULL)): 4-point
// homography RANSAC in pixel coordinates for every pair of a sub-batch, in place of the F-matrix RANSAC of msfm_verify.hip.h, for
// planar scenes and rotation-only views, where an epipolar model is degenerate.  The arithmetic is msfm_hmat.h, shared with the
// host twin (host/GeometricVerification.cpp, HomographyRansacMask): the same bits.
//
// STAGED (msfm_verify_staged.hip.h), in rounds of kVhRound hypotheses with the sample size 4:
//   vf_points_kernel          (msfm_verify.hip.h) the pixel coordinates of every staged match, once;
//   vh_round_kernel           a wave per (listed pair, round) -- a persistent grid of kVhGroupsPerCU waves per CU walks the list:
//                             one lane per hypothesis samples, checks and solves it in registers, then the pair's matches are staged
//                             through LDS in chunks and each lane counts its inliers;
//   vh_mask_compact_kernel    every lane of a wave re-solves the winner (the same bits in each) and the pair's inliers are
//                             compacted in order into the second staging buffer.
//
// Registers, not LDS: the 8 x 9 system is 72 doubles, and with every loop of msfm_hmat::four_point unrolled each index is a
// compile-time constant, so the solve lives in VGPRs with no scratch (DESIGN.md 11 quotes tools/kernel_resources.py).  The round is
// one full wave, kVhRound = 64: the solve uses no LDS, so occupancy is set by the VGPRs alone, and 32 lanes would leave half of each
// wave idle.  A high-inlier pair stops in round 0 (the stopping rule needs ~5 hypotheses at 90 % inliers, ~34 at 60 %); a
// low-inlier one runs max_iters / 64 rounds.
#pragma once
#include "msfm_hmat.h"
#include "msfm_verify.hip.h"
#include "msfm_verify_staged.hip.h"

namespace msfm {

constexpr int kVhRound = 64;        // hypotheses per round = lanes of a vh_round_kernel workgroup (one wave)
constexpr int kVhGroupsPerCU = 8;   // vh_round_kernel waves resident per CU in the persistent grid (two per SIMD)
constexpr int kVhChunk = 256;       // matches staged in LDS at a time (4 float arrays = 4 KiB)

// round prm.round of the pairs listed for it (list[(round & 1) * P ..], count[round & 1]): grid = min(P, kVhGroupsPerCU * CUs).
// prm.thr2 is the squared pixel threshold.
__global__ __launch_bounds__(kVhRound) void vh_round_kernel(const PairDesc* __restrict__ pairs, const int* __restrict__ counts,
                                                            const float* __restrict__ x1, const float* __restrict__ y1,
                                                            const float* __restrict__ x2, const float* __restrict__ y2,
                                                            int* __restrict__ list, int n_pairs, int* __restrict__ hyp_counts,
                                                            StagedParams prm, StagedStats* __restrict__ stats) {
    MSFM_TAIL_PRIO();
    __shared__ float sx1[kVhChunk], sy1[kVhChunk], sx2[kVhChunk], sy2[kVhChunk];
    const int t = threadIdx.x;
    int* count = list + 2 * n_pairs;
    const int listed = count[prm.round & 1];
    const int* mine = list + (prm.round & 1) * n_pairs;
    if (blockIdx.x == 0 && t == 0) count[(prm.round + 1) & 1] = 0;   // (the next round's list: read by the last round, filled after this one)
    const int it = prm.round * kVhRound + t;
    const bool live = it < prm.max_iters;
    unsigned long long solved = 0;
    for (int k = blockIdx.x; k < listed; k += gridDim.x) {   // (uniform over the workgroup)
        const int p = mine[k];
        const int n = counts[p];
        const long long base = pairs[p].out_off;
        double H[9];
        const bool ok = live && msfm_hmat::hypothesis(x1 + base, y1 + base, x2 + base, y2 + base, n, prm.seed, it, H);
        int c = 0;
        for (int c0 = 0; c0 < n; c0 += kVhChunk) {
            const int m = min(kVhChunk, n - c0);
            __syncthreads();
            for (int i = t; i < m; i += kVhRound) {
                sx1[i] = x1[base + c0 + i];
                sy1[i] = y1[base + c0 + i];
                sx2[i] = x2[base + c0 + i];
                sy2[i] = y2[base + c0 + i];
            }
            __syncthreads();
            if (ok)
                for (int i = 0; i < m; ++i)   // every lane reads the same address: LDS broadcast
                    c += msfm_hmat::reproj_error(H, sx1[i], sy1[i], sx2[i], sy2[i]) <= prm.thr2 ? 1 : 0;
        }
        if (live) hyp_counts[(long long)p * prm.max_iters + it] = c;
        solved += live ? 1 : 0;
        __syncthreads();   // (the next pair's staging overwrites the chunk)
    }
    if (solved) atomicAdd(&stats->solved, solved);
}

// the winner's mask and the ordered compaction of the pair's staged matches.  One wave per pair; every lane solves the winner.
__global__ __launch_bounds__(64) void vh_mask_compact_kernel(
    const PairDesc* __restrict__ pairs, const int* __restrict__ counts, const int2* __restrict__ st_qt, const float* __restrict__ st_d,
    const float* __restrict__ x1, const float* __restrict__ y1, const float* __restrict__ x2, const float* __restrict__ y2,
    const int* __restrict__ best_it, StagedParams prm, int2* __restrict__ out_qt, float* __restrict__ out_d, int* __restrict__ out_counts) {
    MSFM_TAIL_PRIO();
    const int p = blockIdx.x;
    const int n = counts[p];
    const long long base = pairs[p].out_off;
    const int tid = threadIdx.x;
    const int bi = best_it[p];
    double H[9];
    const bool run = n >= 4 && bi >= 0 && msfm_hmat::hypothesis(x1 + base, y1 + base, x2 + base, y2 + base, n, prm.seed, bi, H);
    int pos0 = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + tid;
        bool keep = false;
        if (run && i < n) keep = msfm_hmat::reproj_error(H, x1[base + i], y1[base + i], x2[base + i], y2[base + i]) <= prm.thr2;
        pos0 = staged_compact_step(keep, i, pos0, base, tid, st_qt, st_d, out_qt, out_d);
    }
    if (tid == 0) out_counts[p] = pos0;
}

}  // namespace msfm
