// msfm_verify_e.hip.h -- the calibrated geometric verification on the device (msfm_set_verification_model(.., 1, camera)):
// 5-point essential-matrix RANSAC in normalised coordinates for every pair of a sub-batch, in place of the F-matrix RANSAC of
// msfm_verify.hip.h, between the match epilogue and the CSR gather.  The arithmetic is msfm_emat.h, shared with the host twin
// (host/GeometricVerification.cpp, EssentialRansacMask): the same bits.
//
// STAGED (msfm_verify_staged.hip.h), in rounds of kVeRound hypotheses with the sample size 5:
//   ve_points_kernel         the normalised, undistorted coordinates of every staged match, once;
//   ve_round_kernel          a workgroup per (listed pair, round) -- a grid of two workgroups per CU walks the list: one lane per
//                            hypothesis solves it with its workspace in LDS, then the pair's matches are staged through LDS in
//                            chunks and each lane counts the inliers of each of its solutions (its count: the largest);
//   ve_mask_compact_kernel   re-solves the winner, picks its best solution (lowest index among equal counts), and compacts the
//                            pair's inliers in order.  No refit (findEssentialMat has none).
//
// LDS, not registers: the solver's 10 x 20 elimination alone is 200 doubles per hypothesis.  ve_round_kernel keeps the
// kWork = 296-double workspace of each of its lanes in LDS, lane-interleaved, beside a 4 KiB match chunk and the per-solution
// counts; the Sturm chain (66 doubles, read on every bisection step) stays in registers.  The workspace sets the round size:
// kVeRound = 32 lanes take 79 KiB, so two workgroups -- two waves on two of the CU's four SIMDs -- fit the 160 KiB of a CU;
// 64 lanes (148 KiB) left one wave per CU and three SIMDs idle, and the solve is latency-bound.  A high-inlier pair
// still stops after one round (the stopping rule needs ~6 hypotheses at 90 % inliers); a low-inlier one runs max_iters / 32 rounds.
#pragma once
#include "msfm_emat.h"
#include "msfm_verify.hip.h"
#include "msfm_verify_staged.hip.h"

namespace msfm {

constexpr int kVeRound = 32;    // hypotheses per round = lanes of a ve_round_kernel workgroup
constexpr int kVeGroupsPerCU = 2;   // ve_round_kernel workgroups resident per CU (LDS-bound)
constexpr int kVeChunk = 128;   // matches staged in LDS at a time (4 double arrays = 4 KiB)

// normalised, undistorted coordinates of every staged match, once
__global__ void ve_points_kernel(const PairDesc* __restrict__ pairs, const VerifyPair* __restrict__ vp, const int* __restrict__ counts,
                                 const int2* __restrict__ st_qt, msfm_emat::Camera cam, double* __restrict__ x1, double* __restrict__ y1,
                                 double* __restrict__ x2, double* __restrict__ y2) {
    MSFM_TAIL_PRIO();
    const PairDesc pd = pairs[blockIdx.x];
    const VerifyPair v = vp[blockIdx.x];
    const int n = counts[blockIdx.x];
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int2 m = st_qt[pd.out_off + i];
        const float2 a = v.k1[m.x], b = v.k2[m.y];
        msfm_emat::undistort(cam, (double)a.x, (double)a.y, &x1[pd.out_off + i], &y1[pd.out_off + i]);
        msfm_emat::undistort(cam, (double)b.x, (double)b.y, &x2[pd.out_off + i], &y2[pd.out_off + i]);
    }
}

// round prm.round of the pairs listed for it (list[(round & 1) * P ..], count[round & 1]): grid = min(P, kVeGroupsPerCU * CUs)
__global__ __launch_bounds__(kVeRound) void ve_round_kernel(const PairDesc* __restrict__ pairs, const int* __restrict__ counts,
                                                            const double* __restrict__ x1, const double* __restrict__ y1,
                                                            const double* __restrict__ x2, const double* __restrict__ y2,
                                                            int* __restrict__ list, int n_pairs, int* __restrict__ hyp_counts,
                                                            StagedParams prm, StagedStats* __restrict__ stats) {
    MSFM_TAIL_PRIO();
    using namespace msfm_emat;
    __shared__ double ws[kWork * kVeRound];
    __shared__ double sx1[kVeChunk], sy1[kVeChunk], sx2[kVeChunk], sy2[kVeChunk];
    __shared__ int sc[kMaxSolutions * kVeRound];
    const int t = threadIdx.x;
    int* count = list + 2 * n_pairs;
    const int listed = count[prm.round & 1];
    const int* mine = list + (prm.round & 1) * n_pairs;
    if (blockIdx.x == 0 && t == 0) count[(prm.round + 1) & 1] = 0;   // (the next round's list: read by the last round, filled after this one)
    const int it = prm.round * kVeRound + t;
    const bool live = it < prm.max_iters;
    unsigned long long solved = 0;
    for (int k = blockIdx.x; k < listed; k += gridDim.x) {   // (uniform over the workgroup)
        const int p = mine[k];
        const int n = counts[p];
        const long long base = pairs[p].out_off;
        int ns = 0;
        if (live) ns = hypothesis<kVeRound>(x1 + base, y1 + base, x2 + base, y2 + base, n, prm.seed, it, ws + t);
        for (int s = 0; s < kMaxSolutions; ++s) sc[s * kVeRound + t] = 0;
        for (int c0 = 0; c0 < n; c0 += kVeChunk) {
            const int m = min(kVeChunk, n - c0);
            __syncthreads();
            for (int i = t; i < m; i += kVeRound) {
                sx1[i] = x1[base + c0 + i];
                sy1[i] = y1[base + c0 + i];
                sx2[i] = x2[base + c0 + i];
                sy2[i] = y2[base + c0 + i];
            }
            __syncthreads();
            for (int s = 0; s < ns; ++s) {
                double E[9];
#pragma unroll
                for (int q = 0; q < 9; ++q) E[q] = ws[(kWsSol + 9 * s + q) * kVeRound + t];
                int c = 0;
                for (int i = 0; i < m; ++i)   // every lane reads the same address: LDS broadcast
                    c += sampson(E, sx1[i], sy1[i], sx2[i], sy2[i]) <= prm.thr2 ? 1 : 0;
                sc[s * kVeRound + t] += c;
            }
        }
        int best = 0;
        for (int s = 0; s < ns; ++s) best = max(best, sc[s * kVeRound + t]);
        if (live) hyp_counts[(long long)p * prm.max_iters + it] = best;
        solved += live ? 1 : 0;
        __syncthreads();   // (the next pair's staging overwrites the chunk)
    }
    if (solved) atomicAdd(&stats->solved, solved);
}

// the winner's best solution, its mask, and the ordered compaction of the pair's staged matches.  One wave per pair.
__global__ __launch_bounds__(64) void ve_mask_compact_kernel(
    const PairDesc* __restrict__ pairs, const int* __restrict__ counts, const int2* __restrict__ st_qt, const float* __restrict__ st_d,
    const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2, const double* __restrict__ y2,
    const int* __restrict__ best_it, StagedParams prm, int2* __restrict__ out_qt, float* __restrict__ out_d, int* __restrict__ out_counts) {
    MSFM_TAIL_PRIO();
    using namespace msfm_emat;
    __shared__ double ws[kWork];
    __shared__ int s_ns, s_best, s_cnt[kMaxSolutions];
    const int p = blockIdx.x;
    const int n = counts[p];
    const long long base = pairs[p].out_off;
    const int tid = threadIdx.x;
    const bool run = n >= 5 && best_it[p] >= 0;
    if (run) {
        if (tid == 0) s_ns = hypothesis<1>(x1 + base, y1 + base, x2 + base, y2 + base, n, prm.seed, best_it[p], ws);
        if (tid < kMaxSolutions) s_cnt[tid] = 0;
        __syncthreads();
        const int ns = s_ns;
        for (int s = 0; s < ns; ++s) {
            double E[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) E[k] = ws[kWsSol + 9 * s + k];
            int c = 0;
            for (int i = tid; i < n; i += 64) c += sampson(E, x1[base + i], y1[base + i], x2[base + i], y2[base + i]) <= prm.thr2 ? 1 : 0;
            atomicAdd(&s_cnt[s], c);
        }
        __syncthreads();
        if (tid == 0) {
            int b = 0;
            for (int s = 1; s < ns; ++s)
                if (s_cnt[s] > s_cnt[b]) b = s;
            s_best = b;
        }
        __syncthreads();
    }
    double E[9];
    if (run)
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = ws[kWsSol + 9 * s_best + k];
    int pos0 = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + tid;
        bool keep = false;
        if (run && i < n) keep = sampson(E, x1[base + i], y1[base + i], x2[base + i], y2[base + i]) <= prm.thr2;
        pos0 = staged_compact_step(keep, i, pos0, base, tid, st_qt, st_d, out_qt, out_d);
    }
    if (tid == 0) out_counts[p] = pos0;
}

}  // namespace msfm
