// msfm_verify_pose_refine.hip.h -- the two-view pose refinement on the device (msfm_set_two_view_refinement): the pose of every valid
// two-view record with enough kept matches is polished by Levenberg-Marquardt on the Sampson error over ALL the pair's kept matches
// (msfm_pose_refine.h, shared with the host twin RefineTwoView: the same bits).  MatchJob::issue_verify launches tv_refine_kernel on
// the sub-batch's stream directly behind tv_pose_kernel, with no host wait.  It reads what that kernel left in the sub-batch's scratch:
// the kept list in the pair's index slot, the normalised coordinates, the record; the angle slot is overwritten (it is never exported).
//
// tv_refine_kernel, one workgroup of msfm_tvr::kLanes = 256 threads per pair, a grid of kTvrGroupsPerCU workgroups per CU walking the
// sub-batch's pairs.  EVERY thread runs the same msfm_ref::lm_minimise on the same bits, so the control flow is uniform over the
// workgroup (rp_image_kernel's lanes do the same within a wave); the problem's cost and linearise are workgroup reductions through LDS
// in the stated order: each thread's partial over the kept list strided by 256, then the fixed tree, kTvrChunk sums at a time (the 21
// sums of a linearisation in three trees of 7: 14 KiB of LDS instead of 42).  The statistics under the final pose are tv_pose_kernel's
// steps 5 and 6 (tv_statistics, one copy for both kernels).  Thread 0 writes the refinement record and, iff the refined record
// stands, the record.  Plain vector loads and stores, no floating-point atomics; integer LDS atomics where tv_pose_kernel has them
// (the counts, the radix histogram).
#pragma once
#include "msfm_pose_refine.h"
#include "msfm_verify_pose.hip.h"

namespace msfm {

constexpr int kTvrThreads = msfm_tvr::kLanes;
constexpr int kTvrChunk = 7;          // sums reduced by one tree
// tv_refine_kernel workgroups per CU, from the compiler's resource report: 256 VGPRs + 52 AGPRs, no scratch -- one wave per
// SIMD.  (Bounded to two waves the compiler keeps 256 registers and spills 95 to 216 B of scratch per lane: every thread holds the 54
// uniform entries of E and its five derivatives through the pass over its matches.)
constexpr int kTvrGroupsPerCU = 1;
static_assert(kTvrThreads == kTvThreads, "tv_statistics and tv_select are written for the workgroup of tv_pose_kernel");
static_assert(msfm_tvr::kSums % kTvrChunk == 0, "whole chunks");

// the reduced passes of one pair on the device (msfm_tvr::refine_pair's `ev`); every thread of the workgroup calls every member
struct TvrDeviceEval {
    const double *x1, *y1, *x2, *y2;   // the pair's slots
    const int* idx;
    double* angles;
    int n, tid;
    double f, tri_max_error;
    double* s_red;   // kTvrChunk * kTvrThreads doubles of LDS
    int* s_hist;
    unsigned long long* s_sel;
    int* s_cnt;      // n_triangulated, n_positive_depth

    // the tree over `m` arrays of partials in s_red; on return every thread has passed a barrier behind the last add
    __device__ __forceinline__ void tree(int m) const {
        __syncthreads();
        for (int s = kTvrThreads / 2; s >= 1; s >>= 1) {
            if (tid < s)
                for (int k = 0; k < m; ++k) s_red[k * kTvrThreads + tid] = s_red[k * kTvrThreads + tid] + s_red[k * kTvrThreads + tid + s];
            __syncthreads();
        }
    }
    __device__ __forceinline__ double cost(const msfm_tvr::State& s) const {
        double E[9];
        msfm_tvr::cross_mat(s.t, s.R, E);
        s_red[tid] = msfm_tvr::lane_cost(E, f, x1, y1, x2, y2, idx, n, tid);
        tree(1);
        const double c = s_red[0];
        __syncthreads();   // (s_red is rewritten by the next pass)
        return c;
    }
    __device__ __forceinline__ void sums(const msfm_tvr::State& s, double acc[msfm_tvr::kSums]) const {
        double E[9], D[5][9], part[msfm_tvr::kSums];
        msfm_tvr::linear_model(s, E, D);
        msfm_tvr::lane_sums(E, D, f, x1, y1, x2, y2, idx, n, tid, part);
#pragma unroll
        for (int c0 = 0; c0 < msfm_tvr::kSums; c0 += kTvrChunk) {
#pragma unroll
            for (int k = 0; k < kTvrChunk; ++k) s_red[k * kTvrThreads + tid] = part[c0 + k];
            tree(kTvrChunk);
#pragma unroll
            for (int k = 0; k < kTvrChunk; ++k) acc[c0 + k] = s_red[k * kTvrThreads];
            __syncthreads();
        }
    }
    __device__ __forceinline__ void stats(const double P[12], msfm_tvr::Stats* st) const {
        if (tid < 2) s_cnt[tid] = 0;
        __syncthreads();
        double lo, hi;
        tv_statistics<true>(P, f, tri_max_error, x1, y1, x2, y2, idx, angles, n, s_red, s_red + kTvrThreads, s_hist, s_sel, &s_cnt[0],
                            &s_cnt[1], tid, &lo, &hi);
        *st = msfm_tvr::Stats{s_cnt[1], s_cnt[0], s_red[0], s_red[kTvrThreads], lo, hi};
        __syncthreads();   // (s_red and the counts are rewritten by the next pair)
    }
};

// idx / angles: tv_pose_kernel's slots, addressed by PairDesc::out_off; records: read, and rewritten where the refined record stands
__global__ __launch_bounds__(kTvrThreads) void tv_refine_kernel(
    const PairDesc* __restrict__ pairs, const double* __restrict__ x1, const double* __restrict__ y1, const double* __restrict__ x2,
    const double* __restrict__ y2, const int* __restrict__ idx, double focal, msfm_two_view_params tp, msfm_two_view_refine_params rp,
    int n_pairs, double* __restrict__ angles, msfm_two_view_record* records, msfm_two_view_refinement* __restrict__ refinements) {
    MSFM_TAIL_PRIO();
    __shared__ double s_red[kTvrChunk * kTvrThreads];
    __shared__ int s_hist[256];
    __shared__ unsigned long long s_sel[2];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x;
    for (int p = blockIdx.x; p < n_pairs; p += gridDim.x) {   // (uniform over the workgroup)
        const msfm_two_view_record old = records[p];
        const long long base = pairs[p].out_off;
        const TvrDeviceEval ev{x1 + base, y1 + base, x2 + base, y2 + base, idx + base, angles + base, old.n_kept, tid, focal,
                               tp.tri_max_error, s_red, s_hist, s_sel, s_cnt};
        msfm_two_view_record rec;
        msfm_two_view_refinement rf;
        const bool stands = msfm_tvr::refine_pair(ev, rp, tp, old, &rec, &rf);
        __syncthreads();   // (every thread has read the old record)
        if (tid == 0) {
            refinements[p] = rf;
            if (stands) records[p] = rec;
        }
    }
}

}  // namespace msfm
