// msfm_verify_pose.hip.h -- the two-view geometry on the device (msfm_set_two_view_geometry): per verified pair of model 1 the
// relative pose from the winning E, the triangulation statistics over the pair's kept matches and the reference's test for an
// initial pair (msfm_pose.h, shared with the host twin TwoViewGeometry: the same bits).  MatchJob::issue_verify launches
// tv_pose_kernel behind ve_mask_compact_kernel and, under the model selection, behind two_view_select_kernel (it reads which list
// was kept), on the sub-batch's stream, with no host wait.  No existing kernel changes: the winner is re-solved here from best_it
// the way two_view_select_kernel re-solves the homography's (under the selection best_it is saved first: the homography's rounds
// reuse the buffer).
//
// tv_pose_kernel, one workgroup of msfm_pose::kLanes = 256 threads per pair, a grid of kTvGroupsPerCU workgroups per CU walking the
// sub-batch's pairs:
//   1  thread 0 re-solves hypothesis best_it (workspace in LDS); all threads count the inliers of each solution; the best one
//      (the lowest index among equal counts) is E -- ve_mask_compact_kernel's choice;
//   2  wave 0 writes the staged indices of the E-inliers, in order, to the pair's index slot: the kept list;
//   3  thread 0 decomposes E into the four candidates (LDS);
//   4  pass 1: the threads stride over the kept list, triangulate each match under the four candidates and count the matches in
//      front of both cameras (wave ballots, one LDS atomic per wave and candidate); the winner;
//   5  pass 2 under the winner: error, depth test, angle; the angle goes to the pair's angle slot, the two sums are reduced in
//      msfm_pose.h's stated order (per-thread partial sums strided by kLanes, then the fixed tree in LDS);
//   6  the exact median: an MSB-first radix selection (8 bits a pass, LDS histogram) over the fp64 bit patterns of the slot's
//      non-negative angles -- once for an odd nE, twice (both middle ranks) for an even one.
//   (5 and 6 are tv_statistics below: tv_refine_kernel, msfm_verify_pose_refine.hip.h, calls the same function under its final pose.)
// SELECTION ALWAYS, no LDS sort: the slot has just been written by the same CU (L2 / L1 resident), nE spans 5 .. ~8000 and a pair of
// 350 kept matches reads its slot in 2 loads per thread and pass; one path for every size, 10.1 KiB of LDS (10 328 B) whatever nE is, so the
// LDS never limits the residency (the registers do: DESIGN.md 13).
#pragma once
#include "msfm_pose.h"
#include "msfm_verify_e.hip.h"
#include "msfm_verify_select.hip.h"

namespace msfm {

constexpr int kTvThreads = msfm_pose::kLanes;
constexpr int kTvGroupsPerCU = 1;   // tv_pose_kernel workgroups per CU: its 376 VGPRs (the re-solve of the winner) leave one wave per SIMD

// the value of rank k (0-based, ascending) among the n non-negative doubles of `a`.  Every thread of the workgroup calls it and gets
// the value.  hist: 256 ints, s_sel: 2 words of LDS.
__device__ __forceinline__ double tv_select(const double* a, int n, int k, int* hist, unsigned long long* s_sel, int tid) {
    unsigned long long prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        static_assert(kTvThreads == 256, "one thread clears one of the 256 bins of a radix pass");
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += kTvThreads) {
            const unsigned long long key = (unsigned long long)__double_as_longlong(a[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int d = 0, before = 0;
            for (; d < 255; ++d) {
                const int c = hist[d];
                if (before + c > k) break;
                before += c;
            }
            s_sel[0] = (unsigned long long)d;
            s_sel[1] = (unsigned long long)(k - before);
        }
        __syncthreads();
        prefix |= s_sel[0] << shift;
        mask |= 255ull << shift;
        k = (int)s_sel[1];
        __syncthreads();
    }
    return __longlong_as_double((long long)prefix);
}

// Steps 5 and 6 of tv_pose_kernel, shared with tv_refine_kernel (msfm_verify_pose_refine.hip.h): under the pose P = R[9] | t[3] every
// thread of the workgroup strides over the pair's kept list (x1 .. angles: the pair's slots), the angle of every kept match goes to the
// angle slot, the two sums are reduced in msfm_pose.h's stated order into part_r[0] / part_a[0], *n_tri counts the triangulated matches
// and, with kCountDepth, *n_pos those in front of both cameras (one LDS atomic per thread that has any: both must be 0 and visible on
// entry); lo / hi: the two middle angles by the radix selection.  Every thread returns behind a barrier with the same values.
template <bool kCountDepth>
__device__ __forceinline__ void tv_statistics(const double* P, double focal, double tri_max_error, const double* x1, const double* y1,
                                              const double* x2, const double* y2, const int* idx, double* angles, int nk, double* part_r_s,
                                              double* part_a_s, int* hist, unsigned long long* s_sel, int* n_tri_s, int* n_pos_s, int tid,
                                              double* lo_out, double* hi_out) {
    double part_r = 0.0, part_a = 0.0;
    int n_tri = 0, n_pos = 0;
    for (int j = tid; j < nk; j += kTvThreads) {
        const int i = idx[j];
        bool depth;
        double err, ang;
        msfm_pose::evaluate(P, focal, x1[i], y1[i], x2[i], y2[i], &depth, &err, &ang);
        angles[j] = ang;
        if (kCountDepth) n_pos += depth ? 1 : 0;
        if (depth && err < tri_max_error) {
            n_tri += 1;
            part_r = part_r + err;
            part_a = part_a + ang;
        }
    }
    part_r_s[tid] = part_r;
    part_a_s[tid] = part_a;
    if (n_tri) atomicAdd(n_tri_s, n_tri);
    if (kCountDepth && n_pos) atomicAdd(n_pos_s, n_pos);
    __syncthreads();   // (also: the angle slot is visible to the workgroup)
    for (int s = kTvThreads / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            part_r_s[tid] = part_r_s[tid] + part_r_s[tid + s];
            part_a_s[tid] = part_a_s[tid] + part_a_s[tid + s];
        }
        __syncthreads();
    }
    const double hi = tv_select(angles, nk, nk / 2, hist, s_sel, tid);
    *lo_out = (nk & 1) ? hi : tv_select(angles, nk, (nk - 1) / 2, hist, s_sel, tid);
    *hi_out = hi;
}

// counts: the staged counts; best_it: the E winners; sel: the selection's records or NULL; idx / angles: slots of the staged lists'
// size, addressed by PairDesc::out_off
__global__ __launch_bounds__(kTvThreads) void tv_pose_kernel(
    const PairDesc* __restrict__ pairs, const int* __restrict__ counts, const double* __restrict__ x1, const double* __restrict__ y1,
    const double* __restrict__ x2, const double* __restrict__ y2, const int* __restrict__ best_it, const SelectRecord* __restrict__ sel,
    StagedParams prm, double focal, msfm_two_view_params tp, int n_pairs, int* __restrict__ idx, double* __restrict__ angles,
    msfm_two_view_record* __restrict__ records) {
    MSFM_TAIL_PRIO();
    using namespace msfm_emat;
    // (stride 2: an instantiation of the solver of its own, so that the code of the kernels that share hypothesis<1> is compiled as
    // it was before this kernel existed)
    constexpr int kS = 2;
    __shared__ double ws[kS * kWork];
    __shared__ double s_cand[48];
    __shared__ double s_part_r[kTvThreads], s_part_a[kTvThreads];
    __shared__ int s_hist[256];
    __shared__ unsigned long long s_sel[2];
    __shared__ int s_ns, s_cnt[kMaxSolutions], s_front[4], s_nkept, s_ok, s_ntri;
    const int tid = threadIdx.x;
    for (int p = blockIdx.x; p < n_pairs; p += gridDim.x) {   // (uniform over the workgroup)
        __syncthreads();   // (the pair before has been written)
        const int n = counts[p];
        const long long base = pairs[p].out_off;
        const int bi = best_it[p];
        const bool run = n >= 5 && bi >= 0 && (!sel || sel[p].model == MSFM_VERIFY_ESSENTIAL);
        if (!run) {
            if (tid == 0) msfm_pose::clear_record(&records[p]);
            continue;
        }
        // 1: the winning E
        if (tid == 0) s_ns = hypothesis<kS>(x1 + base, y1 + base, x2 + base, y2 + base, n, prm.seed, bi, ws);
        if (tid < kMaxSolutions) s_cnt[tid] = 0;
        if (tid < 4) s_front[tid] = 0;
        if (tid == 0) s_ntri = 0;
        __syncthreads();
        const int ns = s_ns;
        for (int s = 0; s < ns; ++s) {
            double Es[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) Es[k] = ws[(kWsSol + 9 * s + k) * kS];
            int c = 0;
            for (int i = tid; i < n; i += kTvThreads) c += sampson(Es, x1[base + i], y1[base + i], x2[base + i], y2[base + i]) <= prm.thr2 ? 1 : 0;
            if (c) atomicAdd(&s_cnt[s], c);
        }
        __syncthreads();
        int sb = 0;
        for (int s = 1; s < ns; ++s)
            if (s_cnt[s] > s_cnt[sb]) sb = s;
        double E[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = ns > 0 ? ws[(kWsSol + 9 * sb + k) * kS] : 0.0;
        // 2: the kept list, in order (wave 0); 3: the candidates (thread 0 first)
        if (tid == 0) s_ok = ns > 0 && msfm_pose::decompose<1>(E, s_cand) ? 1 : 0;
        if (tid < 64) {
            int pos0 = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + tid;
                const bool keep = ns > 0 && i < n && sampson(E, x1[base + i], y1[base + i], x2[base + i], y2[base + i]) <= prm.thr2;
                const unsigned long long bal = __ballot(keep);
                if (keep) idx[base + pos0 + __popcll(bal & ((1ull << tid) - 1ull))] = i;
                pos0 += __popcll(bal);
            }
            if (tid == 0) s_nkept = pos0;
        }
        __syncthreads();
        const int nk = s_nkept;
        if (!s_ok || nk < 1) {
            if (tid == 0) msfm_pose::clear_record(&records[p]);
            continue;
        }
        // 4: cheirality under the four candidates
        for (int j0 = 0; j0 < nk; j0 += kTvThreads) {
            const int j = j0 + tid;
            const bool live = j < nk;
            const int i = live ? idx[base + j] : 0;
            const double a = x1[base + i], b = y1[base + i], c = x2[base + i], d = y2[base + i];
#pragma nounroll
            for (int k = 0; k < 4; ++k) {
                const bool front = live && msfm_pose::in_front(s_cand + 12 * k, a, b, c, d);
                const int cnt = __popcll(__ballot(front));
                if ((tid & 63) == 0 && cnt) atomicAdd(&s_front[k], cnt);
            }
        }
        __syncthreads();
        int w = 0;
        for (int k = 1; k < 4; ++k)
            if (s_front[k] > s_front[w]) w = k;
        const int n_front = s_front[w];
        if (n_front == 0) {
            if (tid == 0) msfm_pose::clear_record(&records[p]);
            continue;
        }
        // 5 and 6: the per-match quantities under the winner, the two sums, the median (tv_statistics)
        const double* P = s_cand + 12 * w;
        double lo, hi;
        tv_statistics<false>(P, focal, tp.tri_max_error, x1 + base, y1 + base, x2 + base, y2 + base, idx + base, angles + base, nk, s_part_r,
                             s_part_a, s_hist, s_sel, &s_ntri, nullptr, tid, &lo, &hi);
        if (tid == 0) msfm_pose::finish_record<1>(P, nk, n_front, s_ntri, s_part_r[0], s_part_a[0], lo, hi, tp, &records[p]);
    }
}

}  // namespace msfm
