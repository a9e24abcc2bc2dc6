// msfm_verify_select.hip.h -- the two-view model selection (msfm_set_model_selection): every verified pair runs the context's
// epipolar model (F or E) AND the homography on the same staged matches, and keeps one of the two lists by msfm_select_homography
// (msfm_hostutil.h).  MatchJob::issue_verify launches, behind the epipolar path and with no host wait:
//   vf_points_kernel          (model 1 only: under model 0 the F path has written the pixel coordinates already)
//   the staged H RANSAC       staged_decide_kernel<4, kVhRound> / vh_round_kernel (msfm_verify_h.hip.h), unchanged;
//   two_view_select_kernel    one wave per pair: re-solves the H winner (the same bits as vh_mask_compact_kernel), counts its mask
//                             (nH, exactly what model 2 keeps), reads nE from the epipolar list's count, applies the rule; an H pair's
//                             inliers are compacted in order from the FIRST staging buffer over its epipolar list in the second one.
// So every pair's list is bit for bit the model 0 / 1 list or the model 2 list of the same call parameters.  The record
// {model, nE, nH} of each pair goes to the host with the sub-batch's other end words (queue_tail_copies).
#pragma once
#include "msfm_hostutil.h"
#include "msfm_verify_h.hip.h"

namespace msfm {

struct SelectRecord {   // per pair: the model whose list was kept (MSFM_VERIFY_*), nE, nH
    int model;
    int n_epipolar;
    int n_homography;
};

// prm: the homography's StagedParams; best_it: its winners (staged_decide_kernel<4, kVhRound>); out_counts holds the epipolar counts
// on entry.
__global__ __launch_bounds__(64) void two_view_select_kernel(
    const PairDesc* __restrict__ pairs, const int* __restrict__ counts, const int2* __restrict__ st_qt, const float* __restrict__ st_d,
    const float* __restrict__ x1, const float* __restrict__ y1, const float* __restrict__ x2, const float* __restrict__ y2,
    const int* __restrict__ best_it, StagedParams prm, int epipolar_model, double h_ratio, int2* __restrict__ out_qt,
    float* __restrict__ out_d, int* out_counts, SelectRecord* __restrict__ records) {
    MSFM_TAIL_PRIO();
    const int p = blockIdx.x;
    const int n = counts[p];
    const long long base = pairs[p].out_off;
    const int tid = threadIdx.x;
    const int bi = best_it[p];
    const int ne = out_counts[p];
    double H[9];
    const bool run = n >= 4 && bi >= 0 && msfm_hmat::hypothesis(x1 + base, y1 + base, x2 + base, y2 + base, n, prm.seed, bi, H);
    int nh = 0;
    if (run)
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + tid;
            const bool keep = i < n && msfm_hmat::reproj_error(H, x1[base + i], y1[base + i], x2[base + i], y2[base + i]) <= prm.thr2;
            nh += __popcll(__ballot(keep));
        }
    const bool take_h = msfm_select_homography(ne, nh, h_ratio);
    if (take_h) {   // (nh > 0, so run)
        int pos0 = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + tid;
            bool keep = false;
            if (run && i < n) keep = msfm_hmat::reproj_error(H, x1[base + i], y1[base + i], x2[base + i], y2[base + i]) <= prm.thr2;
            pos0 = staged_compact_step(keep, i, pos0, base, tid, st_qt, st_d, out_qt, out_d);
        }
    }
    if (tid == 0) {
        if (take_h) out_counts[p] = nh;
        records[p] = SelectRecord{take_h ? 2 : epipolar_model, ne, nh};
    }
}

}  // namespace msfm
