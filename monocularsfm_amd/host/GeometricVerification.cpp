#include "GeometricVerification.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../csrc/msfm_emat.h"
#include "../csrc/msfm_fmat.h"
#include "../csrc/msfm_hmat.h"
#include "../csrc/msfm_hostutil.h"
#include "../csrc/msfm_pose.h"
#include "../csrc/msfm_pose_refine.h"

namespace MonocularSfM {

// Host twin of the batched device RANSAC (csrc/msfm_verify.hip.h): same sampling, same solver, same error
// measure, same adaptive stopping rule, all through the shared fp64 arithmetic of msfm_fmat.h -- the two give
// identical masks, which is what tests/test_gpu_verify.py checks.  The product path (ComputeMatches) runs the
// device version; this one is the test oracle and serves callers without a device context.
std::vector<unsigned char> FundamentalRansacMask(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2,
                                                 double threshold, double confidence, int max_iters,
                                                 unsigned long long seed) {
    using namespace msfm_fmat;
    const int n = (int)pts1.size();
    if (n < 7) return {};
    if (n == 7) return std::vector<unsigned char>(7, 1);
    std::vector<float> x1((size_t)n), y1((size_t)n), x2((size_t)n), y2((size_t)n);
    for (int i = 0; i < n; ++i) {
        x1[(size_t)i] = pts1[(size_t)i].x;
        y1[(size_t)i] = pts1[(size_t)i].y;
        x2[(size_t)i] = pts2[(size_t)i].x;
        y2[(size_t)i] = pts2[(size_t)i].y;
    }
    const double thr2 = threshold * threshold;
    auto count_inliers = [&](const double F[9], unsigned char* mask) {
        int count = 0;
        for (int i = 0; i < n; ++i) {
            const bool in = epipolar_error(F, x1[(size_t)i], y1[(size_t)i], x2[(size_t)i], y2[(size_t)i]) <= thr2;
            if (mask) mask[i] = in ? 1 : 0;
            count += in ? 1 : 0;
        }
        return count;
    };
    // lazily evaluated per-hypothesis counts (the replay only asks for it < current iteration bound)
    auto count_at = [&](int it) {
        double F[9];
        if (!hypothesis(x1.data(), y1.data(), x2.data(), y2.data(), n, seed, it, F)) return 0;
        return count_inliers(F, nullptr);
    };
    int best_count = 0;
    const int best_it = replay_adaptive(n, max_iters, confidence, count_at, &best_count);
    std::vector<unsigned char> best((size_t)n, 0);
    if (best_it < 0) return best;
    double F[9];
    hypothesis(x1.data(), y1.data(), x2.data(), y2.data(), n, seed, best_it, F);
    count_inliers(F, best.data());
    // one refit on the consensus set, kept if it does not lose inliers
    std::vector<int> in;
    for (int i = 0; i < n; ++i)
        if (best[(size_t)i]) in.push_back(i);
    const int m = (int)in.size();
    const Norm2D t1 = normalizer(x1.data(), y1.data(), m, [&](int i) { return in[(size_t)i]; });
    const Norm2D t2 = normalizer(x2.data(), y2.data(), m, [&](int i) { return in[(size_t)i]; });
    double M[45] = {0};
    for (int i = 0; i < m; ++i) {
        const size_t k = (size_t)in[(size_t)i];
        moment_add(M, t1, t2, x1[k], y1[k], x2[k], y2[k]);
    }
    if (solve(M, t1, t2, F, kFmatRefitSteps, true)) {
        std::vector<unsigned char> cur((size_t)n);
        const int count = count_inliers(F, cur.data());
        if (count >= best_count) best.swap(cur);
    }
    return best;
}

// The sequential loop of msfm_fmat::replay_adaptive<5> over lazily scored hypotheses: hypothesis it is solved and scored when the
// loop reaches it; its count is the largest over its solutions.  The winning solution (the lowest index among equal counts) gives
// the mask.
// (E_out, xy_out: the winner and the normalised coordinates x1 | y1 | x2 | y2 of every match, for TwoViewGeometry; may be NULL)
static std::vector<unsigned char> essential_ransac(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2,
                                                   const CameraIntrinsics& camera, double threshold, double confidence, int max_iters,
                                                   unsigned long long seed, double* E_out, std::vector<double>* xy_out) {
    using namespace msfm_emat;
    const int n = (int)pts1.size();
    if (n < 5) return {};
    const Camera cam{camera.fx, camera.fy, camera.cx, camera.cy, camera.k1, camera.k2, camera.p1, camera.p2};
    std::vector<double> x1((size_t)n), y1((size_t)n), x2((size_t)n), y2((size_t)n);
    for (size_t i = 0; i < (size_t)n; ++i) {
        undistort(cam, (double)pts1[i].x, (double)pts1[i].y, &x1[i], &y1[i]);
        undistort(cam, (double)pts2[i].x, (double)pts2[i].y, &x2[i], &y2[i]);
    }
    const double f = (camera.fx + camera.fy) * 0.5, t = threshold / f, thr2 = t * t;
    std::vector<double> ws((size_t)kWork);
    // best solution of hypothesis it: its count, and (sol) its index; the solutions stay in ws
    auto score = [&](int it, int* sol) {
        const int ns = hypothesis<1>(x1.data(), y1.data(), x2.data(), y2.data(), n, seed, it, ws.data());
        int best = 0, bs = -1;
        for (int s = 0; s < ns; ++s) {
            const double* E = ws.data() + kWsSol + 9 * s;
            int c = 0;
            for (int i = 0; i < n; ++i) c += sampson(E, x1[(size_t)i], y1[(size_t)i], x2[(size_t)i], y2[(size_t)i]) <= thr2 ? 1 : 0;
            if (bs < 0 || c > best) {
                best = c;
                bs = s;
            }
        }
        if (sol) *sol = bs;
        return best;
    };
    int best_count = 0;
    const int best_it = msfm_fmat::replay_adaptive<5>(n, max_iters, confidence, [&](int it) { return score(it, nullptr); }, &best_count);
    if (best_it < 0) return {};
    int sol;
    score(best_it, &sol);
    std::vector<unsigned char> mask((size_t)n, 0);
    const double* E = ws.data() + kWsSol + 9 * sol;
    for (int i = 0; i < n; ++i) mask[(size_t)i] = sampson(E, x1[(size_t)i], y1[(size_t)i], x2[(size_t)i], y2[(size_t)i]) <= thr2 ? 1 : 0;
    if (E_out) std::copy(E, E + 9, E_out);
    if (xy_out) {
        xy_out->clear();
        for (const std::vector<double>* a : {&x1, &y1, &x2, &y2}) xy_out->insert(xy_out->end(), a->begin(), a->end());
    }
    return mask;
}

std::vector<unsigned char> EssentialRansacMask(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2,
                                               const CameraIntrinsics& camera, double threshold, double confidence,
                                               int max_iters, unsigned long long seed) {
    return essential_ransac(pts1, pts2, camera, threshold, confidence, max_iters, seed, nullptr, nullptr);
}

std::vector<unsigned char> TwoViewGeometry(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2,
                                           const CameraIntrinsics& camera, const msfm_two_view_params& params,
                                           msfm_two_view_record* record, double threshold, double confidence, int max_iters,
                                           unsigned long long seed) {
    double E[9];
    std::vector<double> xy;
    msfm_pose::clear_record(record);
    const std::vector<unsigned char> mask = essential_ransac(pts1, pts2, camera, threshold, confidence, max_iters, seed, E, &xy);
    if (mask.empty()) return mask;
    const size_t n = mask.size();
    std::vector<double> k[4];
    for (size_t i = 0; i < n; ++i)
        if (mask[i])
            for (int c = 0; c < 4; ++c) k[c].push_back(xy[(size_t)c * n + i]);
    msfm_pose::two_view_record(E, k[0].data(), k[1].data(), k[2].data(), k[3].data(), (int)k[0].size(),
                               (camera.fx + camera.fy) * 0.5, params, record);
    return mask;
}

void KeptNormalised(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2, const std::vector<unsigned char>& mask,
                    const CameraIntrinsics& camera, std::vector<double> kept[4]) {
    const msfm_emat::Camera cam{camera.fx, camera.fy, camera.cx, camera.cy, camera.k1, camera.k2, camera.p1, camera.p2};
    for (int c = 0; c < 4; ++c) kept[c].clear();
    for (size_t i = 0; i < mask.size(); ++i) {
        if (!mask[i]) continue;
        double v[4];
        msfm_emat::undistort(cam, (double)pts1[i].x, (double)pts1[i].y, &v[0], &v[1]);
        msfm_emat::undistort(cam, (double)pts2[i].x, (double)pts2[i].y, &v[2], &v[3]);
        for (int c = 0; c < 4; ++c) kept[c].push_back(v[c]);
    }
}

void RefineTwoView(const double* x1, const double* y1, const double* x2, const double* y2, int n, const CameraIntrinsics& camera,
                   const msfm_two_view_params& params, const msfm_two_view_refine_params& refine, msfm_two_view_record* record,
                   msfm_two_view_refinement* refinement) {
    msfm_tvr::refine_record(x1, y1, x2, y2, n, (camera.fx + camera.fy) * 0.5, params, refine, record, refinement);
}

// The sequential loop of msfm_fmat::replay_adaptive<4> over lazily scored hypotheses: hypothesis it is sampled, checked, solved
// and scored when the loop reaches it (a rejected sample counts 0).  The winner's inliers are the mask.
std::vector<unsigned char> HomographyRansacMask(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2,
                                                double threshold, double confidence, int max_iters, unsigned long long seed) {
    using namespace msfm_hmat;
    const int n = (int)pts1.size();
    if (n < 4) return {};
    std::vector<float> x1((size_t)n), y1((size_t)n), x2((size_t)n), y2((size_t)n);
    for (size_t i = 0; i < (size_t)n; ++i) {
        x1[i] = pts1[i].x;
        y1[i] = pts1[i].y;
        x2[i] = pts2[i].x;
        y2[i] = pts2[i].y;
    }
    const double thr2 = threshold * threshold;
    auto count = [&](const double H[9]) {
        int c = 0;
        for (size_t i = 0; i < (size_t)n; ++i) c += reproj_error(H, x1[i], y1[i], x2[i], y2[i]) <= thr2 ? 1 : 0;
        return c;
    };
    auto count_at = [&](int it) {
        double H[9];
        return hypothesis(x1.data(), y1.data(), x2.data(), y2.data(), n, seed, it, H) ? count(H) : 0;
    };
    int best_count = 0;
    const int best_it = msfm_fmat::replay_adaptive<4>(n, max_iters, confidence, count_at, &best_count);
    if (best_it < 0) return {};
    double H[9];
    hypothesis(x1.data(), y1.data(), x2.data(), y2.data(), n, seed, best_it, H);
    std::vector<unsigned char> mask((size_t)n, 0);
    for (size_t i = 0; i < (size_t)n; ++i) mask[i] = reproj_error(H, x1[i], y1[i], x2[i], y2[i]) <= thr2 ? 1 : 0;
    return mask;
}

std::vector<unsigned char> TwoViewSelectMask(const std::vector<Point2f>& pts1, const std::vector<Point2f>& pts2, int model,
                                             const CameraIntrinsics& camera, double h_ratio, double threshold, double confidence,
                                             int max_iters, unsigned long long seed, int* chosen, int* n_epipolar, int* n_homography) {
    std::vector<unsigned char> me = model == MSFM_VERIFY_ESSENTIAL
                                        ? EssentialRansacMask(pts1, pts2, camera, threshold, confidence, max_iters, seed)
                                        : FundamentalRansacMask(pts1, pts2, threshold, confidence, max_iters, seed);
    std::vector<unsigned char> mh = HomographyRansacMask(pts1, pts2, threshold, confidence, max_iters, seed);
    const int ne = (int)std::count(me.begin(), me.end(), (unsigned char)1);
    const int nh = (int)std::count(mh.begin(), mh.end(), (unsigned char)1);
    const bool take_h = msfm_select_homography(ne, nh, h_ratio);
    if (chosen) *chosen = take_h ? MSFM_VERIFY_HOMOGRAPHY : model;
    if (n_epipolar) *n_epipolar = ne;
    if (n_homography) *n_homography = nh;
    return take_h ? mh : me;
}

void FilterMatches(const std::vector<KeyPoint>& kpts1, const std::vector<KeyPoint>& kpts2,
                   const std::vector<DMatch>& matches, std::vector<DMatch>* prune_matches, int model,
                   const CameraIntrinsics& camera, bool model_selection, double h_ratio, int* chosen_model) {
    if (chosen_model) *chosen_model = model;
    if (kpts1.empty() || matches.empty()) return;  // FeatureUtils.cpp:181-184
    std::vector<Point2f> a, b;
    a.reserve(matches.size());
    b.reserve(matches.size());
    for (const DMatch& m : matches) {
        a.push_back(Point2f{kpts1[(size_t)m.queryIdx].x, kpts1[(size_t)m.queryIdx].y});
        b.push_back(Point2f{kpts2[(size_t)m.trainIdx].x, kpts2[(size_t)m.trainIdx].y});
    }
    if (model_selection && model != MSFM_VERIFY_HOMOGRAPHY) {
        const std::vector<unsigned char> mask = TwoViewSelectMask(a, b, model, camera, h_ratio, 3.0, 0.99, 1000, 0x5eed5eedULL, chosen_model);
        for (size_t i = 0; i < mask.size(); ++i)
            if (mask[i]) prune_matches->push_back(matches[i]);
        return;
    }
    const std::vector<unsigned char> mask = model == MSFM_VERIFY_ESSENTIAL    ? EssentialRansacMask(a, b, camera, 3.0, 0.99)
                                            : model == MSFM_VERIFY_HOMOGRAPHY ? HomographyRansacMask(a, b, 3.0, 0.99)
                                                                              : FundamentalRansacMask(a, b, 3.0, 0.99);
    for (size_t i = 0; i < mask.size(); ++i)
        if (mask[i]) prune_matches->push_back(matches[i]);
}

}  // namespace MonocularSfM
