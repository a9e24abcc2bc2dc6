// A stand-alone driver of the pose refinement's host twin (csrc/msfm_refine_poses.h, RefinePoses) for sanitizer builds: the corrupted
// ring scene of refine_points_sanitize.cpp with 2 px of noise -- tracks of 3 .. 130 views, every third with one observation moved by
// 40 px, every seventh image unposed, some tracks inconsistent -- with every posed image but the first turned by 1 mrad; the poses are
// refined after the plain and after the robust triangulation with max_iters 0, 1, 10 and 100, min_observations 3 and 15, one image
// fixed, alternating with the point refinement, with the trace.  The pose list is NOT in rank order and shorter than the declared set
// (position k holds image (37 k + 11) mod 130, every 13th position left out), and the records and the trace hold exactly one entry per
// listed image: an index by rank where the list position is meant runs off their end.  A second scene has nearly coincident points
// (1e-9 apart): ill-conditioned systems, LM runs to max_iters.  Prints the counters; exits 1 if nothing was refined or a cost rose.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/refine_poses_sanitize.cpp -o refine_poses_sanitize && ./refine_poses_sanitize
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../monocularsfm_amd/csrc/msfm_refine_poses.h"

static int scene(bool coincident, long long* refined_out) {
    const int n_img = 130, n_tr = 240;
    const msfm_emat::Camera cam{2500.0, 2400.0, 1536.0, 1152.0, -0.1, 0.02, 1e-3, -5e-4};
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> box(-1.0, 1.0);
    std::normal_distribution<double> noise(0.0, 2.0);
    std::vector<msfm_tri::Pose> poses((size_t)n_img);
    std::vector<int> rank_of((size_t)MSFM_MAX_IMAGES, -1);
    for (int i = 0; i < n_img; ++i) {
        const double th = 2.0 * 3.14159265358979323846 * i / 300.0;
        msfm_pose_rt p = {};
        p.valid = i % 7 != 3;
        const double z[3] = {-std::sin(th), 0.0, std::cos(th)}, x[3] = {z[2], 0.0, -z[0]};
        const double R[9] = {x[0], x[1], x[2], 0.0, 1.0, 0.0, z[0], z[1], z[2]};
        for (int k = 0; k < 9; ++k) p.R[k] = R[k];
        p.t[2] = 6.5;
        msfm_tri::prepare_pose(p, &poses[(size_t)i]);
        rank_of[(size_t)(3 * i + 1)] = i;
    }
    std::vector<std::vector<float>> kxy((size_t)n_img, std::vector<float>((size_t)(2 * n_tr), 0.f));
    std::vector<int64_t> offsets{0};
    std::vector<int32_t> img, idx;
    std::vector<uint8_t> cons;
    for (int j = 0; j < n_tr; ++j) {
        const int len = j % 40 == 0 ? n_img : 3 + j % 9;
        const double X[3] = {coincident ? 0.1 + 1e-9 * box(rng) : box(rng), coincident ? -0.2 + 1e-9 * box(rng) : box(rng),
                             coincident ? 0.05 + 1e-9 * box(rng) : box(rng)};
        for (int i = 0; i < len; ++i) {
            const msfm_tri::Pose& p = poses[(size_t)i];
            const double Y0 = p.R[0] * X[0] + p.R[1] * X[1] + p.R[2] * X[2] + p.t[0], Y1 = p.R[3] * X[0] + p.R[4] * X[1] + p.R[5] * X[2] + p.t[1],
                         Y2 = p.R[6] * X[0] + p.R[7] * X[1] + p.R[8] * X[2] + p.t[2];
            kxy[(size_t)i][(size_t)(2 * j)] = (float)(cam.fx * Y0 / Y2 + cam.cx + noise(rng) + ((j % 3 == 0 && i == (j / 3) % len) ? 40.0 : 0.0));
            kxy[(size_t)i][(size_t)(2 * j + 1)] = (float)(cam.fy * Y1 / Y2 + cam.cy + noise(rng));
            img.push_back(3 * i + 1);
            idx.push_back(j);
        }
        offsets.push_back((int64_t)img.size());
        cons.push_back(j % 11 != 5);
    }
    std::vector<const float*> ptr;
    for (auto& k : kxy) ptr.push_back(k.data());
    std::vector<msfm_tri::Pose> bad = poses;   // every posed image but the first: turned by 1 mrad about y, moved by 0.005
    for (int i = 1; i < n_img; ++i) {
        if (!bad[(size_t)i].valid) continue;
        const double a = (i % 2 ? 1e-3 : -1e-3), c = std::cos(a), s = std::sin(a);
        msfm_tri::Pose& p = bad[(size_t)i];
        for (int k = 0; k < 3; ++k) {
            const double r0 = p.R[k], r2 = p.R[6 + k];
            p.R[k] = c * r0 + s * r2;
            p.R[6 + k] = -s * r0 + c * r2;
        }
        p.t[0] += 0.005;
        msfm_tri::centre(p.R, p.t, p.O);
    }
    std::vector<int> list_rank;
    std::vector<int32_t> list_ids;
    for (int k = 0; k < n_img; ++k) {
        if (k % 13 == 12) continue;
        const int i = (37 * k + 11) % n_img;   // (37 and 130 are coprime: every image at most once)
        list_rank.push_back(i);
        list_ids.push_back(3 * i + 1);
    }
    const int n_list = (int)list_rank.size();
    std::vector<uint8_t> fixed((size_t)n_img, 0), changed((size_t)n_img, 0);
    fixed[0] = 1;
    long long refined = 0;
    bool rose = false;
    for (int robust = 0; robust < 2; ++robust) {
        std::vector<msfm_tri::Pose> cur = bad;
        std::vector<msfm_point3d> pts((size_t)n_tr);
        std::vector<double> res(img.size());
        std::vector<uint8_t> mask(img.size());
        if (robust) {
            msfm_tri::RobustCounts c = {0, 0, 0, 0};
            msfm_tri::TriangulateTracksRobust(offsets.data(), img.data(), idx.data(), cons.data(), 0, n_tr, rank_of.data(), ptr.data(), cur.data(),
                                              cam, msfm_tri::RobustParams{12.0, 1.5, 3, 64}, pts.data(), res.data(), mask.data(), &c);
        } else {
            msfm_tri::TriangulateTracks(offsets.data(), img.data(), idx.data(), cons.data(), 0, n_tr, rank_of.data(), ptr.data(), cur.data(), cam,
                                        msfm_tri::Params{12.0, 1.5, 3, 0}, pts.data(), res.data());
        }
        int round = 0;
        for (int max_iters : {0, 1, 10, 10, 100}) {   // (each call refines from what the one before left)
            const int min_obs = round++ % 2 ? 3 : 15;
            std::vector<msfm_ref::Trace> trace((size_t)n_list);
            std::vector<msfm_pose_refinement> rec((size_t)n_list);
            msfm_rp::Counts c = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0};
            msfm_rp::RefinePoses(offsets.data(), img.data(), idx.data(), n_tr, rank_of.data(), ptr.data(), cur.data(), n_img,
                                 robust ? mask.data() : nullptr, cam, msfm_ref::Verdict{12.0, 1.5}, msfm_rp::Params{1e-6, max_iters, min_obs},
                                 list_rank.data(), list_ids.data(), n_list, fixed.data(), pts.data(), res.data(), rec.data(), changed.data(), &c,
                                 trace.data());
            long long steps = 0;
            for (const auto& t : trace) steps += t.steps;
            std::printf("coincident %d robust %d max_iters %3d min_observations %2d: eligible %lld refined %lld rejected_by_inliers %lld iterations %lld observations %lld "
                        "reposed %lld lost %lld gained %lld cost %.6f -> %.6f\n",
                        (int)coincident, robust, max_iters, min_obs, c.eligible, c.refined, c.rejected_by_inliers, c.iterations, c.observations, c.points_reposed,
                        c.points_lost, c.points_gained, c.cost_before, c.cost_after);
            refined += c.refined;
            rose = rose || !(c.cost_after <= c.cost_before) || steps != c.iterations;
            msfm_ref::Counts pc = {0, 0, 0, 0, 0, 0.0, 0.0};   // the other half of the alternation
            msfm_ref::RefinePoints(offsets.data(), img.data(), idx.data(), 0, n_tr, rank_of.data(), ptr.data(), cur.data(),
                                   robust ? mask.data() : nullptr, cam, msfm_ref::Verdict{12.0, 1.5}, msfm_ref::Params{1e-6, 5, 0}, pts.data(),
                                   res.data(), &pc);
        }
    }
    *refined_out += refined;
    return rose ? 1 : 0;
}

int main() {
    long long refined = 0;
    const int rose = scene(false, &refined) + scene(true, &refined);
    return refined > 0 && !rose ? 0 : 1;
}
