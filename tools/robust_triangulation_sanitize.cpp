// A stand-alone driver of the robust triangulation's host twin (csrc/msfm_triangulate.h, TriangulateTracksRobust) for sanitizer builds:
// one corrupted ring scene -- tracks of 3 .. 130 views, every third with one observation moved by 40 px, every seventh image unposed --
// under enumerated and sampled hypotheses.  Prints the counters; exits 1 if nothing was rescued.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/robust_triangulation_sanitize.cpp -o robust_triangulation_sanitize && ./robust_triangulation_sanitize
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../monocularsfm_amd/csrc/msfm_triangulate.h"

int main() {
    const int n_img = 130, n_tr = 240;
    const msfm_emat::Camera cam{2500.0, 2500.0, 1536.0, 1152.0, -0.1, 0.02, 1e-3, -5e-4};
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> box(-1.0, 1.0);
    std::normal_distribution<double> noise(0.0, 0.3);
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
        const double X[3] = {box(rng), box(rng), box(rng)};
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
    long long rescued = 0;
    for (int max_h : {64, 5, 1024}) {
        std::vector<msfm_point3d> pts((size_t)n_tr);
        std::vector<double> res(img.size());
        std::vector<uint8_t> mask(img.size());
        msfm_tri::RobustCounts c = {0, 0, 0, 0};
        msfm_tri::TriangulateTracksRobust(offsets.data(), img.data(), idx.data(), cons.data(), 0, n_tr, rank_of.data(), ptr.data(), poses.data(),
                                          cam, msfm_tri::RobustParams{2.0, 1.5, 3, max_h}, pts.data(), res.data(), mask.data(), &c);
        std::printf("max_hypotheses %d: retried %lld rescued %lld rejected %lld hypotheses %lld\n", max_h, c.retried, c.rescued,
                    c.observations_rejected, c.hypotheses);
        rescued += c.rescued;
    }
    return rescued > 0 ? 0 : 1;
}
