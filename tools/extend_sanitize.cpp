// A stand-alone driver of the map extension's host twin (csrc/msfm_extend.h, ExtendPoints) for sanitizer builds: a generated ring job
// of 12 images -- tracks of 2 .. 12 views (a track of two elements: one view posed at the triangulation, one new), every fifth with
// one observation moved by 40 px, some tracks inconsistent, image ids 3 i + 1 with the ranks in ANOTHER order than the ids -- whose
// first three images are posed at the triangulation; the rest arrive in three increments (two images, an EMPTY list, the remaining
// seven), after the plain and after the robust triangulation, on both routes.  The pose table and `gained` have exactly one entry per
// rank, records, residuals and bytes exactly one per track / observation: an index by image id or list position where the rank is
// meant, or past a track's own slots, runs off the end.  Prints the counters; exits 1 if nothing was continued or created, if an
// untouched track changed, or if a created track differs from the full triangulation apart from MSFM_TRI_EXTENDED.
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/extend_sanitize.cpp -o extend_sanitize && ./extend_sanitize
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../monocularsfm_amd/csrc/msfm_extend.h"

int main() {
    const int n_img = 12, n_tr = 150;
    const msfm_emat::Camera cam{2500.0, 2400.0, 1536.0, 1152.0, -0.1, 0.02, 1e-3, -5e-4};
    const msfm_tri::Params prm = {6.0, 1.5, 2, 0};
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> box(-1.0, 1.0);
    std::normal_distribution<double> noise(0.0, 1.0);
    std::vector<msfm_pose_rt> truth((size_t)n_img);
    std::vector<int> rank_of((size_t)MSFM_MAX_IMAGES, -1), rank((size_t)n_img);
    for (int i = 0; i < n_img; ++i) {
        const double th = 2.0 * 3.14159265358979323846 * i / 300.0;
        msfm_pose_rt p = {};
        p.valid = 1;
        const double z[3] = {-std::sin(th), 0.0, std::cos(th)}, x[3] = {z[2], 0.0, -z[0]};
        const double R[9] = {x[0], x[1], x[2], 0.0, 1.0, 0.0, z[0], z[1], z[2]};
        for (int k = 0; k < 9; ++k) p.R[k] = R[k];
        p.t[2] = 6.5;
        truth[(size_t)i] = p;
        rank[(size_t)i] = (5 * i + 3) % n_img;   // (5 and 12 are coprime: a permutation)
        rank_of[(size_t)(3 * i + 1)] = rank[(size_t)i];
    }
    std::vector<std::vector<float>> kxy((size_t)n_img, std::vector<float>((size_t)(2 * n_tr), 0.f));   // by rank
    std::vector<int64_t> offsets{0};
    std::vector<int32_t> img, idx;
    std::vector<uint8_t> cons;
    for (int j = 0; j < n_tr; ++j) {
        // track j runs through the images first .. first + len - 1; j % 10 == 9: two elements, the images 2 and 3 (one old, one new)
        const int len = j % 10 == 9 ? 2 : 2 + j % (n_img - 1), first = j % 10 == 9 ? 2 : 0;
        const double X[3] = {box(rng), box(rng), box(rng)};
        for (int i = first; i < first + len; ++i) {
            const msfm_pose_rt& p = truth[(size_t)i];
            const double Y0 = p.R[0] * X[0] + p.R[1] * X[1] + p.R[2] * X[2] + p.t[0], Y1 = p.R[3] * X[0] + p.R[4] * X[1] + p.R[5] * X[2] + p.t[1],
                         Y2 = p.R[6] * X[0] + p.R[7] * X[1] + p.R[8] * X[2] + p.t[2];
            std::vector<float>& k = kxy[(size_t)rank[(size_t)i]];
            k[(size_t)(2 * j)] = (float)(cam.fx * Y0 / Y2 + cam.cx + noise(rng) + ((j % 5 == 0 && i == first + (j / 5) % len) ? 40.0 : 0.0));
            k[(size_t)(2 * j + 1)] = (float)(cam.fy * Y1 / Y2 + cam.cy + noise(rng));
            img.push_back(3 * i + 1);
            idx.push_back(j);
        }
        offsets.push_back((int64_t)img.size());
        cons.push_back(j % 11 != 5);
    }
    std::vector<const float*> ptr;
    for (auto& k : kxy) ptr.push_back(k.data());
    const std::vector<std::vector<int>> increments = {{3, 4}, {}, {5, 6, 7, 8, 9, 10, 11}};
    long long continued = 0, created = 0;
    bool bad = false;
    for (int robust = 0; robust < 2; ++robust)
        for (int max_hyp : {0, 16}) {
            std::vector<msfm_tri::Pose> table((size_t)n_img);
            const msfm_pose_rt none = {};
            for (auto& p : table) msfm_tri::prepare_pose(none, &p);
            for (int i = 0; i < 3; ++i) msfm_tri::prepare_pose(truth[(size_t)i], &table[(size_t)rank[(size_t)i]]);
            std::vector<msfm_point3d> pts((size_t)n_tr);
            std::vector<double> res(img.size());
            std::vector<uint8_t> mask(img.size());
            bool have_mask = robust != 0;
            if (robust) {
                msfm_tri::RobustCounts c = {0, 0, 0, 0};
                msfm_tri::TriangulateTracksRobust(offsets.data(), img.data(), idx.data(), cons.data(), 0, n_tr, rank_of.data(), ptr.data(), table.data(),
                                                  cam, msfm_tri::RobustParams{prm.max_error, prm.min_angle, prm.min_views, 64}, pts.data(), res.data(),
                                                  mask.data(), &c);
            } else {
                msfm_tri::TriangulateTracks(offsets.data(), img.data(), idx.data(), cons.data(), 0, n_tr, rank_of.data(), ptr.data(), table.data(), cam,
                                            prm, pts.data(), res.data());
            }
            for (const auto& inc : increments) {
                std::vector<uint8_t> gained((size_t)n_img, 0);
                for (int i : inc) {
                    msfm_tri::prepare_pose(truth[(size_t)i], &table[(size_t)rank[(size_t)i]]);
                    gained[(size_t)rank[(size_t)i]] = 1;
                }
                const std::vector<msfm_point3d> p0 = pts;
                const std::vector<double> r0 = res;
                const std::vector<uint8_t> m0 = mask;
                std::vector<msfm_ext::Trace> trace((size_t)n_tr);
                msfm_ext::Counts c = {0, 0, 0, 0, 0, 0, 0};
                msfm_ext::ExtendPoints(offsets.data(), img.data(), idx.data(), cons.data(), 0, n_tr, rank_of.data(), ptr.data(), table.data(),
                                       gained.data(), cam, prm, max_hyp, have_mask, pts.data(), res.data(), mask.data(), &c, trace.data());
                // the full triangulation under the enlarged table, for the created tracks
                std::vector<msfm_point3d> fp((size_t)n_tr);
                std::vector<double> fr(img.size());
                std::vector<uint8_t> fm(img.size());
                msfm_tri::RobustCounts fc = {0, 0, 0, 0};
                if (max_hyp)
                    msfm_tri::TriangulateTracksRobust(offsets.data(), img.data(), idx.data(), cons.data(), 0, n_tr, rank_of.data(), ptr.data(),
                                                      table.data(), cam, msfm_tri::RobustParams{prm.max_error, prm.min_angle, prm.min_views, max_hyp},
                                                      fp.data(), fr.data(), fm.data(), &fc);
                else
                    msfm_tri::TriangulateTracks(offsets.data(), img.data(), idx.data(), cons.data(), 0, n_tr, rank_of.data(), ptr.data(), table.data(),
                                                cam, prm, fp.data(), fr.data());
                for (int t = 0; t < n_tr; ++t) {
                    const size_t b = (size_t)offsets[(size_t)t], n = (size_t)offsets[(size_t)t + 1] - b;
                    if (trace[(size_t)t].kind == msfm_ext::KIND_UNTOUCHED) {
                        bad = bad || std::memcmp(&pts[(size_t)t], &p0[(size_t)t], sizeof(msfm_point3d)) || std::memcmp(&res[b], &r0[b], n * sizeof(double)) ||
                              (have_mask && std::memcmp(&mask[b], &m0[b], n));
                    } else if (trace[(size_t)t].kind == msfm_ext::KIND_CREATE) {
                        msfm_point3d r = pts[(size_t)t];
                        bad = bad || !(r.status & MSFM_TRI_EXTENDED);
                        r.status &= ~MSFM_TRI_EXTENDED;
                        bad = bad || std::memcmp(&r, &fp[(size_t)t], sizeof(msfm_point3d)) || std::memcmp(&res[b], &fr[b], n * sizeof(double)) ||
                              (max_hyp && std::memcmp(&mask[b], &fm[b], n));
                    } else {
                        bad = bad || (pts[(size_t)t].status & p0[(size_t)t].status) != p0[(size_t)t].status ||
                              std::memcmp(pts[(size_t)t].X, p0[(size_t)t].X, sizeof(double) * 3);
                    }
                }
                std::printf("robust %d max_hypotheses %2d +%zu images: touched %lld continued %lld added %lld rejected %lld created %lld of %lld retried %lld\n",
                            robust, max_hyp, inc.size(), c.tracks_touched, c.continued, c.observations_added, c.observations_rejected, c.created,
                            c.created_attempted, c.retried);
                bad = bad || (inc.empty() && c.tracks_touched != 0);
                continued += c.continued;
                created += c.created;
                have_mask = true;
            }
        }
    return continued > 0 && created > 0 && !bad ? 0 : 1;
}
