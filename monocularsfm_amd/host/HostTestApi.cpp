// HostTestApi.cpp -- C-linkage shims over the host-only pieces (YAML reader, Database, F-, E- and H-RANSAC)
// so that the CPU test-suite can exercise them through ctypes without a GPU.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "Database.h"
#include "GeometricVerification.h"
#include "HostTwinMap.h"
#include "MatchEmission.h"
#include "YamlConfig.h"
#include "../csrc/msfm_emat.h"
#include "../csrc/msfm_fmat.h"
#include "../csrc/msfm_hmat.h"
#include "../csrc/msfm_hostutil.h"
#include "../csrc/msfm_pose.h"
#include "../csrc/msfm_pose_refine.h"
#include "../csrc/msfm_tracks.h"
#include "../csrc/msfm_triangulate.h"
#include "../csrc/msfm_refine.h"
#include "../csrc/msfm_refine_poses.h"
#include "../csrc/msfm_refine_camera.h"
#include "../csrc/msfm_extend.h"
#include "../csrc/msfm_filter.h"
#include "../csrc/msfm_complete.h"
#include "../csrc/msfm_visibility.h"
#include "../csrc/msfm_align.h"
#include "../csrc/msfm_register.h"

using namespace MonocularSfM;

extern "C" {

int host_yaml_is_opened(const char* path) {
    msfm_host::YamlConfig y;
    y.Open(path);
    return y.isOpened() ? 1 : 0;
}

int host_yaml_get_string(const char* path, const char* key, char* out, int cap) {
    msfm_host::YamlConfig y;
    if (!y.Open(path)) return -1;
    std::string v;
    y.Get(key, &v);
    std::strncpy(out, v.c_str(), (size_t)cap - 1);
    out[cap - 1] = 0;
    return y.Has(key) ? 1 : 0;
}

double host_yaml_get_double(const char* path, const char* key, double dflt) {
    msfm_host::YamlConfig y;
    y.Open(path);
    double v = dflt;
    y.Get(key, &v);
    return v;
}

int host_yaml_get_int(const char* path, const char* key, int dflt) {
    msfm_host::YamlConfig y;
    y.Open(path);
    int v = dflt;
    y.Get(key, &v);
    return v;
}

int host_yaml_get_bool(const char* path, const char* key, int dflt) {
    msfm_host::YamlConfig y;
    y.Open(path);
    bool v = dflt != 0;
    y.Get(key, &v);
    return v ? 1 : 0;
}

int host_db_num_images(const char* path) {
    Database db;
    db.Open(path);
    const int n = (int)db.ReadAllImages().size();
    db.Close();
    return n;
}

// returns rows; copies min(rows*cols, cap) floats
int host_db_read_descriptors(const char* path, int image_id, float* out, long long cap, int* cols) {
    Database db;
    db.Open(path);
    const Descriptors d = db.ReadDescriptors(image_id);
    db.Close();
    *cols = d.cols;
    const long long n = std::min<long long>((long long)d.data.size(), cap);
    if (n > 0) std::memcpy(out, d.data.data(), (size_t)n * 4);
    return d.rows;
}

int host_db_read_keypoints(const char* path, int image_id, float* out, long long cap) {
    Database db;
    db.Open(path);
    const std::vector<KeyPoint> k = db.ReadKeyPoints(image_id);
    db.Close();
    const long long n = std::min<long long>((long long)k.size() * 4, cap);
    if (n > 0) std::memcpy(out, k.data(), (size_t)n * 4);
    return (int)k.size();
}

int host_db_write_matches(const char* path, int id1, int id2, const int* qt, int m) {
    Database db;
    db.Open(path);
    std::vector<DMatch> ms((size_t)m);
    for (int i = 0; i < m; ++i) {
        ms[(size_t)i].queryIdx = qt[2 * i];
        ms[(size_t)i].trainIdx = qt[2 * i + 1];
    }
    db.BeginTransaction();
    db.WriteMatches(id1, id2, ms);
    db.EndTransaction();
    db.Close();
    return 0;
}

int host_db_exist_matches(const char* path, int id1, int id2) {
    Database db;
    db.Open(path);
    const int e = db.ExistMatches(id1, id2) ? 1 : 0;
    db.Close();
    return e;
}

// returns m; writes (queryIdx, trainIdx) pairs as seen from (id1, id2)
int host_db_read_matches(const char* path, int id1, int id2, int* qt, int cap_pairs) {
    Database db;
    db.Open(path);
    const std::vector<DMatch> ms = db.ReadMatches(id1, id2);
    db.Close();
    for (size_t i = 0; i < ms.size() && (int)i < cap_pairs; ++i) {
        qt[2 * i] = ms[i].queryIdx;
        qt[2 * i + 1] = ms[i].trainIdx;
    }
    return (int)ms.size();
}

int host_pair_id(int id1, int id2) { return Database::ImagePairToPairId(id1, id2); }

// ---- bulk loader + u8 side table --------------------------------------------------------------------
int host_db_write_descriptors_u8(const char* path, int image_id, const unsigned char* data, int rows, int cols) {
    Database db;
    db.Open(path);
    db.CreateDescriptorsU8Table();
    db.BeginTransaction();
    db.WriteDescriptorsU8(image_id, data, (size_t)rows, (size_t)cols);
    db.EndTransaction();
    db.Close();
    return 0;
}

// One sweep over a table (which: 0 descriptors, 1 keypoints, 2 descriptors_u8): per row image id, rows, cols, a checksum
// of the blob bytes; returns the number of rows visited (-1: the u8 side table does not exist).
int host_db_visit_all(const char* path, int which, int* ids, int* rows, int* cols, unsigned long long* checksums, int cap) {
    struct Acc {
        int *ids, *rows, *cols;
        unsigned long long* sums;
        int cap, n;
    } acc{ids, rows, cols, checksums, cap, 0};
    auto visit = [](void* user, image_t id, const void* data, size_t r, size_t c, size_t elem) {
        Acc* a = static_cast<Acc*>(user);
        if (a->n < a->cap) {
            unsigned long long h = 1469598103934665603ull;   // FNV-1a over the blob
            const unsigned char* b = static_cast<const unsigned char*>(data);
            for (size_t i = 0; i < r * c * elem; ++i) h = (h ^ b[i]) * 1099511628211ull;
            a->ids[a->n] = (int)id;
            a->rows[a->n] = (int)r;
            a->cols[a->n] = (int)c;
            a->sums[a->n] = h;
        }
        a->n += 1;
    };
    Database db;
    db.Open(path);
    size_t n = 0;
    if (which == 2 && !db.HasDescriptorsU8()) {
        db.Close();
        return -1;
    }
    if (which == 0) n = db.VisitAllDescriptors(visit, &acc);
    else if (which == 1) n = db.VisitAllKeyPoints(visit, &acc);
    else n = db.VisitAllDescriptorsU8(visit, &acc);
    db.Close();
    return (int)n;
}

// ---- row emission -------------------------------------------------------------------------------------
// in / out: m (queryIdx, trainIdx) pairs of pair (id1, id2); returns the new count
int host_apply_emission(int id1, int id2, int scene_graph_order, int min_num_matches, int* qt, int m) {
    std::vector<DMatch> ms((size_t)m);
    for (int i = 0; i < m; ++i) {
        ms[(size_t)i].queryIdx = qt[2 * i];
        ms[(size_t)i].trainIdx = qt[2 * i + 1];
    }
    EmissionOptions o;
    o.scene_graph_order = scene_graph_order != 0;
    o.min_num_matches = min_num_matches;
    ApplyEmissionOptions(o, id1, id2, &ms);
    for (size_t i = 0; i < ms.size(); ++i) {
        qt[2 * i] = ms[i].queryIdx;
        qt[2 * i + 1] = ms[i].trainIdx;
    }
    return (int)ms.size();
}

int host_check_row_contract(const int* qt, int m, int num_keypoints1, int num_keypoints2) {
    std::vector<DMatch> ms((size_t)m);
    for (int i = 0; i < m; ++i) {
        ms[(size_t)i].queryIdx = qt[2 * i];
        ms[(size_t)i].trainIdx = qt[2 * i + 1];
    }
    return CheckRowContract(ms, (size_t)num_keypoints1, (size_t)num_keypoints2);
}

// mask length n (0/1); returns number of mask entries written (0 if no model)
int host_fundamental_ransac(const float* p1, const float* p2, int n, unsigned char* mask) {
    std::vector<Point2f> a((size_t)n), b((size_t)n);
    for (int i = 0; i < n; ++i) {
        a[(size_t)i] = Point2f{p1[2 * i], p1[2 * i + 1]};
        b[(size_t)i] = Point2f{p2[2 * i], p2[2 * i + 1]};
    }
    const std::vector<unsigned char> m = FundamentalRansacMask(a, b);
    for (size_t i = 0; i < m.size(); ++i) mask[i] = m[i];
    return (int)m.size();
}

// the same with every RANSAC parameter explicit
int host_fundamental_ransac_ex(const float* p1, const float* p2, int n, double threshold, double confidence, int max_iters,
                               unsigned long long seed, unsigned char* mask) {
    std::vector<Point2f> a((size_t)n), b((size_t)n);
    for (int i = 0; i < n; ++i) {
        a[(size_t)i] = Point2f{p1[2 * i], p1[2 * i + 1]};
        b[(size_t)i] = Point2f{p2[2 * i], p2[2 * i + 1]};
    }
    const std::vector<unsigned char> m = FundamentalRansacMask(a, b, threshold, confidence, max_iters, seed);
    for (size_t i = 0; i < m.size(); ++i) mask[i] = m[i];
    return (int)m.size();
}

// ---- the pieces of msfm_fmat.h, one by one (tests/test_fmat_reference.py compares them with oracle/fmat_ref.py) ------
void host_fmat_sample8(unsigned long long seed, int it, int n, int* idx) { msfm_fmat::sample8(seed, it, n, idx); }

int host_fmat_hypothesis(const float* x1, const float* y1, const float* x2, const float* y2, int n, unsigned long long seed,
                         int it, double* F) {
    return msfm_fmat::hypothesis(x1, y1, x2, y2, n, seed, it, F) ? 1 : 0;
}

// the consensus refit of FundamentalRansacMask: normaliser over the masked points, moments in index order, solve
int host_fmat_refit(const float* x1, const float* y1, const float* x2, const float* y2, int n, const unsigned char* mask,
                    double* F) {
    using namespace msfm_fmat;
    std::vector<int> in;
    for (int i = 0; i < n; ++i)
        if (mask[i]) in.push_back(i);
    const int m = (int)in.size();
    if (m == 0) return 0;
    const Norm2D t1 = normalizer(x1, y1, m, [&](int i) { return in[(size_t)i]; });
    const Norm2D t2 = normalizer(x2, y2, m, [&](int i) { return in[(size_t)i]; });
    double M[45] = {0};
    for (int k : in) moment_add(M, t1, t2, x1[k], y1[k], x2[k], y2[k]);
    return solve(M, t1, t2, F, kFmatRefitSteps, true) ? 1 : 0;
}

double host_fmat_epipolar_error(const double* F, float ax, float ay, float bx, float by) {
    return msfm_fmat::epipolar_error(F, ax, ay, bx, by);
}

double host_fmat_det_log(double x) { return msfm_fmat::det_log(x); }

int host_fmat_replay(const int* counts, int n_counts, int n, int max_iters, double confidence, int* best_count) {
    return msfm_fmat::replay_adaptive(n, max_iters, confidence, [&](int it) { return it < n_counts ? counts[it] : 0; },
                                      best_count);
}

// inlier count of every hypothesis 0 .. max_iters-1 (0 where the solve fails), as the device computes them
void host_fmat_counts(const float* x1, const float* y1, const float* x2, const float* y2, int n, unsigned long long seed,
                      int max_iters, double thr2, int* out_counts) {
    for (int it = 0; it < max_iters; ++it) {
        double F[9];
        int c = 0;
        if (msfm_fmat::hypothesis(x1, y1, x2, y2, n, seed, it, F))
            for (int i = 0; i < n; ++i) c += msfm_fmat::epipolar_error(F, x1[i], y1[i], x2[i], y2[i]) <= thr2 ? 1 : 0;
        out_counts[it] = c;
    }
}

// ---- the pieces of msfm_emat.h (tests/test_emat_reference.py compares them with tests/emat_ref.py) -------------------------
// cam: fx fy cx cy k1 k2 p1 p2
void host_emat_undistort(const double* cam, const double* uv, int n, double* xy) {
    const msfm_emat::Camera c{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6], cam[7]};
    for (int i = 0; i < n; ++i) msfm_emat::undistort(c, uv[2 * i], uv[2 * i + 1], &xy[2 * i], &xy[2 * i + 1]);
}

void host_emat_sample5(unsigned long long seed, int it, int n, int* idx) { msfm_emat::sample5(seed, it, n, idx); }

// q1, q2: 5 x 2 normalised points; E: room for 10 x 9; roots: room for 10.  Returns the number of solutions.
int host_emat_five_point(const double* q1, const double* q2, double* E, double* roots) {
    double ws[msfm_emat::kWork];
    double a[5], b[5], c[5], d[5];
    for (int k = 0; k < 5; ++k) {
        a[k] = q1[2 * k];
        b[k] = q1[2 * k + 1];
        c[k] = q2[2 * k];
        d[k] = q2[2 * k + 1];
    }
    const int ns = msfm_emat::five_point<1>(a, b, c, d, ws);
    for (int s = 0; s < ns; ++s) {
        for (int k = 0; k < 9; ++k) E[9 * s + k] = ws[msfm_emat::kWsSol + 9 * s + k];
        roots[s] = ws[msfm_emat::kWsRoots + s];
    }
    return ns;
}

double host_emat_sampson(const double* E, double x1, double y1, double x2, double y2) {
    return msfm_emat::sampson(E, x1, y1, x2, y2);
}

// replay_adaptive<5> over counts [0, avail); *decided = 0 when it needed more
int host_emat_replay(const int* counts, int avail, int n, int max_iters, double confidence, int* best_count, int* decided) {
    bool dec = true;
    const int r = msfm_fmat::replay_adaptive<5>(n, max_iters, confidence, [&](int it) { return counts[it]; }, best_count, avail, &dec);
    *decided = dec ? 1 : 0;
    return r;
}

// count of every hypothesis 0 .. max_iters-1 (largest over its solutions) and the solution that reaches it (-1: none);
// x1..y2 normalised
void host_emat_counts(const double* x1, const double* y1, const double* x2, const double* y2, int n, unsigned long long seed,
                      int max_iters, double thr2, int* out_counts, int* out_sol) {
    std::vector<double> ws((size_t)msfm_emat::kWork);
    for (int it = 0; it < max_iters; ++it) {
        const int ns = msfm_emat::hypothesis<1>(x1, y1, x2, y2, n, seed, it, ws.data());
        int best = 0, bs = -1;
        for (int s = 0; s < ns; ++s) {
            int c = 0;
            for (int i = 0; i < n; ++i) c += msfm_emat::sampson(ws.data() + msfm_emat::kWsSol + 9 * s, x1[i], y1[i], x2[i], y2[i]) <= thr2 ? 1 : 0;
            if (bs < 0 || c > best) {
                best = c;
                bs = s;
            }
        }
        out_counts[it] = best;
        out_sol[it] = bs;
    }
}

// EssentialRansacMask on pixel coordinates p1, p2 (n x 2); returns the mask length (0: nothing kept)
int host_essential_ransac(const float* p1, const float* p2, int n, const double* cam, double threshold, double confidence,
                          int max_iters, unsigned long long seed, unsigned char* mask) {
    std::vector<Point2f> a((size_t)n), b((size_t)n);
    for (int i = 0; i < n; ++i) {
        a[(size_t)i] = Point2f{p1[2 * i], p1[2 * i + 1]};
        b[(size_t)i] = Point2f{p2[2 * i], p2[2 * i + 1]};
    }
    const CameraIntrinsics c{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6], cam[7]};
    const std::vector<unsigned char> m = EssentialRansacMask(a, b, c, threshold, confidence, max_iters, seed);
    for (size_t i = 0; i < m.size(); ++i) mask[i] = m[i];
    return (int)m.size();
}

// ---- the pieces of msfm_hmat.h (tests/test_hmat_reference.py compares them with tests/hmat_ref.py) -------------------------
void host_hmat_sample4(unsigned long long seed, int it, int n, int* idx) { msfm_hmat::sample4(seed, it, n, idx); }

// q1, q2: 4 x 2 pixel points; 1 when the sample passes the subset check
int host_hmat_check_subset(const double* q1, const double* q2) {
    double a[4], b[4], c[4], d[4];
    for (int k = 0; k < 4; ++k) {
        a[k] = q1[2 * k];
        b[k] = q1[2 * k + 1];
        c[k] = q2[2 * k];
        d[k] = q2[2 * k + 1];
    }
    return msfm_hmat::check_subset(a, b, c, d) ? 1 : 0;
}

// q1, q2: 4 x 2 pixel points; H: room for 9.  Returns 1 when solved (no subset check here)
int host_hmat_four_point(const double* q1, const double* q2, double* H) {
    double a[4], b[4], c[4], d[4];
    for (int k = 0; k < 4; ++k) {
        a[k] = q1[2 * k];
        b[k] = q1[2 * k + 1];
        c[k] = q2[2 * k];
        d[k] = q2[2 * k + 1];
    }
    return msfm_hmat::four_point(a, b, c, d, H) ? 1 : 0;
}

double host_hmat_error(const double* H, double x, double y, double u, double v) { return msfm_hmat::reproj_error(H, x, y, u, v); }

// replay_adaptive<4> over counts [0, avail); *decided = 0 when it needed more
int host_hmat_replay(const int* counts, int avail, int n, int max_iters, double confidence, int* best_count, int* decided) {
    bool dec = true;
    const int r = msfm_fmat::replay_adaptive<4>(n, max_iters, confidence, [&](int it) { return counts[it]; }, best_count, avail, &dec);
    *decided = dec ? 1 : 0;
    return r;
}

// count of every hypothesis it0 .. it0 + n_its - 1 (0 for a rejected sample) and whether its sample was solved; pixel coordinates
void host_hmat_counts(const float* x1, const float* y1, const float* x2, const float* y2, int n, unsigned long long seed, int it0,
                      int n_its, double thr2, int* out_counts, int* out_solved) {
    for (int k = 0; k < n_its; ++k) {
        double H[9];
        const bool ok = msfm_hmat::hypothesis(x1, y1, x2, y2, n, seed, it0 + k, H);
        int c = 0;
        if (ok)
            for (int i = 0; i < n; ++i) c += msfm_hmat::reproj_error(H, x1[i], y1[i], x2[i], y2[i]) <= thr2 ? 1 : 0;
        out_counts[k] = c;
        out_solved[k] = ok ? 1 : 0;
    }
}

// HomographyRansacMask on pixel coordinates p1, p2 (n x 2); returns the mask length (0: nothing kept)
int host_homography_ransac(const float* p1, const float* p2, int n, double threshold, double confidence, int max_iters,
                           unsigned long long seed, unsigned char* mask) {
    std::vector<Point2f> a((size_t)n), b((size_t)n);
    for (int i = 0; i < n; ++i) {
        a[(size_t)i] = Point2f{p1[2 * i], p1[2 * i + 1]};
        b[(size_t)i] = Point2f{p2[2 * i], p2[2 * i + 1]};
    }
    const std::vector<unsigned char> m = HomographyRansacMask(a, b, threshold, confidence, max_iters, seed);
    for (size_t i = 0; i < m.size(); ++i) mask[i] = m[i];
    return (int)m.size();
}

// TwoViewSelectMask on pixel coordinates p1, p2 (n x 2): model 0 (F) or 1 (E with the camera fx, fy, cx, cy, k1, k2, p1, p2 of `cam`;
// NULL under model 0) against the homography.  out3 = {chosen model, nE, nH}; returns the mask length (0: nothing kept)
int host_two_view_select(const float* p1, const float* p2, int n, int model, const double* cam, double h_ratio, double threshold,
                         double confidence, int max_iters, unsigned long long seed, unsigned char* mask, int* out3) {
    std::vector<Point2f> a((size_t)n), b((size_t)n);
    for (int i = 0; i < n; ++i) {
        a[(size_t)i] = Point2f{p1[2 * i], p1[2 * i + 1]};
        b[(size_t)i] = Point2f{p2[2 * i], p2[2 * i + 1]};
    }
    CameraIntrinsics c = {0, 0, 0, 0, 0, 0, 0, 0};
    if (cam) c = CameraIntrinsics{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6], cam[7]};
    const std::vector<unsigned char> m =
        TwoViewSelectMask(a, b, model, c, h_ratio, threshold, confidence, max_iters, seed, &out3[0], &out3[1], &out3[2]);
    for (size_t i = 0; i < m.size(); ++i) mask[i] = m[i];
    return (int)m.size();
}

// The staging schedule of the device's staged RANSAC (csrc/msfm_verify_staged.hip.h) for one pair of model 1 (E, `cam` as in
// host_essential_ransac) or 2 (H) on pixel coordinates p1, p2 (n x 2): the counts of the twin, computed lazily, replayed with
// avail = min((r + 1) * kRound, max_iters) for r = 0, 1, .. until the replay is decided.  *rounds = r + 1 (the rounds the pair
// runs) and *solved = min(*rounds * kRound, max_iters) (the live lanes of those rounds); 0 and 0 when n < kSample.  Returns 0, or
// -1 for another model.
int host_staged_schedule(int model, const float* p1, const float* p2, int n, const double* cam, double threshold, double confidence,
                         int max_iters, unsigned long long seed, int* rounds, long long* solved) {
    constexpr int kEmatRound = 32;   // kVeRound (csrc/msfm_verify_e.hip.h)
    constexpr int kHmatRound = 64;   // kVhRound (csrc/msfm_verify_h.hip.h)
    *rounds = 0;
    *solved = 0;
    if (model != MSFM_VERIFY_ESSENTIAL && model != MSFM_VERIFY_HOMOGRAPHY) return -1;
    const bool e = model == MSFM_VERIFY_ESSENTIAL;
    const int k_sample = e ? 5 : 4, k_round = e ? kEmatRound : kHmatRound;
    if (n < k_sample) return 0;
    std::vector<double> dx1((size_t)n), dy1((size_t)n), dx2((size_t)n), dy2((size_t)n);
    std::vector<float> fx1((size_t)n), fy1((size_t)n), fx2((size_t)n), fy2((size_t)n);
    double thr2;
    if (e) {
        const msfm_emat::Camera c{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6], cam[7]};
        for (int i = 0; i < n; ++i) {
            msfm_emat::undistort(c, (double)p1[2 * i], (double)p1[2 * i + 1], &dx1[(size_t)i], &dy1[(size_t)i]);
            msfm_emat::undistort(c, (double)p2[2 * i], (double)p2[2 * i + 1], &dx2[(size_t)i], &dy2[(size_t)i]);
        }
        const double t = threshold / ((cam[0] + cam[1]) * 0.5);
        thr2 = t * t;
    } else {
        for (int i = 0; i < n; ++i) {
            fx1[(size_t)i] = p1[2 * i];
            fy1[(size_t)i] = p1[2 * i + 1];
            fx2[(size_t)i] = p2[2 * i];
            fy2[(size_t)i] = p2[2 * i + 1];
        }
        thr2 = threshold * threshold;
    }
    std::vector<double> ws((size_t)msfm_emat::kWork);
    std::vector<int> counts;   // hypotheses 0 .. counts.size() - 1, computed so far
    auto count_at = [&](int it) {
        while ((int)counts.size() <= it) {
            const int h = (int)counts.size();
            int c = 0;
            if (e) {   // the largest count over the hypothesis' solutions (EssentialRansacMask)
                const int ns = msfm_emat::hypothesis<1>(dx1.data(), dy1.data(), dx2.data(), dy2.data(), n, seed, h, ws.data());
                for (int s = 0; s < ns; ++s) {
                    const double* E = ws.data() + msfm_emat::kWsSol + 9 * s;
                    int cs = 0;
                    for (int i = 0; i < n; ++i) cs += msfm_emat::sampson(E, dx1[(size_t)i], dy1[(size_t)i], dx2[(size_t)i], dy2[(size_t)i]) <= thr2 ? 1 : 0;
                    c = std::max(c, cs);
                }
            } else {   // 0 for a rejected sample (HomographyRansacMask)
                double H[9];
                if (msfm_hmat::hypothesis(fx1.data(), fy1.data(), fx2.data(), fy2.data(), n, seed, h, H))
                    for (int i = 0; i < n; ++i) c += msfm_hmat::reproj_error(H, fx1[(size_t)i], fy1[(size_t)i], fx2[(size_t)i], fy2[(size_t)i]) <= thr2 ? 1 : 0;
            }
            counts.push_back(c);
        }
        return counts[(size_t)it];
    };
    for (int r = 0;; ++r) {
        const int avail = std::min((r + 1) * k_round, max_iters);
        int best_count = 0;
        bool decided = false;
        if (e) msfm_fmat::replay_adaptive<5>(n, max_iters, confidence, count_at, &best_count, avail, &decided);
        else msfm_fmat::replay_adaptive<4>(n, max_iters, confidence, count_at, &best_count, avail, &decided);
        if (decided) {
            *rounds = r + 1;
            *solved = std::min((long long)(r + 1) * k_round, (long long)max_iters);
            return 0;
        }
    }
}

// msfm_select_homography (csrc/msfm_hostutil.h), the rule itself
int host_select_homography(int n_epipolar, int n_homography, double h_ratio) { return msfm_select_homography(n_epipolar, n_homography, h_ratio) ? 1 : 0; }

// ---- the pieces of msfm_pose.h (tests/test_pose_reference.py compares them with tests/pose_ref.py) --------------------------
// the four candidates of E, each R[9] | t[3]; returns 1, or 0 when E has no decomposition
int host_pose_decompose(const double* E, double* cand48) { return msfm_pose::decompose<1>(E, cand48) ? 1 : 0; }

// the DLT point of one match under P = R[9] | t[3]; returns 1 when triangulated
int host_pose_triangulate(const double* P, double x1, double y1, double x2, double y2, double* X) {
    return msfm_pose::triangulate(P, x1, y1, x2, y2, X) ? 1 : 0;
}

// one kept match under P: out3 = {positive depth (0 / 1), error in pixels, angle in degrees}
void host_pose_evaluate(const double* P, double f, double x1, double y1, double x2, double y2, double* out3) {
    bool depth;
    msfm_pose::evaluate(P, f, x1, y1, x2, y2, &depth, &out3[1], &out3[2]);
    out3[0] = depth ? 1.0 : 0.0;
}

void host_pose_acos(const double* x, int n, double* out) {
    for (int i = 0; i < n; ++i) out[i] = msfm_pose::acos(x[i]);
}

int host_initial_candidate(int n_triangulated, double median_tri_angle, double mean_tri_angle, double mean_residual, int min_num_inliers,
                           double tri_max_error, double tri_min_angle) {
    return msfm_initial_candidate(n_triangulated, median_tri_angle, mean_tri_angle, mean_residual, min_num_inliers, tri_max_error,
                                  tri_min_angle) ? 1 : 0;
}

// msfm_pose::two_view_record on a given E and kept matches in normalised coordinates (n each); returns the winning candidate or -1
int host_pose_record(const double* E, const double* x1, const double* y1, const double* x2, const double* y2, int n, double f,
                     int min_num_inliers, double tri_max_error, double tri_min_angle, msfm_two_view_record* record) {
    const msfm_two_view_params prm = {min_num_inliers, 0, tri_max_error, tri_min_angle};
    int winner = -1;
    msfm_pose::two_view_record(E, x1, y1, x2, y2, n, f, prm, record, &winner);
    return winner;
}

// TwoViewGeometry on pixel coordinates p1, p2 (n x 2) with the camera fx, fy, cx, cy, k1, k2, p1, p2 of `cam`; returns the mask
// length (0: nothing kept)
int host_two_view_geometry(const float* p1, const float* p2, int n, const double* cam, int min_num_inliers, double tri_max_error,
                           double tri_min_angle, double threshold, double confidence, int max_iters, unsigned long long seed,
                           unsigned char* mask, msfm_two_view_record* record) {
    std::vector<Point2f> a((size_t)n), b((size_t)n);
    for (int i = 0; i < n; ++i) {
        a[(size_t)i] = Point2f{p1[2 * i], p1[2 * i + 1]};
        b[(size_t)i] = Point2f{p2[2 * i], p2[2 * i + 1]};
    }
    const CameraIntrinsics c{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6], cam[7]};
    const msfm_two_view_params prm = {min_num_inliers, 0, tri_max_error, tri_min_angle};
    const std::vector<unsigned char> m = TwoViewGeometry(a, b, c, prm, record, threshold, confidence, max_iters, seed);
    for (size_t i = 0; i < m.size(); ++i) mask[i] = m[i];
    return (int)m.size();
}

// RefineTwoView on the kept matches in normalised coordinates (n each, list order) under the focal length f: *record is read and
// rewritten iff the refined record stands, *refinement is always filled
void host_refine_two_view(const double* x1, const double* y1, const double* x2, const double* y2, int n, double f, int min_num_inliers,
                          double tri_max_error, double tri_min_angle, int max_iters, int min_matches, double step_tol,
                          msfm_two_view_record* record, msfm_two_view_refinement* refinement) {
    const CameraIntrinsics c{f, f, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const msfm_two_view_params prm = {min_num_inliers, 0, tri_max_error, tri_min_angle};
    const msfm_two_view_refine_params rp = {max_iters, min_matches, step_tol};
    RefineTwoView(x1, y1, x2, y2, n, c, prm, rp, record, refinement);
}

// the pieces of csrc/msfm_pose_refine.h at the pose (R, t): the residuals r[n], with J != NULL the Jacobian J[n x 5] too
void host_tvr_residuals(const double* R, const double* t, double f, const double* x1, const double* y1, const double* x2, const double* y2,
                        int n, double* r, double* J) {
    msfm_tvr::State s;
    for (int k = 0; k < 9; ++k) s.R[k] = R[k];
    for (int k = 0; k < 3; ++k) s.t[k] = t[k];
    double E[9], D[5][9];
    msfm_tvr::linear_model(s, E, D);
    for (int i = 0; i < n; ++i) {
        if (J) r[i] = msfm_tvr::jacobian(E, D, f, x1[i], y1[i], x2[i], y2[i], J + 5 * i);
        else r[i] = msfm_tvr::residual(E, f, x1[i], y1[i], x2[i], y2[i]);
    }
}

// (R, t) moved by delta = (a, b): msfm_tvr::apply_step; returns 0 when the new pose is not finite
int host_tvr_update(const double* R, const double* t, const double* delta, double* Rn, double* tn) {
    msfm_tvr::State s, sn;
    for (int k = 0; k < 9; ++k) s.R[k] = R[k];
    for (int k = 0; k < 3; ++k) s.t[k] = t[k];
    const bool ok = msfm_tvr::apply_step(s, delta, &sn);
    for (int k = 0; k < 9; ++k) Rn[k] = sn.R[k];
    for (int k = 0; k < 3; ++k) tn[k] = sn.t[k];
    return ok ? 1 : 0;
}

// msfm_pair_scratch_bytes with its two defaulted arguments spelled out
long long host_pair_scratch_bytes_refine(int n1, int n2, int n1pad, int n2pad, int blocks128, int blocks512, int route, int two_view,
                                         int two_view_refine) {
    return msfm_pair_scratch_bytes(n1, n2, n1pad, n2pad, blocks128, blocks512, route, two_view != 0, two_view_refine != 0);
}

// ---- feature tracks: the host twin of the device session (csrc/msfm_tracks.h) ------------------------------------------------------
// One session in one call: begin over (ids, rows), the CSR lists, optional forests to import (n_forests x nodes), finish under the
// filter.  counts: the 12 integer fields of msfm_track_stats in order.  Returns 0, 1 + the numbering error, 10 for a forest entry out of
// range, 11 when the result does not fit the caller's capacities (counts are valid then).
int host_tracks_build(const int* ids, const int* rows, int n, int min_pair_matches, const int* pairs, int n_pairs, const long long* offsets,
                      const int* qt, const int* forests, int n_forests, int min_length, int max_length, int keep_inconsistent,
                      long long* counts, long long* out_offsets, int* out_image_ids, int* out_point_idx, unsigned char* out_consistent,
                      int* out_track_of, int* out_forest, long long cap_tracks, long long cap_observations) {
    MsfmTrackNodes nd;
    const int e = msfm_track_number_nodes(ids, rows, n, MSFM_MAX_IMAGES, &nd);
    if (e != MSFM_TRACK_NODES_OK) return 1 + e;
    MsfmTrackTwin tw;
    tw.begin(nd, min_pair_matches);
    std::vector<int64_t> offs((size_t)n_pairs + 1, 0);
    for (int p = 0; p <= n_pairs && offsets; ++p) offs[(size_t)p] = offsets[p];
    tw.add(pairs, n_pairs, offs.data(), qt);
    for (int k = 0; k < n_forests; ++k)
        if (!tw.import_forest(forests + (size_t)k * (size_t)nd.nodes())) return 10;
    MsfmTrackFilter f;
    f.min_length = min_length;
    f.max_length = max_length;
    f.keep_inconsistent = keep_inconsistent;
    const MsfmTrackResult r = tw.finish(f);
    const long long c[12] = {r.counts.nodes, r.counts.edges, r.counts.pairs, r.counts.pairs_skipped, r.counts.pairs_below_min,
                             r.counts.matches_ignored, r.counts.tracks_total, r.counts.tracks_inconsistent,
                             r.counts.tracks_over_max_length, r.counts.tracks_kept, r.counts.observations_kept, r.counts.longest_track};
    for (int k = 0; k < 12; ++k) counts[k] = c[k];
    if (out_forest) tw.export_forest(out_forest);
    if (r.counts.tracks_kept > cap_tracks || r.counts.observations_kept > cap_observations) return 11;
    std::copy(r.offsets.begin(), r.offsets.end(), out_offsets);
    std::copy(r.image_ids.begin(), r.image_ids.end(), out_image_ids);
    std::copy(r.point_idx.begin(), r.point_idx.end(), out_point_idx);
    std::copy(r.consistent.begin(), r.consistent.end(), out_consistent);
    std::copy(r.track_of.begin(), r.track_of.end(), out_track_of);
    return 0;
}

// ---- track triangulation: the host twin of the device kernels (csrc/msfm_triangulate.h, TriangulateTracks) ---------------------------
// Every twin of the reconstruction stage (twin_triangulate_tracks .. twin_map_visibility) takes one host_map (HostTwinMap.h): the
// track result, the declared images with their keypoints, the pose list, the camera, the triangulation's thresholds, the slice and the
// state.  Each twin's comment names the fields it reads and the ones it rewrites; its own parameters and outputs follow the block.
// All of them return 0; 1: a pose's image is not declared or given twice; 2: an image id outside [0, MSFM_MAX_IMAGES); 3 and 4 as each
// twin says.  The host_* exports of the same names, with the block's fields spelt out as raw arguments, stand behind
// twin_map_visibility and the two twins of the map alignment (which have no host_* form).
// What every twin makes of the block first: the rank of each declared image, the prepared pose of each rank (invalid where the list
// has none), the rank of each entry of the pose list, and the camera.
struct TwinScene {
    std::vector<int> rank_of;
    std::vector<msfm_tri::Pose> table;
    std::vector<int> list_rank;
    msfm_emat::Camera cam;
    // the rank of a declared id, -1 for any other
    int rank(int id) const { return (id >= 0 && id < MSFM_MAX_IMAGES) ? rank_of[(size_t)id] : -1; }
};
// Returns 0, or the twins' codes 2 and 1.
static int twin_scene(const host_map& m, TwinScene* s) {
    s->rank_of.assign((size_t)MSFM_MAX_IMAGES, -1);
    for (int k = 0; k < m.n_images; ++k) {
        if (m.ids[k] < 0 || m.ids[k] >= MSFM_MAX_IMAGES) return 2;
        s->rank_of[(size_t)m.ids[k]] = k;   // (any one-to-one numbering serves the twin: the device's ranks never reach the output)
    }
    s->table.resize((size_t)std::max(m.n_images, 1));
    s->list_rank.assign((size_t)std::max(m.n_poses, 1), 0);
    std::vector<char> given((size_t)std::max(m.n_images, 1), 0);
    const msfm_pose_rt none = {};
    for (auto& p : s->table) msfm_tri::prepare_pose(none, &p);
    for (int k = 0; k < m.n_poses; ++k) {
        const int r = s->rank(m.pose_ids[k]);
        if (r < 0 || given[(size_t)r]) return 1;
        given[(size_t)r] = 1;
        s->list_rank[(size_t)k] = r;
        msfm_tri::prepare_pose(m.poses[k], &s->table[(size_t)r]);
    }
    s->cam = msfm_emat::Camera{m.cam[0], m.cam[1], m.cam[2], m.cam[3], m.cam[4], m.cam[5], m.cam[6], m.cam[7]};
    return 0;
}
// A list of ids as one byte per rank; false (the twins' code 4) for an id that is not declared, is given twice or, with `posed`, has
// no valid pose in the scene's table.
static bool twin_rank_bytes(const TwinScene& s, const int* ids, int n, bool posed, std::vector<uint8_t>* bytes) {
    bytes->assign(s.table.size(), 0);
    for (int k = 0; k < n; ++k) {
        const int r = s.rank(ids[k]);
        if (r < 0 || (*bytes)[(size_t)r] || (posed && !s.table[(size_t)r].valid)) return false;
        (*bytes)[(size_t)r] = 1;
    }
    return true;
}

// Reads the tracks with `consistent`, the images, the pose list, cam, the three thresholds and the slice; WRITES points and residuals
// of the slice's tracks (mask and have_mask are not used).
int twin_triangulate_tracks(const host_map* m) {
    TwinScene sc;
    if (const int rc = twin_scene(*m, &sc)) return rc;
    const msfm_tri::Params prm = {m->max_error, m->min_angle, m->min_views, 0};
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are int64");
    static_assert(sizeof(msfm_tri::RobustTrace) == 12 * sizeof(int), "the trace is twelve int32");
    msfm_tri::TriangulateTracks(m->offsets, m->image_ids, m->point_idx, m->consistent, m->first, m->count, sc.rank_of.data(), m->kxy,
                                sc.table.data(), sc.cam, prm, m->points, m->residuals);
    return 0;
}

// The robust twin (TriangulateTracksRobust): as twin_triangulate_tracks, with max_hypotheses, and it WRITES mask as well, the inlier
// byte per observation.  counts4 (may be NULL): retried, rescued, observations_rejected, hypotheses of the tracks computed by this call
// are ADDED to it.  out_trace (may be NULL) receives msfm_tri::RobustTrace (12 int32) per computed track at the track's own position:
// the route it took.  3: max_hypotheses outside 1 .. 1024.
int twin_triangulate_tracks_robust(const host_map* m, int max_hypotheses, long long* counts4, int* out_trace) {
    TwinScene sc;
    if (const int e = twin_scene(*m, &sc)) return e;
    if (max_hypotheses < 1 || max_hypotheses > 1024) return 3;
    const msfm_tri::RobustParams prm = {m->max_error, m->min_angle, m->min_views, max_hypotheses};
    msfm_tri::RobustCounts rc = {0, 0, 0, 0};
    msfm_tri::TriangulateTracksRobust(m->offsets, m->image_ids, m->point_idx, m->consistent, m->first, m->count, sc.rank_of.data(), m->kxy,
                                      sc.table.data(), sc.cam, prm, m->points, m->residuals, m->mask, &rc,
                                      reinterpret_cast<msfm_tri::RobustTrace*>(out_trace));
    if (counts4) {
        counts4[0] += rc.retried;
        counts4[1] += rc.rescued;
        counts4[2] += rc.observations_rejected;
        counts4[3] += rc.hypotheses;
    }
    return 0;
}
void host_tri_sample2(long long track, int h, int m, int* idx2) { msfm_tri::sample2(msfm_tri::tri_seed(track), h, m, idx2); }

// ---- point refinement: the host twin of the device kernels (csrc/msfm_refine.h, RefinePoints) ---------------------------------------
// Reads the tracks (not `consistent`), the images, the pose list, cam, max_error and min_angle (the verdict's: the thresholds the
// triangulation ran with), the slice and mask (may be NULL: the points are the plain call's); points and residuals of the slice's
// tracks are read and REWRITTEN in place.  counts5 (may be NULL): eligible, refined, gained_error_ok, rejected_by_verdict, iterations
// of those tracks are ADDED to it; costs2 (may be NULL): their cost_before and cost_after, summed in track order, are ADDED to it.
// out_trace (may be NULL) receives msfm_ref::Trace (40 bytes) per computed track at the track's own position.  3: max_iters outside
// 0 .. 100 or a bad step_tol.
int twin_refine_points(const host_map* m, double step_tol, int max_iters, long long* counts5, double* costs2, void* out_trace) {
    static_assert(sizeof(msfm_ref::Trace) == 40 && sizeof(msfm_ref::Obs) == 24, "the trace is six int32 and two doubles");
    TwinScene sc;
    if (const int e = twin_scene(*m, &sc)) return e;
    if (max_iters < 0 || max_iters > 100 || !(step_tol >= 0.0) || !msfm_pose::finite(step_tol)) return 3;
    msfm_ref::Counts rc = {0, 0, 0, 0, 0, 0.0, 0.0};
    msfm_ref::RefinePoints(m->offsets, m->image_ids, m->point_idx, m->first, m->count, sc.rank_of.data(), m->kxy, sc.table.data(), m->mask,
                           sc.cam, msfm_ref::Verdict{m->max_error, m->min_angle}, msfm_ref::Params{step_tol, max_iters, 0}, m->points,
                           m->residuals, &rc, static_cast<msfm_ref::Trace*>(out_trace));
    if (counts5) {
        counts5[0] += rc.eligible;
        counts5[1] += rc.refined;
        counts5[2] += rc.gained_error_ok;
        counts5[3] += rc.rejected_by_verdict;
        counts5[4] += rc.iterations;
    }
    if (costs2) {
        costs2[0] += rc.cost_before;
        costs2[1] += rc.cost_after;
    }
    return 0;
}

// ---- pose refinement: the host twin of the device kernels (csrc/msfm_refine_poses.h, RefinePoses) -------------------------------------
// Reads the tracks (not `consistent`; all n_tracks of them, not the slice: an image's fitting set runs through every track), the
// images, cam, max_error and min_angle (the verdict's) and mask (may be NULL); min_observations and the ids to hold fixed are its own.
// The entries of `poses` are read AND REWRITTEN: where a refined pose stands its R and t replace the entry.  points and residuals are
// read and REWRITTEN by the re-verdict.  out_records: one msfm_pose_refinement per entry of the pose list.  counts9 (may be NULL):
// images, eligible, refined, rejected_by_inliers, iterations, observations, points_reposed, points_lost, points_gained are ADDED to it;
// costs2 (may be NULL): cost_before and cost_after, summed in list order, are ADDED to it.  out_trace (may be NULL) receives
// msfm_ref::Trace (40 bytes) per entry of the pose list.  3: a bad parameter; 4: a fixed id that is not declared or given twice.
int twin_refine_poses(host_map* m, double step_tol, int max_iters, int min_observations, const int* fixed_ids, int n_fixed,
                      msfm_pose_refinement* out_records, long long* counts9, double* costs2, void* out_trace) {
    static_assert(sizeof(msfm_ref::Trace) == 40 && sizeof(msfm_pose_refinement) == 48, "the trace is six int32 and two doubles");
    TwinScene sc;
    if (const int e = twin_scene(*m, &sc)) return e;
    if (max_iters < 0 || max_iters > 100 || !(step_tol >= 0.0) || !msfm_pose::finite(step_tol) || min_observations < 3 || n_fixed < 0) return 3;
    std::vector<uint8_t> fixed, changed(sc.table.size(), 0);
    if (!twin_rank_bytes(sc, fixed_ids, n_fixed, false, &fixed)) return 4;
    msfm_rp::Counts rc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0};
    msfm_rp::RefinePoses(m->offsets, m->image_ids, m->point_idx, m->n_tracks, sc.rank_of.data(), m->kxy, sc.table.data(), m->n_images, m->mask,
                         sc.cam, msfm_ref::Verdict{m->max_error, m->min_angle}, msfm_rp::Params{step_tol, max_iters, min_observations},
                         sc.list_rank.data(), m->pose_ids, m->n_poses, fixed.data(), m->points, m->residuals, out_records, changed.data(), &rc,
                         static_cast<msfm_ref::Trace*>(out_trace));
    for (int k = 0; k < m->n_poses; ++k) {
        const size_t r = (size_t)sc.list_rank[(size_t)k];
        if (!changed[r]) continue;
        for (int q = 0; q < 9; ++q) m->poses[k].R[q] = sc.table[r].R[q];
        for (int q = 0; q < 3; ++q) m->poses[k].t[q] = sc.table[r].t[q];
    }
    if (counts9) {
        const long long v[9] = {rc.images, rc.eligible, rc.refined, rc.rejected_by_inliers, rc.iterations, rc.observations, rc.points_reposed,
                                rc.points_lost, rc.points_gained};
        for (int k = 0; k < 9; ++k) counts9[k] += v[k];
    }
    if (costs2) {
        costs2[0] += rc.cost_before;
        costs2[1] += rc.cost_after;
    }
    return 0;
}

// ---- camera refinement: the host twin of the device kernels (csrc/msfm_refine_camera.h, RefineCamera) ----------------------------------
// Reads the tracks (not `consistent`; all n_tracks of them, not the slice), the images, the pose list, max_error and min_angle (the
// verdict's) and mask (may be NULL); mask_bits (MSFM_CAM_*) and min_observations are its own.  The block's `cam` is read AND
// REWRITTEN: the refined camera where it stands.  points and residuals are read and REWRITTEN by the re-verdict.  counts12 (may be
// NULL) RECEIVES observations, behind, iterations, accepted_steps, stop, refined, rejected_by_inliers, inliers_before, inliers_after,
// points_recalibrated, points_lost, points_gained; costs2 (may be NULL) cost_before and cost_after.  out_trace (may be NULL) receives one
// msfm_ref::Trace (40 bytes).  3: a bad parameter.
int twin_refine_camera(host_map* m, double step_tol, int mask_bits, int max_iters, int min_observations, long long* counts12, double* costs2,
                       void* out_trace) {
    static_assert(sizeof(msfm_rc::Slot) == 40 && sizeof(msfm_camera_refine_params) == 24 && sizeof(msfm_camera_refine_stats) == 248, "sizes");
    TwinScene sc;
    if (const int e = twin_scene(*m, &sc)) return e;
    if (!msfm_rc::mask_ok(mask_bits) || max_iters < 0 || max_iters > 100 || !(step_tol >= 0.0) || !msfm_pose::finite(step_tol) ||
        min_observations < 6)
        return 3;
    msfm_rc::Counts rc = {};
    msfm_rc::RefineCamera(m->offsets, m->image_ids, m->point_idx, m->n_tracks, sc.rank_of.data(), m->kxy, sc.table.data(), m->mask, &sc.cam,
                          msfm_ref::Verdict{m->max_error, m->min_angle}, msfm_rc::Params{step_tol, mask_bits, max_iters, min_observations, 0},
                          m->points, m->residuals, &rc, static_cast<msfm_ref::Trace*>(out_trace));
    const double c8[8] = {sc.cam.fx, sc.cam.fy, sc.cam.cx, sc.cam.cy, sc.cam.k1, sc.cam.k2, sc.cam.p1, sc.cam.p2};
    for (int k = 0; k < 8; ++k) m->cam[k] = c8[k];
    if (counts12) {
        const long long v[12] = {rc.observations, rc.behind, rc.iterations, rc.accepted_steps, rc.stop, rc.refined, rc.rejected_by_inliers,
                                 rc.inliers_before, rc.inliers_after, rc.points_recalibrated, rc.points_lost, rc.points_gained};
        for (int k = 0; k < 12; ++k) counts12[k] = v[k];
    }
    if (costs2) {
        costs2[0] = rc.cost_before;
        costs2[1] = rc.cost_after;
    }
    return 0;
}
// the 256-element tree and the two levels of the camera refinement's summation over n doubles (tests)
double host_rc_reduce(const double* v, long long n) {
    double out[1];
    msfm_rc::reduce_slots<1>(n, [&](long long s, double* o) { o[0] = v[s]; }, out);
    return out[0];
}

// ---- map extension: the host twin of the device kernels (csrc/msfm_extend.h, ExtendPoints) --------------------------------------------
// Reads the tracks with `consistent`, the images, cam, the triangulation's three thresholds and the slice.  The block's pose list is
// the ENLARGED one (the session's list with the new images appended or replaced in place, as msfm_extend_points leaves it); new_ids,
// its own: the images that gained their valid pose in this call (each must be in the enlarged list with a valid pose); max_hypotheses
// 0 = plain route for created tracks.  points, residuals and mask of the slice's tracks are read and REWRITTEN in place; have_mask 0:
// the points are the plain call's and the bytes of the computed tracks are created first.  counts7 (may be NULL): tracks_touched,
// continued, observations_added, observations_rejected, created_attempted, created, retried of those tracks are ADDED to it.
// out_trace (may be NULL) receives msfm_ext::Trace (four int32) per computed track at the track's own position.  3: max_hypotheses
// outside 0 .. 1024; 4: a new id that is not in the enlarged list with a valid pose, or given twice.
int twin_extend_points(const host_map* m, const int* new_ids, int n_new, int max_hypotheses, long long* counts7, int* out_trace) {
    static_assert(sizeof(msfm_ext::Trace) == 4 * sizeof(int), "the trace is four int32");
    TwinScene sc;
    if (const int e = twin_scene(*m, &sc)) return e;
    if (max_hypotheses < 0 || max_hypotheses > 1024) return 3;
    std::vector<uint8_t> gained;
    if (!twin_rank_bytes(sc, new_ids, n_new, true, &gained)) return 4;
    msfm_ext::Counts ec = {0, 0, 0, 0, 0, 0, 0};
    msfm_ext::ExtendPoints(m->offsets, m->image_ids, m->point_idx, m->consistent, m->first, m->count, sc.rank_of.data(), m->kxy,
                           sc.table.data(), gained.data(), sc.cam, msfm_tri::Params{m->max_error, m->min_angle, m->min_views, 0},
                           max_hypotheses, m->have_mask != 0, m->points, m->residuals, m->mask, &ec,
                           reinterpret_cast<msfm_ext::Trace*>(out_trace));
    if (counts7) {
        const long long v[7] = {ec.tracks_touched, ec.continued, ec.observations_added, ec.observations_rejected, ec.created_attempted,
                                ec.created, ec.retried};
        for (int k = 0; k < 7; ++k) counts7[k] += v[k];
    }
    return 0;
}

// ---- map filtering: the host twin of the device kernel (csrc/msfm_filter.h, FilterPoints) ----------------------------------------------
// Reads the tracks with `consistent`, the images, the pose list (the session's CURRENT one), cam, max_error and min_angle (of the
// triangulation that made the points; min_views is not used) and the slice.  Its own: the call's thresholds (flt_max_error,
// flt_min_angle) and scope_ids, the images the call is limited to (n_scope == 0: every track).  points, residuals and mask of the
// slice's tracks are read and REWRITTEN in place; have_mask 0: the bytes of the computed tracks are created first.  counts7 (may be
// NULL): eligible, dropped_by_depth, dropped_by_error, trimmed, regained, removed_by_views, removed_by_angle of those tracks are ADDED
// to it.  out_trace (may be NULL) receives msfm_flt::Trace (four int32) per computed track at the track's own position.  3: a
// non-finite or negative threshold or n_scope < 0; 4: a scope id that is not declared or given twice.
int twin_filter_points(const host_map* m, const int* scope_ids, int n_scope, double flt_max_error, double flt_min_angle, long long* counts7,
                       int* out_trace) {
    static_assert(sizeof(msfm_flt::Trace) == 4 * sizeof(int), "the trace is four int32");
    TwinScene sc;
    if (const int e = twin_scene(*m, &sc)) return e;
    if (!msfm_pose::finite(flt_max_error) || !msfm_pose::finite(flt_min_angle) || !(flt_max_error >= 0.0) || !(flt_min_angle >= 0.0) ||
        n_scope < 0)
        return 3;
    std::vector<uint8_t> scope;
    if (!twin_rank_bytes(sc, scope_ids, n_scope, false, &scope)) return 4;
    msfm_flt::Counts fc = {0, 0, 0, 0, 0, 0, 0};
    msfm_flt::FilterPoints(m->offsets, m->image_ids, m->point_idx, m->consistent, m->first, m->count, sc.rank_of.data(), m->kxy,
                           sc.table.data(), m->n_images, n_scope > 0 ? scope.data() : nullptr, sc.cam,
                           msfm_tri::Params{m->max_error, m->min_angle, 2, 0}, msfm_ref::Verdict{flt_max_error, flt_min_angle},
                           m->have_mask != 0, m->points, m->residuals, m->mask, &fc, reinterpret_cast<msfm_flt::Trace*>(out_trace));
    if (counts7) {
        const long long v[7] = {fc.eligible, fc.dropped_by_depth, fc.dropped_by_error, fc.trimmed, fc.regained, fc.removed_by_views,
                                fc.removed_by_angle};
        for (int k = 0; k < 7; ++k) counts7[k] += v[k];
    }
    return 0;
}

// ---- map completion: the host twin of the device kernel (csrc/msfm_complete.h, CompletePoints) ----------------------------------------
// Reads the tracks with `consistent`, the images, the pose list (the session's CURRENT one), cam, max_error and min_angle (of the
// triangulation that made the points; min_views is not used) and the slice.  Its own: the call's one threshold (cmp_max_error) and
// scope_ids, the images whose candidates the call is limited to (n_scope == 0: every image).  points, residuals and mask of the
// slice's tracks are read and REWRITTEN in place; have_mask 0: the bytes of the computed tracks are created first.  counts6 (may be
// NULL): eligible, candidates, admitted, rejected_by_depth, rejected_by_error, completed of those tracks are ADDED to it.  out_trace
// (may be NULL) receives msfm_cmp::Trace (four int32) per computed track at the track's own position.  3: a non-finite or negative
// threshold, one above max_error, or n_scope < 0; 4: a scope id that is not declared or given twice.
int twin_complete_points(const host_map* m, const int* scope_ids, int n_scope, double cmp_max_error, long long* counts6, int* out_trace) {
    static_assert(sizeof(msfm_cmp::Trace) == 4 * sizeof(int), "the trace is four int32");
    TwinScene sc;
    if (const int e = twin_scene(*m, &sc)) return e;
    if (!msfm_pose::finite(cmp_max_error) || !(cmp_max_error >= 0.0) || cmp_max_error > m->max_error || n_scope < 0) return 3;
    std::vector<uint8_t> scope;
    if (!twin_rank_bytes(sc, scope_ids, n_scope, false, &scope)) return 4;
    msfm_cmp::Counts cc = {0, 0, 0, 0, 0, 0};
    msfm_cmp::CompletePoints(m->offsets, m->image_ids, m->point_idx, m->consistent, m->first, m->count, sc.rank_of.data(), m->kxy,
                             sc.table.data(), m->n_images, n_scope > 0 ? scope.data() : nullptr, sc.cam,
                             msfm_tri::Params{m->max_error, m->min_angle, 2, 0}, cmp_max_error, m->have_mask != 0, m->points, m->residuals,
                             m->mask, &cc, reinterpret_cast<msfm_cmp::Trace*>(out_trace));
    if (counts6) {
        const long long v[6] = {cc.eligible, cc.candidates, cc.admitted, cc.rejected_by_depth, cc.rejected_by_error, cc.completed};
        for (int k = 0; k < 6; ++k) counts6[k] += v[k];
    }
    return 0;
}

// ---- map visibility: the host twin of the device kernels (csrc/msfm_visibility.h, MapVisibility) -----------------------------------------
// Reads the tracks' offsets, image_ids and `consistent` (all n_tracks of them, not the slice), the declared images `ids` IN RANK ORDER
// (the records and the matrix columns follow it; no pixel is read: kxy, cam and the thresholds are not used) and, under basis 1 only,
// the pose list (the session's current one), points (the records) and mask (the session's inlier bytes or NULL).  Its own: the query
// list and the basis (0 tracks, 1 map).  out_records: n_images msfm_image_visibility; out_matrix: n_query x n_images uint32 (may be
// NULL without a query); counts3 (may be NULL) RECEIVES tracks_counted, elements_counted, pair_increments.  Nothing in the block is
// rewritten: the call counts.  3: an unknown basis or n_query < 0; 4: a query id that is not declared or given twice.
int twin_map_visibility(const host_map* m, const int* query_ids, int n_query, int basis, msfm_image_visibility* out_records,
                        unsigned* out_matrix, long long* counts3) {
    static_assert(sizeof(msfm_image_visibility) == 24 && sizeof(msfm_visibility_params) == 8 && sizeof(msfm_visibility_stats) == 56,
                  "the visibility structs of include/msfm_match.h");
    host_map seen = *m;   // (only the poses' validity counts, and only on the map)
    if (basis != msfm_vis::BASIS_MAP) seen.n_poses = 0;
    const int n_images = m->n_images;
    TwinScene sc;
    if (const int e = twin_scene(seen, &sc)) return e;
    if ((basis != msfm_vis::BASIS_TRACKS && basis != msfm_vis::BASIS_MAP) || n_query < 0) return 3;
    std::vector<uint8_t> queried;
    if (!twin_rank_bytes(sc, query_ids, n_query, false, &queried)) return 4;
    const size_t n = (size_t)std::max(n_images, 1);
    std::vector<uint8_t> posed(n, 0);
    std::vector<int> row_of(n, -1);
    for (size_t r = 0; r < n; ++r) posed[r] = sc.table[r].valid ? 1 : 0;
    for (int k = 0; k < n_query; ++k) row_of[(size_t)sc.rank(query_ids[k])] = k;
    std::vector<uint32_t> image_counters((size_t)msfm_vis::kImageCounters * n, 0);
    msfm_vis::Tally tl = {0, 0, 0};
    msfm_vis::MapVisibility(m->offsets, m->image_ids, m->consistent, m->n_tracks, sc.rank_of.data(), (int)n, posed.data(), row_of.data(),
                            n_query, basis, basis == msfm_vis::BASIS_MAP ? m->points : nullptr,
                            basis == msfm_vis::BASIS_MAP ? m->mask : nullptr, image_counters.data(), out_matrix, &tl);
    for (int r = 0; r < n_images; ++r) {
        msfm_image_visibility v = {};
        v.image_id = m->ids[r];
        v.flags = (posed[(size_t)r] ? MSFM_VIS_POSED : 0) | (queried[(size_t)r] ? MSFM_VIS_QUERIED : 0);
        v.n_elements = (int32_t)image_counters[(size_t)msfm_vis::IMG_ELEMENTS * n + (size_t)r];
        v.n_visible = (int32_t)image_counters[(size_t)msfm_vis::IMG_VISIBLE * n + (size_t)r];
        v.n_points = (int32_t)image_counters[(size_t)msfm_vis::IMG_POINTS * n + (size_t)r];
        out_records[r] = v;
    }
    if (counts3) {
        counts3[0] = tl.tracks;
        counts3[1] = tl.elements;
        counts3[2] = tl.increments;
    }
    return 0;
}
// ---- map alignment: the host twins of the device kernels (csrc/msfm_align.h, EstimateAlignment / TransformMap) ----------------------------
// twin_estimate_alignment reads the images and the pose list (the session's current one) and nothing else of the block, and rewrites
// nothing.  Its own: the n priors (prior_ids, positions: 3 doubles per id), max_error, confidence, max_hypotheses (0: least squares),
// min_inliers.  out: one msfm_alignment (estimate_ms 0); out_per_prior (may be NULL): n msfm_alignment_residual.  3: a bad parameter;
// 4: a prior's id that is not declared or given twice; 5: a non-finite position.
int twin_estimate_alignment(const host_map* m, const int* prior_ids, const double* positions, int n, double max_error, double confidence,
                            int max_hypotheses, int min_inliers, msfm_alignment* out, msfm_alignment_residual* out_per_prior) {
    static_assert(sizeof(msfm_similarity) == 104 && sizeof(msfm_alignment_params) == 24 && sizeof(msfm_alignment) == 144 &&
                      sizeof(msfm_alignment_residual) == 16 && sizeof(msfm_transform_stats) == 48 && sizeof(msfm_aln::Prior) == 48,
                  "the alignment structs of include/msfm_match.h");
    TwinScene sc;
    if (const int e = twin_scene(*m, &sc)) return e;
    if (n < 0 || max_hypotheses < 0 || max_hypotheses > msfm_aln::kMaxHypotheses || !(confidence > 0.0 && confidence < 1.0) ||
        (max_hypotheses > 0 && !(msfm_pose::finite(max_error) && max_error > 0.0)))
        return 3;
    std::vector<uint8_t> listed;
    if (!twin_rank_bytes(sc, prior_ids, n, false, &listed)) return 4;
    for (long long k = 0; k < 3LL * n; ++k)
        if (!msfm_pose::finite(positions[k])) return 5;
    std::vector<msfm_aln::Prior> priors;
    std::vector<int> at;
    for (int k = 0; k < n; ++k) {
        const msfm_tri::Pose& p = sc.table[(size_t)sc.rank(prior_ids[k])];
        if (!p.valid) continue;
        priors.push_back(msfm_aln::Prior{{p.O[0], p.O[1], p.O[2]}, {positions[3 * k], positions[3 * k + 1], positions[3 * k + 2]}});
        at.push_back(k);
    }
    const int used = (int)priors.size();
    std::vector<msfm_alignment_residual> rec((size_t)std::max(used, 1));
    msfm_aln::EstimateAlignment(priors.data(), used, msfm_aln::Params{max_error, confidence, max_hypotheses, min_inliers}, out, rec.data());
    out->n_listed = n;
    if (out_per_prior) {
        for (int k = 0; k < n; ++k) out_per_prior[k] = msfm_alignment_residual{0, 0, -1.0};
        for (int j = 0; j < used; ++j) out_per_prior[at[(size_t)j]] = rec[(size_t)j];
    }
    return 0;
}

// twin_transform_map reads the tracks (not `consistent`; all n_tracks of them, not the slice), the images, cam, max_error and min_angle
// (the verdict's) and mask (may be NULL).  The entries of `poses` are read AND REWRITTEN, as are points and residuals.  counts5 (may be
// NULL) RECEIVES poses_transformed, points_transformed, points_lost, points_gained, succeeded.  3: a similarity msfm_transform_map does
// not take, or a new pose that would not be finite -- nothing is written then.
int twin_transform_map(host_map* m, const msfm_similarity* g, long long* counts5) {
    TwinScene sc;
    if (const int e = twin_scene(*m, &sc)) return e;
    if (!g || !msfm_aln::similarity_ok(*g)) return 3;
    long long moved = 0;
    if (!msfm_aln::TransformPoses(*g, m->poses, m->n_poses, m->poses, &moved)) return 3;
    if (const int e = twin_scene(*m, &sc)) return e;   // the table of the new poses
    msfm_aln::TransformCounts tc = {};
    msfm_aln::TransformMap(m->offsets, m->image_ids, m->point_idx, m->n_tracks, sc.rank_of.data(), m->kxy, sc.table.data(), m->mask, sc.cam,
                           msfm_ref::Verdict{m->max_error, m->min_angle}, *g, m->points, m->residuals, &tc);
    if (counts5) {
        const long long v[5] = {moved, tc.points_transformed, tc.points_lost, tc.points_gained, tc.succeeded};
        for (int k = 0; k < 5; ++k) counts5[k] = v[k];
    }
    return 0;
}
// the fit of n priors (6 doubles each: centre, position) in the header's summation order, no sampling: 1 valid, 0 not (tests)
int host_aln_fit(const double* priors6, int n, msfm_similarity* out) {
    std::vector<int> counts(1);
    const msfm_aln::HostPriors pv{reinterpret_cast<const msfm_aln::Prior*>(priors6), n, counts.data(), nullptr};
    msfm_aln::clear_similarity(out);
    msfm_similarity g;
    if (!msfm_aln::fit_set(pv, [](const msfm_aln::Prior&) { return true; }, &g)) return 0;
    *out = g;
    return 1;
}

// ---- the nine twins under their host_* names, the block's fields as raw arguments -----------------------------------------------------
// The exports as they were before host_map, for callers built against those lists.  Each fills a block from its arguments and calls
// the twin above; a field that twin does not read stays 0 or NULL, and nothing is computed here.  tests/*_twin.py call the twins;
// tests/test_twin_host_abi.py holds each of these against its twin.
static host_map raw_map(const long long* offsets, const int* image_ids, const int* point_idx, const unsigned char* consistent, long long n_tracks,
                        const int* ids, int n_images, const float* const* kxy, const int* pose_ids, const msfm_pose_rt* poses, int n_poses,
                        const double* cam, double max_error, double min_angle, int min_views, long long first, long long count,
                        const msfm_point3d* points, double* residuals, const unsigned char* mask, int have_mask) {
    host_map m = {};
    m.offsets = reinterpret_cast<const int64_t*>(offsets);
    m.image_ids = image_ids;
    m.point_idx = point_idx;
    m.consistent = consistent;
    m.n_tracks = n_tracks;
    m.ids = ids;
    m.kxy = kxy;
    m.pose_ids = pose_ids;
    m.poses = const_cast<msfm_pose_rt*>(poses);
    m.n_images = n_images;
    m.n_poses = n_poses;
    for (int k = 0; k < 8; ++k) m.cam[k] = cam[k];
    m.max_error = max_error;
    m.min_angle = min_angle;
    m.min_views = min_views;
    m.have_mask = have_mask;
    m.first = first;
    m.count = count;
    m.points = const_cast<msfm_point3d*>(points);
    m.residuals = residuals;
    m.mask = const_cast<unsigned char*>(mask);
    return m;
}
int host_triangulate_tracks(const long long* offsets, const int* image_ids, const int* point_idx, const unsigned char* consistent,
                            const int* ids, int n_images, const float* const* kxy, const int* pose_ids, const msfm_pose_rt* poses,
                            int n_poses, const double* cam, double max_error, double min_angle, int min_views, long long first,
                            long long count, msfm_point3d* out_points, double* out_residuals) {
    const host_map m = raw_map(offsets, image_ids, point_idx, consistent, 0, ids, n_images, kxy, pose_ids, poses, n_poses, cam, max_error,
                               min_angle, min_views, first, count, out_points, out_residuals, nullptr, 0);
    return twin_triangulate_tracks(&m);
}
int host_triangulate_tracks_robust_trace(const long long* offsets, const int* image_ids, const int* point_idx, const unsigned char* consistent,
                                         const int* ids, int n_images, const float* const* kxy, const int* pose_ids, const msfm_pose_rt* poses,
                                         int n_poses, const double* cam, double max_error, double min_angle, int min_views,
                                         int max_hypotheses, long long first, long long count, msfm_point3d* out_points,
                                         double* out_residuals, unsigned char* out_mask, long long* counts4, int* out_trace) {
    const host_map m = raw_map(offsets, image_ids, point_idx, consistent, 0, ids, n_images, kxy, pose_ids, poses, n_poses, cam, max_error,
                               min_angle, min_views, first, count, out_points, out_residuals, out_mask, 0);
    return twin_triangulate_tracks_robust(&m, max_hypotheses, counts4, out_trace);
}
int host_triangulate_tracks_robust(const long long* offsets, const int* image_ids, const int* point_idx, const unsigned char* consistent,
                                   const int* ids, int n_images, const float* const* kxy, const int* pose_ids, const msfm_pose_rt* poses,
                                   int n_poses, const double* cam, double max_error, double min_angle, int min_views, int max_hypotheses,
                                   long long first, long long count, msfm_point3d* out_points, double* out_residuals,
                                   unsigned char* out_mask, long long* counts4) {
    return host_triangulate_tracks_robust_trace(offsets, image_ids, point_idx, consistent, ids, n_images, kxy, pose_ids, poses, n_poses, cam,
                                                max_error, min_angle, min_views, max_hypotheses, first, count, out_points, out_residuals,
                                                out_mask, counts4, nullptr);
}
int host_refine_points(const long long* offsets, const int* image_ids, const int* point_idx, const int* ids, int n_images,
                       const float* const* kxy, const int* pose_ids, const msfm_pose_rt* poses, int n_poses, const double* cam,
                       double max_error, double min_angle, double step_tol, int max_iters, long long first, long long count,
                       msfm_point3d* points, double* residuals, const unsigned char* mask, long long* counts5, double* costs2,
                       void* out_trace) {
    const host_map m = raw_map(offsets, image_ids, point_idx, nullptr, 0, ids, n_images, kxy, pose_ids, poses, n_poses, cam, max_error,
                               min_angle, 0, first, count, points, residuals, mask, 0);
    return twin_refine_points(&m, step_tol, max_iters, counts5, costs2, out_trace);
}
int host_refine_poses(const long long* offsets, const int* image_ids, const int* point_idx, long long n_tracks, const int* ids, int n_images,
                      const float* const* kxy, const int* pose_ids, msfm_pose_rt* poses, int n_poses, const double* cam, double max_error,
                      double min_angle, double step_tol, int max_iters, int min_observations, const int* fixed_ids, int n_fixed,
                      msfm_point3d* points, double* residuals, const unsigned char* mask, msfm_pose_refinement* out_records,
                      long long* counts9, double* costs2, void* out_trace) {
    host_map m = raw_map(offsets, image_ids, point_idx, nullptr, n_tracks, ids, n_images, kxy, pose_ids, poses, n_poses, cam, max_error,
                         min_angle, 0, 0, n_tracks, points, residuals, mask, 0);
    return twin_refine_poses(&m, step_tol, max_iters, min_observations, fixed_ids, n_fixed, out_records, counts9, costs2, out_trace);
}
int host_refine_camera(const long long* offsets, const int* image_ids, const int* point_idx, long long n_tracks, const int* ids, int n_images,
                       const float* const* kxy, const int* pose_ids, const msfm_pose_rt* poses, int n_poses, double* cam, double max_error,
                       double min_angle, double step_tol, int mask_bits, int max_iters, int min_observations, msfm_point3d* points,
                       double* residuals, const unsigned char* mask, long long* counts12, double* costs2, void* out_trace) {
    host_map m = raw_map(offsets, image_ids, point_idx, nullptr, n_tracks, ids, n_images, kxy, pose_ids, poses, n_poses, cam, max_error,
                         min_angle, 0, 0, n_tracks, points, residuals, mask, 0);
    const int rc = twin_refine_camera(&m, step_tol, mask_bits, max_iters, min_observations, counts12, costs2, out_trace);
    for (int k = 0; k < 8; ++k) cam[k] = m.cam[k];   // (the refined camera; the given one where the twin refused)
    return rc;
}
int host_extend_points(const long long* offsets, const int* image_ids, const int* point_idx, const unsigned char* consistent, const int* ids,
                       int n_images, const float* const* kxy, const int* pose_ids, const msfm_pose_rt* poses, int n_poses, const int* new_ids,
                       int n_new, const double* cam, double max_error, double min_angle, int min_views, int max_hypotheses, long long first,
                       long long count, msfm_point3d* points, double* residuals, unsigned char* mask, int have_mask, long long* counts7,
                       int* out_trace) {
    const host_map m = raw_map(offsets, image_ids, point_idx, consistent, 0, ids, n_images, kxy, pose_ids, poses, n_poses, cam, max_error,
                               min_angle, min_views, first, count, points, residuals, mask, have_mask);
    return twin_extend_points(&m, new_ids, n_new, max_hypotheses, counts7, out_trace);
}
int host_filter_points(const long long* offsets, const int* image_ids, const int* point_idx, const unsigned char* consistent, const int* ids,
                       int n_images, const float* const* kxy, const int* pose_ids, const msfm_pose_rt* poses, int n_poses,
                       const int* scope_ids, int n_scope, const double* cam, double max_error, double min_angle, double flt_max_error,
                       double flt_min_angle, long long first, long long count, msfm_point3d* points, double* residuals, unsigned char* mask,
                       int have_mask, long long* counts7, int* out_trace) {
    const host_map m = raw_map(offsets, image_ids, point_idx, consistent, 0, ids, n_images, kxy, pose_ids, poses, n_poses, cam, max_error,
                               min_angle, 0, first, count, points, residuals, mask, have_mask);
    return twin_filter_points(&m, scope_ids, n_scope, flt_max_error, flt_min_angle, counts7, out_trace);
}
int host_complete_points(const long long* offsets, const int* image_ids, const int* point_idx, const unsigned char* consistent,
                         const int* ids, int n_images, const float* const* kxy, const int* pose_ids, const msfm_pose_rt* poses, int n_poses,
                         const int* scope_ids, int n_scope, const double* cam, double max_error, double min_angle, double cmp_max_error,
                         long long first, long long count, msfm_point3d* points, double* residuals, unsigned char* mask, int have_mask,
                         long long* counts6, int* out_trace) {
    const host_map m = raw_map(offsets, image_ids, point_idx, consistent, 0, ids, n_images, kxy, pose_ids, poses, n_poses, cam, max_error,
                               min_angle, 0, first, count, points, residuals, mask, have_mask);
    return twin_complete_points(&m, scope_ids, n_scope, cmp_max_error, counts6, out_trace);
}
int host_map_visibility(const long long* offsets, const int* image_ids, const unsigned char* consistent, long long n_tracks, const int* ids,
                        int n_images, const int* pose_ids, const msfm_pose_rt* poses, int n_poses, const int* query_ids, int n_query, int basis,
                        const msfm_point3d* points, const unsigned char* mask, msfm_image_visibility* out_records, unsigned* out_matrix,
                        long long* counts3) {
    const double cam[8] = {1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // (no pixel is read: only the poses' validity)
    const host_map m = raw_map(offsets, image_ids, nullptr, consistent, n_tracks, ids, n_images, nullptr, pose_ids, poses, n_poses, cam, 0.0, 0.0,
                               0, 0, n_tracks, points, nullptr, mask, 0);
    return twin_map_visibility(&m, query_ids, n_query, basis, out_records, out_matrix, counts3);
}

// msfm_vis::vis_route: out4 = route (0: ROUTE_LDS asked for and no fit), lds_bytes, matrix_in_lds, wgs_per_cu
void host_vis_route(int want, long long n, long long n_query, long long T, long long O, int* out4) {
    const msfm_vis::Route r = msfm_vis::vis_route(want, n, n_query, T, O);
    out4[0] = r.route;
    out4[1] = r.lds_bytes;
    out4[2] = r.matrix_in_lds;
    out4[3] = r.wgs_per_cu;
}

// pieces, for tests/test_triangulation_reference.py
void host_tri_centre(const double* R, const double* t, double* O) { msfm_tri::centre(R, t, O); }
double host_tri_parallax(const double* X, const double* Oi, const double* Oj) { return msfm_tri::parallax(X, Oi, Oj); }

// ---- image registration: the host twin of the device kernels (csrc/msfm_register.h, RegisterImages) ---------------------------------
// A finished track result and its points (msfm_fetch_tracks / msfm_fetch_points3d), the list of images to register with kxy[k] = the
// (x, y) fp32 pairs of list_ids[k], cam = fx, fy, cx, cy, k1, k2, p1, p2.  host_register_counts: the correspondences per listed image.
// host_register_images: the images [first, first + count) of the list, written at their own positions (out_offsets: n_list + 1, the
// running sum of the counts), so that several threads can share one result.  Return 0; 1: an id twice in the list; 2: an id outside
// [0, MSFM_MAX_IMAGES).
static int reg_positions(const int* list_ids, int n_list, std::vector<int>* pos) {
    pos->assign((size_t)MSFM_MAX_IMAGES, -1);
    for (int k = 0; k < n_list; ++k) {
        if (list_ids[k] < 0 || list_ids[k] >= MSFM_MAX_IMAGES) return 2;
        if ((*pos)[(size_t)list_ids[k]] >= 0) return 1;
        (*pos)[(size_t)list_ids[k]] = k;
    }
    return 0;
}

int host_register_counts(const long long* offsets, const int* image_ids, long long n_tracks, const msfm_point3d* points,
                         const int* list_ids, int n_list, long long* counts) {
    std::vector<int> pos;
    if (const int rc = reg_positions(list_ids, n_list, &pos)) return rc;
    msfm_reg::CountCorrespondences(reinterpret_cast<const int64_t*>(offsets), image_ids, n_tracks, points, pos.data(), n_list,
                                   reinterpret_cast<int64_t*>(counts));
    return 0;
}

int host_register_images(const long long* offsets, const int* image_ids, const int* point_idx, long long n_tracks,
                         const msfm_point3d* points, const int* list_ids, int n_list, const float* const* kxy, const double* cam,
                         double max_error, double confidence, int max_iters, int min_inliers, int refine_iters,
                         const long long* out_offsets, int first, int count, msfm_registration* records, int* out_tid,
                         unsigned char* out_flags, double* out_residuals) {
    std::vector<int> pos;
    if (const int rc = reg_positions(list_ids, n_list, &pos)) return rc;
    const msfm_emat::Camera c{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], cam[6], cam[7]};
    const msfm_reg::Params prm = {max_error, confidence, max_iters, min_inliers, refine_iters, 0};
    msfm_reg::RegisterImages(reinterpret_cast<const int64_t*>(offsets), image_ids, point_idx, n_tracks, points, list_ids, pos.data(), kxy,
                             c, prm, reinterpret_cast<const int64_t*>(out_offsets), first, count, records, out_tid, out_flags,
                             out_residuals);
    return 0;
}

// pieces, for tests/test_registration_reference.py
void host_register_sample3(int image_id, int it, int n, int* idx3) { msfm_reg::sample3(msfm_reg::reg_seed(image_id), it, n, idx3); }
// u[3], v[3]: normalised observations; X[9]: the three points; poses48: up to 4 x (R[9] | t[3]); returns the number of poses
int host_p3p(const double* u, const double* v, const double* X, double* poses48) { return msfm_reg::p3p<1>(u, v, X, poses48); }
// `steps` refinement steps of (R, t) on n correspondences (all of them inliers); returns the steps taken
int host_register_refine(const double* cu, const double* cv, const double* cX, const double* cY, const double* cZ, int n, int steps,
                         double* R, double* t) {
    int done = 0;
    for (; done < steps; ++done) {
        double part[msfm_reg::kRegRound][msfm_reg::kRegSums];
        msfm_reg::partial_sums(R, t, cu, cv, cX, cY, cZ, nullptr, n, part);
        if (!msfm_reg::gn_step(part[0], R, t)) break;
    }
    return done;
}

}  // extern "C"
