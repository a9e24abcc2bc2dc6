// msfm_pose.h -- two-view geometry arithmetic shared by the device kernel (msfm_verify_pose.hip.h, hipcc) and the host twin
// (host/GeometricVerification.cpp, TwoViewGeometry, g++): what the reference's Initializer computes after it has chosen a model
// (src/Reconstruction/Initializer.cpp:300-420, cv::recoverPose + Triangulate + the statistics of RecoverPoseFromFundanmental),
// from the winning E of the calibrated verification (msfm_emat.h) and the pair's kept matches (the nE E-inliers, in list order, as
// normalised undistorted coordinates).  The pose of a homography is NOT computed: a pair whose H list was kept by the model
// selection gets an invalid record.
//
// The contract of msfm_fmat.h / msfm_emat.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on
// both sides -> the host twin and the device produce the SAME bits.  The one exception is the bits of a NaN, which belong to the
// processor: every double that can be NaN where it is stored to an output goes through canonical() below ("THE NaN RULE"), so the
// outputs agree there too.
//
//   decomposition    one-sided (Hestenes) Jacobi on the columns of E, kSvdSweeps fixed cyclic sweeps: E V = U S.  The columns are
//                    ordered by norm with a fixed compare-and-swap network; u1, u2 are the two largest ones normalised,
//                    u3 = u1 x u2, v3 = v1 x v2 (so det U = det V = +1 and both rotations are proper by construction):
//                        R' = u2 v1^T - u1 v2^T + u3 v3^T  (U W V^T),   R'' = -u2 v1^T + u1 v2^T + u3 v3^T  (U W^T V^T),   t' = u3.
//                    Ra is the one of R', R'' with the larger trace (the smaller rotation angle; R' when equal), Rb the other; +t is
//                    the sign of t' whose component of largest magnitude (the lowest index among equal ones) is positive.
//                    Candidates, in this order: (Ra, +t), (Ra, -t), (Rb, +t), (Rb, -t).  x2 ~ R x1 + t.
//   triangulation    the reference's DLT (Initializer.cpp:436-463) for P1 = [I | 0], P2 = [R | t]: the right singular vector of the
//                    smallest singular value of the 4 x 4 system, by the same one-sided Jacobi (the column of V whose rotated column
//                    of A has the smallest norm, the lowest index among equal ones).  The Householder null vector of five_point /
//                    four_point does not fit: with noise the system has full rank and the answer is a singular vector, not a null
//                    vector.  w == 0 or a non-finite point: not triangulated.
//   cheirality       Projection::HasPositiveDepth: depth > DBL_EPSILON in both views.  The candidate with the most kept matches in
//                    front of both cameras wins, the lowest index among equal counts; a count of 0 gives an invalid record.
//   per match        reprojection error (Projection.cpp:114-146): the Euclidean distance in each view, the mean of the two, on
//                    the normalised undistorted coordinates, times (fx + fy) / 2 (the reference projects with K alone onto the
//                    distorted pixels; this path compares with the undistorted observation, as the E threshold does).
//                    Triangulation angle (Projection.cpp:171-194): law of cosines, NaN -> 0, min(a, pi - a), degrees; acos() below.
//   statistics       n_triangulated: positive depth and error < tri_max_error; the sums of error and angle over those in a STATED
//                    ORDER: partial sum l (l < kLanes) adds the kept matches l, l + kLanes, l + 2 kLanes, .. in that order,
//                    starting from 0.0; then the tree  for (s = kLanes / 2; s >= 1; s /= 2) part[l] = part[l] + part[l + s], l < s;
//                    the sum is part[0].  Means: the sum divided by n_triangulated (0 when there is none).  The median of the
//                    angles of ALL kept matches is exact (the reference's even rule: the mean of the two middle ones).
//   the rule         msfm_initial_candidate (msfm_hostutil.h).
#pragma once

#include "msfm_emat.h"
#include "msfm_hostutil.h"
#include "msfm_match.h"

#if !defined(__HIPCC__)
#include <algorithm>
#include <vector>
#endif

#if defined(__HIPCC__)
#define MSFM_NOUNROLL _Pragma("nounroll")
#else
#define MSFM_NOUNROLL
#endif

namespace msfm_pose {

constexpr int kLanes = 256;      // partial sums of the statistics = threads of a tv_pose_kernel workgroup
constexpr int kSvdSweeps = 6;    // cyclic sweeps of the one-sided Jacobi (3 x 3 and 4 x 4: converged to the last bits after 4 - 5)
constexpr double kPi = 3.14159265358979323846;
constexpr double kDepthEps = 2.220446049250313e-16;   // std::numeric_limits<double>::epsilon(), Projection.cpp:55
constexpr double kMaxFinite = 1.7976931348623157e308;

MSFM_FHD bool finite(double v) { return v >= -kMaxFinite && v <= kMaxFinite; }   // (false for NaN)

// THE NaN RULE of everything this stage hands out.  Keypoint coordinates are not validated (msfm_upload_keypoints): a NaN, an
// infinity or a huge coordinate reaches the arithmetic, and every decision on it is written so that a NaN FAILS (err <= max_error,
// depth > kDepthEps, h[3] != 0, finite(X) are all false for one), which makes its observation a gross outlier.  The only doubles that
// can then be NaN in an output are the per-observation error slots (residuals), and "the same bits" cannot be asked of a NaN as it
// falls out of the arithmetic: which operand's payload survives an operation, and the sign of a NaN that an operation generates
// (inf - inf, 0 * inf, sqrt(-1)), belong to the processor -- x86 generates 0xfff8000000000000, the GPU 0x7ff8000000000000.  So every
// double that can be NaN goes through canonical() where it is stored to an output: v itself when v == v (infinities included), else
// THE NaN 0x7ff8000000000000, built from these bits and not from arithmetic.
constexpr unsigned long long kCanonicalNaN = 0x7ff8000000000000ULL;
MSFM_FHD double canonical(double v) {
    double q;
    const unsigned long long bits = kCanonicalNaN;
    __builtin_memcpy(&q, &bits, sizeof q);
    return v == v ? v : q;
}

// asin(z) = z * sum_k c_k z^2k for |z| <= 1/2: c_0 = 1, c_k = c_{k-1} (2k - 1)^2 / (2k (2k + 1)), k < 22 (the first term left out is
// below 1e-16 there)
constexpr int kAsinTerms = 22;
constexpr double kAsin[kAsinTerms] = {1.0, 0.16666666666666666, 0.075, 0.044642857142857144, 0.030381944444444444, 0.022372159090909092,
                                      0.017352764423076924, 0.01396484375, 0.011551800896139705, 0.009761609529194078,
                                      0.008390335809616815, 0.0073125258735988454, 0.006447210311889649, 0.005740037670841924,
                                      0.005153309682319905, 0.004660143486915096, 0.004240907093679363, 0.003880964558837669,
                                      0.0035692053938259347, 0.003297059503473485, 0.0030578216492580306, 0.002846178401108942};
MSFM_FHD double asin_half(double z) {
    const double z2 = z * z;
    double p = kAsin[kAsinTerms - 1];
MSFM_UNROLL
    for (int k = kAsinTerms - 2; k >= 0; --k) p = p * z2 + kAsin[k];
    return z * p;
}
// acos on [-1, 1] to 1e-12 absolute (tests/test_pose_reference.py): pi / 2 - asin(x) for |x| <= 1/2, else the half-angle forms
// 2 asin(sqrt((1 - x) / 2)) and pi - 2 asin(sqrt((1 + x) / 2)).  NaN outside [-1, 1] (the square root of a negative number).
MSFM_FHD double acos(double x) {
    if (x > 0.5) return 2.0 * asin_half(sqrt((1.0 - x) * 0.5));
    if (x < -0.5) return kPi - 2.0 * asin_half(sqrt((1.0 + x) * 0.5));
    return kPi * 0.5 - asin_half(x);
}

// One-sided Jacobi: the N columns a[j][0 .. M) of a matrix are rotated in pairs until they are orthogonal (A V = U S); v[j][0 .. N)
// is column j of V.  Cyclic order (0,1) (0,2) .. (N-2,N-1), kSvdSweeps sweeps, a pair with an exactly zero inner product is skipped.
template <int M, int N>
MSFM_FHD void onesided_jacobi(double a[N][M], double v[N][N]) {
MSFM_UNROLL
    for (int j = 0; j < N; ++j)
MSFM_UNROLL
        for (int k = 0; k < N; ++k) v[j][k] = j == k ? 1.0 : 0.0;
MSFM_NOUNROLL
    for (int sweep = 0; sweep < kSvdSweeps; ++sweep) {
MSFM_UNROLL
        for (int p = 0; p < N - 1; ++p)
MSFM_UNROLL
            for (int q = p + 1; q < N; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
MSFM_UNROLL
                for (int k = 0; k < M; ++k) {
                    alpha += a[p][k] * a[p][k];
                    beta += a[q][k] * a[q][k];
                    gamma += a[p][k] * a[q][k];
                }
                if (gamma > 0.0 || gamma < 0.0) {
                    const double zeta = (beta - alpha) / (2.0 * gamma);
                    const double az = zeta >= 0.0 ? zeta : -zeta;
                    double tt = 1.0 / (az + sqrt(1.0 + zeta * zeta));
                    if (zeta < 0.0) tt = -tt;
                    const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
MSFM_UNROLL
                    for (int k = 0; k < M; ++k) {
                        const double ap = a[p][k], aq = a[q][k];
                        a[p][k] = c * ap - s * aq;
                        a[q][k] = s * ap + c * aq;
                    }
MSFM_UNROLL
                    for (int k = 0; k < N; ++k) {
                        const double vp = v[p][k], vq = v[q][k];
                        v[p][k] = c * vp - s * vq;
                        v[q][k] = s * vp + c * vq;
                    }
                }
            }
    }
}

// The four candidates of E (row-major, x2^T E x1 = 0), each as 12 doubles R[9] (row-major) | t[3] at cand + 12 c * S, in the order
// of the header comment.  False (cand untouched) when E has fewer than two non-zero singular values or is not finite.
template <int S>
MSFM_FHD bool decompose(const double E[9], double* cand) {
    double a[3][3], v[3][3], n[3];
MSFM_UNROLL
    for (int j = 0; j < 3; ++j)
MSFM_UNROLL
        for (int i = 0; i < 3; ++i) a[j][i] = E[3 * i + j];
    onesided_jacobi<3, 3>(a, v);
MSFM_UNROLL
    for (int j = 0; j < 3; ++j) n[j] = a[j][0] * a[j][0] + a[j][1] * a[j][1] + a[j][2] * a[j][2];
    // descending by norm: compare-and-swap (0,1) (1,2) (0,1), whole columns, no runtime indexing
MSFM_UNROLL
    for (int step = 0; step < 3; ++step) {
        const int p = step == 1 ? 1 : 0, q = p + 1;
        const bool sw = n[q] > n[p];
        const double np = n[p], nq = n[q];
        n[p] = sw ? nq : np;
        n[q] = sw ? np : nq;
MSFM_UNROLL
        for (int k = 0; k < 3; ++k) {
            const double ap = a[p][k], aq = a[q][k], vp = v[p][k], vq = v[q][k];
            a[p][k] = sw ? aq : ap;
            a[q][k] = sw ? ap : aq;
            v[p][k] = sw ? vq : vp;
            v[q][k] = sw ? vp : vq;
        }
    }
    if (!(n[1] > 0.0) || !finite(n[0])) return false;
    const double i0 = 1.0 / sqrt(n[0]), i1 = 1.0 / sqrt(n[1]);
    const double u1[3] = {a[0][0] * i0, a[0][1] * i0, a[0][2] * i0}, u2[3] = {a[1][0] * i1, a[1][1] * i1, a[1][2] * i1};
    const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
    const double* v1 = v[0];
    const double* v2 = v[1];
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    double R1[9], R2[9];
    bool ok = true;
MSFM_UNROLL
    for (int i = 0; i < 3; ++i)
MSFM_UNROLL
        for (int j = 0; j < 3; ++j) {
            const double w = u2[i] * v1[j] - u1[i] * v2[j], z = u3[i] * v3[j];
            R1[3 * i + j] = w + z;
            R2[3 * i + j] = z - w;
            ok = ok && finite(R1[3 * i + j]) && finite(R2[3 * i + j]);
        }
    if (!ok) return false;
    const bool first = (R1[0] + R1[4] + R1[8]) >= (R2[0] + R2[4] + R2[8]);
    // +t: the component of largest magnitude positive
    const double m0 = u3[0] >= 0.0 ? u3[0] : -u3[0], m1 = u3[1] >= 0.0 ? u3[1] : -u3[1], m2 = u3[2] >= 0.0 ? u3[2] : -u3[2];
    const double lead = (m0 >= m1 && m0 >= m2) ? u3[0] : (m1 >= m2 ? u3[1] : u3[2]);
    const double sg = lead < 0.0 ? -1.0 : 1.0;
MSFM_UNROLL
    for (int c = 0; c < 4; ++c) {
        const bool ra = c < 2;
MSFM_UNROLL
        for (int k = 0; k < 9; ++k) cand[(12 * c + k) * S] = (ra == first) ? R1[k] : R2[k];
MSFM_UNROLL
        for (int k = 0; k < 3; ++k) cand[(12 * c + 9 + k) * S] = (c & 1) ? -(sg * u3[k]) : sg * u3[k];
    }
    return true;
}

// DLT point of (x1, y1) <-> (x2, y2) under P1 = [I | 0], P2 = [R | t] (P = R[9] | t[3]).  False: not triangulated.
MSFM_FHD bool triangulate(const double* P, double x1, double y1, double x2, double y2, double X[3]) {
    double a[4][4], v[4][4];   // a[j][i]: column j, row i
MSFM_UNROLL
    for (int j = 0; j < 4; ++j) {
        const double p0 = j < 3 ? P[j] : P[9], p1 = j < 3 ? P[3 + j] : P[10], p2 = j < 3 ? P[6 + j] : P[11];
        a[j][0] = x1 * (j == 2 ? 1.0 : 0.0) - (j == 0 ? 1.0 : 0.0);
        a[j][1] = y1 * (j == 2 ? 1.0 : 0.0) - (j == 1 ? 1.0 : 0.0);
        a[j][2] = x2 * p2 - p0;
        a[j][3] = y2 * p2 - p1;
    }
    onesided_jacobi<4, 4>(a, v);
    double best = 0.0, h[4] = {0.0, 0.0, 0.0, 0.0};
MSFM_UNROLL
    for (int j = 0; j < 4; ++j) {
        const double nn = a[j][0] * a[j][0] + a[j][1] * a[j][1] + a[j][2] * a[j][2] + a[j][3] * a[j][3];
        if (j == 0 || nn < best) {
            best = nn;
MSFM_UNROLL
            for (int k = 0; k < 4; ++k) h[k] = v[j][k];
        }
    }
    if (!(h[3] > 0.0 || h[3] < 0.0)) return false;
    X[0] = h[0] / h[3];
    X[1] = h[1] / h[3];
    X[2] = h[2] / h[3];
    return finite(X[0]) && finite(X[1]) && finite(X[2]);
}

// Projection::HasPositiveDepth in both views
MSFM_FHD bool positive_depth(const double* P, const double X[3]) {
    const double z2 = P[6] * X[0] + P[7] * X[1] + P[8] * X[2] + P[11];
    return X[2] > kDepthEps && z2 > kDepthEps;
}

// a kept match in front of both cameras under candidate P (the cheirality count)
MSFM_FHD bool in_front(const double* P, double x1, double y1, double x2, double y2) {
    double X[3];
    return triangulate(P, x1, y1, x2, y2, X) && positive_depth(P, X);
}

// One kept match under the winner P: *depth (false when not triangulated), *err in pixels (f = (fx + fy) / 2), *angle in degrees
// (0 when not triangulated).
MSFM_FHD void evaluate(const double* P, double f, double x1, double y1, double x2, double y2, bool* depth, double* err, double* angle) {
    double X[3];
    *depth = false;
    *err = kMaxFinite;
    *angle = 0.0;
    if (!triangulate(P, x1, y1, x2, y2, X)) return;
    *depth = positive_depth(P, X);
    double Y[3], O[3];
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) {
        Y[k] = P[3 * k] * X[0] + P[3 * k + 1] * X[1] + P[3 * k + 2] * X[2] + P[9 + k];
        O[k] = -(P[k] * P[9] + P[3 + k] * P[10] + P[6 + k] * P[11]);   // the second camera's centre, -R^T t
    }
    const double dx1 = X[0] / X[2] - x1, dy1 = X[1] / X[2] - y1, dx2 = Y[0] / Y[2] - x2, dy2 = Y[1] / Y[2] - y2;
    *err = (sqrt(dx1 * dx1 + dy1 * dy1) + sqrt(dx2 * dx2 + dy2 * dy2)) / 2.0 * f;
    const double baseline = sqrt(O[0] * O[0] + O[1] * O[1] + O[2] * O[2]);
    const double ray1 = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
    const double e0 = X[0] - O[0], e1 = X[1] - O[1], e2 = X[2] - O[2];
    const double ray2 = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    double ang = acos((ray1 * ray1 + ray2 * ray2 - baseline * baseline) / (2.0 * ray1 * ray2));
    if (ang < 0.0) ang = -ang;
    if (!(ang == ang)) return;   // NaN -> 0
    const double other = kPi - ang;
    *angle = (ang < other ? ang : other) * 180.0 / kPi;
}

MSFM_FHD void clear_record(msfm_two_view_record* r) {
    r->valid = 0;
    r->reserved = 0;
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) r->R[k] = 0.0;
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) r->t[k] = 0.0;
    r->n_kept = r->n_positive_depth = r->n_triangulated = r->is_initial_candidate = 0;
    r->median_tri_angle = r->mean_tri_angle = r->mean_residual = 0.0;
}

// the record from the winner P (stride S), the counts, the two sums (in the stated order) and the two middle angles of the sorted
// list (lo = sorted[(n - 1) / 2], hi = sorted[n / 2])
template <int S>
MSFM_FHD void finish_record(const double* P, int n_kept, int n_positive_depth, int n_triangulated, double sum_residual, double sum_angle,
                            double lo, double hi, const msfm_two_view_params& prm, msfm_two_view_record* r) {
    r->valid = 1;
    r->reserved = 0;
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) r->R[k] = P[k * S];
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) r->t[k] = P[(9 + k) * S];
    r->n_kept = n_kept;
    r->n_positive_depth = n_positive_depth;
    r->n_triangulated = n_triangulated;
    r->median_tri_angle = (n_kept & 1) ? hi : (lo + hi) / 2.0;
    r->mean_tri_angle = n_triangulated > 0 ? sum_angle / (double)n_triangulated : 0.0;
    r->mean_residual = n_triangulated > 0 ? sum_residual / (double)n_triangulated : 0.0;
    r->is_initial_candidate = msfm_initial_candidate(n_triangulated, r->median_tri_angle, r->mean_tri_angle, r->mean_residual,
                                                     prm.min_num_inliers, prm.tri_max_error, prm.tri_min_angle) ? 1 : 0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The statistics of the n kept matches under the pose P = R[9] | t[3] on the host, literally the definition above (tv_pose_kernel's
// steps 5 and 6): n_positive_depth counts the matches evaluate puts in front of both cameras, the two sums are in the stated order,
// lo / hi are the two middle angles of the sorted list.  The ONE host copy: two_view_record and the refinement's twin
// (msfm_pose_refine.h) both call it.
struct HostStatistics {
    int n_positive_depth, n_triangulated;
    double sum_residual, sum_angle, lo, hi;
};
inline HostStatistics host_statistics(const double* P, const double* x1, const double* y1, const double* x2, const double* y2, int n, double f,
                                      double tri_max_error) {
    std::vector<double> angles((size_t)n), part_r((size_t)kLanes, 0.0), part_a((size_t)kLanes, 0.0);
    int n_pos = 0, n_tri = 0;
    for (int i = 0; i < n; ++i) {   // (lane i % kLanes meets its matches in ascending order)
        bool depth;
        double err, ang;
        evaluate(P, f, x1[i], y1[i], x2[i], y2[i], &depth, &err, &ang);
        angles[(size_t)i] = ang;
        n_pos += depth ? 1 : 0;
        if (depth && err < tri_max_error) {
            n_tri += 1;
            part_r[(size_t)(i % kLanes)] = part_r[(size_t)(i % kLanes)] + err;
            part_a[(size_t)(i % kLanes)] = part_a[(size_t)(i % kLanes)] + ang;
        }
    }
    for (int s = kLanes / 2; s >= 1; s /= 2)
        for (int l = 0; l < s; ++l) {
            part_r[(size_t)l] = part_r[(size_t)l] + part_r[(size_t)(l + s)];
            part_a[(size_t)l] = part_a[(size_t)l] + part_a[(size_t)(l + s)];
        }
    std::sort(angles.begin(), angles.end());
    return HostStatistics{n_pos, n_tri, part_r[0], part_a[0], angles[(size_t)((n - 1) / 2)], angles[(size_t)(n / 2)]};
}

// The whole record of one pair on the host, literally the definition above: E the winner, (x1, y1) <-> (x2, y2) the n kept
// matches in list order, f = (fx + fy) / 2.  `winner` (may be NULL): the candidate index, -1 for an invalid record.
inline void two_view_record(const double E[9], const double* x1, const double* y1, const double* x2, const double* y2, int n, double f,
                            const msfm_two_view_params& prm, msfm_two_view_record* r, int* winner = nullptr) {
    clear_record(r);
    if (winner) *winner = -1;
    double cand[48];
    if (n < 1 || !decompose<1>(E, cand)) return;
    int count[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < 4; ++c) count[c] += in_front(cand + 12 * c, x1[i], y1[i], x2[i], y2[i]) ? 1 : 0;
    int w = 0;
    for (int c = 1; c < 4; ++c)
        if (count[c] > count[w]) w = c;
    if (count[w] == 0) return;
    const double* P = cand + 12 * w;
    const HostStatistics st = host_statistics(P, x1, y1, x2, y2, n, f, prm.tri_max_error);
    finish_record<1>(P, n, count[w], st.n_triangulated, st.sum_residual, st.sum_angle, st.lo, st.hi, prm, r);
    if (winner) *winner = w;
}
#endif

}  // namespace msfm_pose
