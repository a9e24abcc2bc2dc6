// msfm_hmat.h -- homography arithmetic shared by the device kernels (msfm_verify_h.hip.h, hipcc) and the host twin
// (host/GeometricVerification.cpp, g++): the verification of planar and rotation-only pairs (msfm_set_verification_model(.., 2,
// NULL)), the check the reference runs itself with cv::findHomography beside findFundamentalMat when it picks its initial pair
// (src/Reconstruction/Initializer.cpp:38-66).
//
// The contract of msfm_fmat.h holds here too: fp64 with +, -, *, / only, static loop structure, -ffp-contract=off on both sides
// -> the host twin and the device produce the SAME bits.  The points are the keypoints' pixel coordinates (as for F and for
// findHomography): no camera, no undistortion.
//
//   sample          4 distinct indices from the counter-based stream of sample8 (sample4: k < 4, as sample5 is derived).
//   subset check    OpenCV's checkSubset for homographies: for each of the triples (0 1 2) (1 2 3) (0 2 3) (0 1 3) the sign of the
//                   orientation determinant in image 1 against the one in image 2; the sample is kept only when all four agree or
//                   all four flip.  A triple that is collinear in either image rejects the sample too: collinear when
//                   det^2 <= kCollinearSin^2 |b - a|^2 |c - a|^2, i.e. the sine of the angle at a is at most kCollinearSin (coincident
//                   points included).  A rejected sample is a hypothesis with count 0.
//   solver          Hartley normalisation of the 4 points of each image (centroid to the origin, mean distance sqrt(2): the
//                   isotropic form, msfm_fmat::normalizer); the 8 x 9 DLT system; its null vector from the Householder QR of its
//                   transpose (the 9 x 8 factorisation of msfm_emat.h's five_point, but fully unrolled: every index is a
//                   compile-time constant, so on the device the 72 doubles stay in registers and nothing goes to scratch);
//                   denormalised, scaled to unit Frobenius norm, sign such that the entry of largest magnitude (lowest index among
//                   equal ones) is positive.
//   error           findHomography's one-sided squared reprojection error |x2 - pi(H x1)|^2; inlier when <= threshold^2.  A
//                   projected w that is 0 or not finite makes the match an outlier.
//   stopping rule   msfm_fmat::replay_adaptive<4>; the highest count wins, the lowest index among equal counts; a winner needs
//                   >= 4 inliers, n < 4 keeps nothing.
//   no refit        findHomography refines the winner by Levenberg-Marquardt, but the mask it returns is RANSAC's: the mask here
//                   is the winning hypothesis's, with no refinement.
#pragma once

#include "msfm_fmat.h"

namespace msfm_hmat {

using msfm_fmat::mix64;

constexpr double kCollinearSin = 1e-6;   // a triple whose angle at its first point has |sin| <= this is collinear

// the 4 distinct match indices of hypothesis `it` (n >= 4): sample8's stream, k < 4
MSFM_FHD void sample4(unsigned long long seed, int it, int n, int idx[4]) {
MSFM_UNROLL
    for (int k = 0; k < 4; ++k) idx[k] = -1;
MSFM_UNROLL
    for (int k = 0; k < 4; ++k) {
        int c = 0;
        for (int attempt = 0;; ++attempt) {
            c = attempt < 32 ? (int)(mix64(seed ^ mix64(((unsigned long long)it << 20) ^ ((unsigned long long)k << 8) ^ (unsigned long long)attempt)) % (unsigned long long)n)
                             : (c + 1) % n;  // linear probe: terminates because n >= 4
            bool dup = false;
MSFM_UNROLL
            for (int j = 0; j < 4; ++j) dup |= (idx[j] == c);
            if (!dup) break;
        }
        idx[k] = c;
    }
}

// orientation determinant of the triangle (a, b, c), det [[ax ay 1] [bx by 1] [cx cy 1]] = (b - a) x (c - a); *collinear when the
// sine of the angle at a is at most kCollinearSin
MSFM_FHD double orient(double ax, double ay, double bx, double by, double cx, double cy, bool* collinear) {
    const double ux = bx - ax, uy = by - ay, vx = cx - ax, vy = cy - ay;
    const double det = ux * vy - uy * vx;
    const double uu = ux * ux + uy * uy, vv = vx * vx + vy * vy;
    *collinear = det * det <= (kCollinearSin * kCollinearSin) * (uu * vv);
    return det;
}

// OpenCV's checkSubset for homographies plus the collinearity test: true when the sample may be solved
MSFM_FHD bool check_subset(const double x1[4], const double y1[4], const double x2[4], const double y2[4]) {
    constexpr int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    int negative = 0;
    bool degenerate = false;
MSFM_UNROLL
    for (int q = 0; q < 4; ++q) {
        const int a = tt[q][0], b = tt[q][1], c = tt[q][2];
        bool c1, c2;
        const double d1 = orient(x1[a], y1[a], x1[b], y1[b], x1[c], y1[c], &c1);
        const double d2 = orient(x2[a], y2[a], x2[b], y2[b], x2[c], y2[c], &c2);
        degenerate |= c1 || c2;
        negative += d1 * d2 < 0.0 ? 1 : 0;
    }
    return !degenerate && (negative == 0 || negative == 4);
}

// Four-point solver: H (row-major, x2 ~ H x1) of the 4 correspondences in pixel coordinates, unit Frobenius norm, deterministic
// sign.  false when the normalised system has no usable null vector (cannot happen after check_subset; kept as a guard).
MSFM_FHD bool four_point(const double x1[4], const double y1[4], const double x2[4], const double y2[4], double Hout[9]) {
    // Hartley normalisation of each image's 4 points
    double c1x = 0.0, c1y = 0.0, c2x = 0.0, c2y = 0.0;
MSFM_UNROLL
    for (int k = 0; k < 4; ++k) {
        c1x += x1[k];
        c1y += y1[k];
        c2x += x2[k];
        c2y += y2[k];
    }
    c1x /= 4.0;
    c1y /= 4.0;
    c2x /= 4.0;
    c2y /= 4.0;
    double d1 = 0.0, d2 = 0.0;
MSFM_UNROLL
    for (int k = 0; k < 4; ++k) {
        const double ax = x1[k] - c1x, ay = y1[k] - c1y, bx = x2[k] - c2x, by = y2[k] - c2y;
        d1 += sqrt(ax * ax + ay * ay);
        d2 += sqrt(bx * bx + by * by);
    }
    d1 /= 4.0;
    d2 /= 4.0;
    const double s1 = d1 > 1e-12 ? 1.4142135623730951 / d1 : 1.0;
    const double s2 = d2 > 1e-12 ? 1.4142135623730951 / d2 : 1.0;
    // A^T (9 x 8): column 2k and 2k + 1 are the DLT rows of correspondence k
    //   [x y 1 0 0 0 -u x -u y -u] and [0 0 0 x y 1 -v x -v y -v]
    double a[8][9];
MSFM_UNROLL
    for (int k = 0; k < 4; ++k) {
        const double x = (x1[k] - c1x) * s1, y = (y1[k] - c1y) * s1;
        const double u = (x2[k] - c2x) * s2, v = (y2[k] - c2y) * s2;
        const double r0[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -(u * x), -(u * y), -u};
        const double r1[9] = {0.0, 0.0, 0.0, x, y, 1.0, -(v * x), -(v * y), -v};
MSFM_UNROLL
        for (int i = 0; i < 9; ++i) {
            a[2 * k][i] = r0[i];
            a[2 * k + 1][i] = r1[i];
        }
    }
    // Householder QR of A^T: column j's reflector v_j overwrites rows j.. of column j; beta_j = 2 / |v_j|^2
    double beta[8];
MSFM_UNROLL
    for (int j = 0; j < 8; ++j) {
        double nn = 0.0;
MSFM_UNROLL
        for (int i = j; i < 9; ++i) nn += a[j][i] * a[j][i];
        const double a0 = a[j][j];
        const double nrm = sqrt(nn);
        const double alpha = a0 >= 0.0 ? -nrm : nrm;
        const double v0 = a0 - alpha;
        const double vv = nn - a0 * a0 + v0 * v0;
        beta[j] = vv > 0.0 ? 2.0 / vv : 0.0;
        a[j][j] = v0;
MSFM_UNROLL
        for (int c = j + 1; c < 8; ++c) {
            double d = 0.0;
MSFM_UNROLL
            for (int i = j; i < 9; ++i) d += a[j][i] * a[c][i];
            d *= beta[j];
MSFM_UNROLL
            for (int i = j; i < 9; ++i) a[c][i] -= d * a[j][i];
        }
    }
    // null vector Q e_8 = H_0 H_1 .. H_7 e_8
    double h[9];
MSFM_UNROLL
    for (int i = 0; i < 9; ++i) h[i] = i == 8 ? 1.0 : 0.0;
MSFM_UNROLL
    for (int j = 7; j >= 0; --j) {
        double d = 0.0;
MSFM_UNROLL
        for (int i = j; i < 9; ++i) d += a[j][i] * h[i];
        d *= beta[j];
MSFM_UNROLL
        for (int i = j; i < 9; ++i) h[i] -= d * a[j][i];
    }
    // denormalise: H = T2^-1 Hn T1, T1 = [s1 0 -s1 c1x; 0 s1 -s1 c1y; 0 0 1], T2^-1 = [1/s2 0 c2x; 0 1/s2 c2y; 0 0 1]
    double m[9];   // Hn T1
MSFM_UNROLL
    for (int r = 0; r < 3; ++r) {
        const double p = h[3 * r], q = h[3 * r + 1], w = h[3 * r + 2];
        m[3 * r] = p * s1;
        m[3 * r + 1] = q * s1;
        m[3 * r + 2] = w - (p * (s1 * c1x) + q * (s1 * c1y));
    }
    const double is2 = 1.0 / s2;
    double H[9];
MSFM_UNROLL
    for (int c = 0; c < 3; ++c) {
        H[c] = m[c] * is2 + c2x * m[6 + c];
        H[3 + c] = m[3 + c] * is2 + c2y * m[6 + c];
        H[6 + c] = m[6 + c];
    }
    // unit Frobenius norm; the entry of largest magnitude (lowest index among equal ones) positive
    double nn = 0.0, big = 0.0, sgn = 1.0;
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) {
        nn += H[k] * H[k];
        const double ak = H[k] >= 0.0 ? H[k] : -H[k];
        if (ak > big) {
            big = ak;
            sgn = H[k] >= 0.0 ? 1.0 : -1.0;
        }
    }
    if (!(nn > 0.0) || !(nn - nn == 0.0)) return false;   // zero, NaN or inf
    const double inv = sgn / sqrt(nn);
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) Hout[k] = H[k] * inv;
    return true;
}

// findHomography's error: |(u, v) - pi(H (x, y, 1))|^2; a projected w of 0 or not finite is +inf (an outlier)
MSFM_FHD double reproj_error(const double H[9], double x, double y, double u, double v) {
    const double w = H[6] * x + H[7] * y + H[8];
    if (!(w != 0.0) || !(w - w == 0.0)) return __builtin_inf();
    const double ww = 1.0 / w;
    const double dx = (H[0] * x + H[1] * y + H[2]) * ww - u;
    const double dy = (H[3] * x + H[4] * y + H[5]) * ww - v;
    return dx * dx + dy * dy;   // NaN (an infinite H entry) fails the <= test
}

// hypothesis `it` of a pair with n >= 4 matches (pixel coordinates): false when the sample is rejected (count 0)
MSFM_FHD bool hypothesis(const float* x1, const float* y1, const float* x2, const float* y2, int n, unsigned long long seed, int it,
                         double H[9]) {
    int idx[4];
    sample4(seed, it, n, idx);
    double a[4], b[4], c[4], d[4];
MSFM_UNROLL
    for (int k = 0; k < 4; ++k) {
        a[k] = (double)x1[idx[k]];
        b[k] = (double)y1[idx[k]];
        c[k] = (double)x2[idx[k]];
        d[k] = (double)y2[idx[k]];
    }
    if (!check_subset(a, b, c, d)) return false;
    return four_point(a, b, c, d, H);
}

}  // namespace msfm_hmat
