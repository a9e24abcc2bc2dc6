// msfm_register.h -- image registration arithmetic shared by the device kernels (msfm_register.hip.h, hipcc) and the host twin
// (host/HostTestApi.cpp, RegisterImages, g++): what the reference's Registrant::Register computes for one unposed image
// (src/Reconstruction/Registrant.cpp: cv::solvePnPRansac over the image's 2D-3D correspondences, then the inlier test) -- P3P RANSAC
// over the image's correspondences with the triangulated tracks, and a Gauss-Newton refinement of the winner.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides -> the host
// twin and the device produce the SAME bits.  undistort is msfm_emat.h's, kDepthEps msfm_pose.h's, transform msfm_triangulate.h's,
// mix64 / replay_adaptive msfm_fmat.h's.
//
//   correspondences the kept tracks with POINT & ERROR_OK & ANGLE_OK that have an element (I, k), by ascending track number (a
//                   triangulated track is consistent: at most one element per image).  (u, v) = undistort(pixel of keypoint k),
//                   X = the track's point.
//   sample3         three distinct indices of hypothesis `it` from sample8's counter stream under the seed reg_seed(image id).
//   p3p             Grunert's method.  Unit bearings j_i = (u_i, v_i, 1) / |.|, cos_a = j2.j3, cos_b = j1.j3, cos_g = j1.j2; squared
//                   distances a2 = |X2 - X3|^2, b2 = |X1 - X3|^2, c2 = |X1 - X2|^2.  With the depths s2 = p s1, s3 = q s1 the law of
//                   cosines gives two quadratics in p whose coefficients are polynomials in q,
//                       p^2 - 2 q cos_a p + q^2 - (a2 / b2) D(q) = 0,   p^2 - 2 cos_g p + 1 - (c2 / b2) D(q) = 0,   D = 1 + q^2 - 2 q cos_b;
//                   their resultant is the quartic g(q) (polynomial arithmetic, no closed form), their difference is linear in p.
//                   Real roots q in (0, B], B = 1 + max |g_i / g_4| (Cauchy): the roots of g'' in closed form (one sqrt) split (0, B]
//                   into intervals where g' is monotone, the roots of g' found there split it into intervals where g is monotone;
//                   a root is taken where the sign changes across an interval, by kRegBisect bisection steps and kRegNewton Newton
//                   steps that are kept while they stay inside the bracket.  (A double root has no sign change: not a solution.)
//                   Where the quadratics COINCIDE at qs = -l0 / l1 (d(qs) and k(qs) within kRegCoincide of their terms' sizes: a
//                   triangle seen along its axis of symmetry) the linear equation is 0 p = 0 and qs is a double root: the roots of g
//                   within kRegCoincideRadius of qs are not used, and both roots p of the second quadratic at qs give poses, last.
//                   Per root, ascending: p from the linear equation, s1 = sqrt(b2 / D(q)); p, q, s1 must be finite and > 0 (a point
//                   behind the camera: no pose).  The pose from the orthonormal frames of the triangles (X1, X2, X3) and
//                   (s1 j1, s2 j2, s3 j3): e1 = d12 / |.|, e3 = d12 x d13 / |.|, e2 = e3 x e1; R = sum_k c_k w_k^T, t = Y1 - R X1.
//                   A sample with |d12 x d13|^2 <= kRegCollinear c2 b2 (collinear or repeated points) or a non-finite pose: no pose.
//   score           inlier(R, t): Y = R X + t; Y.z > kDepthEps and ((Y.x / Y.z - u)^2 + (Y.y / Y.z - v)^2) f^2 <= max_error^2 (a NaN
//                   fails).  A hypothesis counts the largest count of its poses, the lowest index among equal ones.
//   stopping        msfm_fmat::replay_adaptive<3> over the counts; `hypotheses` of the record = min(max_iters, 64 x the rounds of 64
//                   hypotheses the rule needs before it is decided) -- what the staged device form scores.
//   refinement      refine_iters Gauss-Newton steps on the winner's inliers (the list is fixed).  Residual in normalised coordinates,
//                   unknowns (a, dt):  R <- C(a) R,  t <- C(a) t + dt,  C(a) = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a)  (Cayley: an
//                   exact rotation), linearised at a = 0: dY = 2 a x Y + dt.  27 sums (21 of J^T J, 6 of J^T r): partial j < 64 sums
//                   the inliers at positions j, j + 64, .. of the list from 0.0, then the butterfly v_j <- v_j + v_(j xor s) for
//                   s = 32, 16, .., 1 (every j ends with the same bits).  6 x 6 Cholesky; a pivot that is not > 0 or a non-finite
//                   step ends the refinement with the pose before it.  The refined pose is kept iff its inlier count >= the winner's.
//   record          msfm_registration (include/msfm_match.h); residual of EVERY correspondence under the final pose:
//                   sqrt(dx^2 + dy^2) f; mean_residual = (the inliers' residuals summed in list order from 0.0) / n_inliers.
#pragma once

#include "msfm_triangulate.h"

#if !defined(__HIPCC__)
#include <algorithm>
#include <vector>
#endif

namespace msfm_reg {

constexpr int kRegRound = 64;            // hypotheses per round = lanes of a reg_round_kernel workgroup = partial sums
constexpr int kRegBisect = 60;           // bisection steps per root
constexpr int kRegNewton = 3;            // Newton steps inside the final bracket
constexpr double kRegCoincide = 1e-12;        // |d(qs)|, |k(qs)| <= this x their terms' sizes: the two quadratics coincide at qs
constexpr double kRegCoincideRadius = 1e-5;  // roots of g within this (relative) of such a qs are the split double root
constexpr double kRegCollinear = 1e-10;  // |d12 x d13|^2 <= this x |d12|^2 |d13|^2 (an angle below 1e-5 rad): no triangle
constexpr unsigned long long kRegSeed = 0x5265676973746572ULL;

struct Params {
    double max_error, confidence;
    int32_t max_iters, min_inliers, refine_iters, reserved;
};

MSFM_FHD unsigned long long reg_seed(int image_id) { return msfm_fmat::mix64(kRegSeed ^ (unsigned long long)(unsigned)image_id); }

// the 3 distinct correspondence indices of hypothesis `it` (n >= 3): sample8's stream, k < 3
MSFM_FHD void sample3(unsigned long long seed, int it, int n, int idx[3]) {
    using msfm_fmat::mix64;
    idx[0] = idx[1] = idx[2] = -1;
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) {
        int c = 0;
        for (int attempt = 0;; ++attempt) {
            c = attempt < 32 ? (int)(mix64(seed ^ mix64(((unsigned long long)it << 20) ^ ((unsigned long long)k << 8) ^ (unsigned long long)attempt)) % (unsigned long long)n)
                             : (c + 1) % n;  // linear probe: terminates because n >= 3
            if (!(idx[0] == c || idx[1] == c || idx[2] == c)) break;
        }
        idx[k] = c;
    }
}

template <int D>
MSFM_FHD double horner(const double (&c)[D + 1], double x) {
    double v = c[D];
MSFM_UNROLL
    for (int k = D - 1; k >= 0; --k) v = v * x + c[k];
    return v;
}

// the root of the degree-D polynomial c in [lo, hi] if its sign changes across the interval (c is monotone there)
template <int D>
MSFM_FHD bool bracket_root(const double (&c)[D + 1], double lo, double hi, double* root) {
    const double flo = horner<D>(c, lo), fhi = horner<D>(c, hi);
    const bool rising = flo < 0.0 && fhi >= 0.0, falling = flo > 0.0 && fhi <= 0.0;
    if (!(rising || falling)) return false;   // (a NaN: no root)
    for (int k = 0; k < kRegBisect; ++k) {
        const double mid = 0.5 * (lo + hi);
        const double fm = horner<D>(c, mid);
        const bool low = rising ? fm < 0.0 : fm > 0.0;   // mid is still on lo's side
        lo = low ? mid : lo;
        hi = low ? hi : mid;
    }
    double x = 0.5 * (lo + hi);
    double d[D];
MSFM_UNROLL
    for (int k = 0; k < D; ++k) d[k] = (double)(k + 1) * c[k + 1];
    for (int k = 0; k < kRegNewton; ++k) {
        const double xn = x - horner<D>(c, x) / horner<D - 1>(d, x);
        x = (xn >= lo && xn <= hi) ? xn : x;
    }
    *root = x;
    return true;
}

MSFM_FHD double absd(double x) { return x < 0.0 ? -x : x; }

MSFM_FHD double clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

MSFM_FHD void cross3(const double a[3], const double b[3], double c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// the orthonormal frame (rows e[0..2], e[3..5], e[6..8]) of the triangle P1, P2, P3; false: no triangle
MSFM_FHD bool frame(const double P1[3], const double P2[3], const double P3[3], double e[9]) {
    const double d12[3] = {P2[0] - P1[0], P2[1] - P1[1], P2[2] - P1[2]}, d13[3] = {P3[0] - P1[0], P3[1] - P1[1], P3[2] - P1[2]};
    const double n12 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2], n13 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
    double w[3];
    cross3(d12, d13, w);
    const double nw = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (!(nw > kRegCollinear * n12 * n13)) return false;
    const double i1 = 1.0 / sqrt(n12), i3 = 1.0 / sqrt(nw);
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) {
        e[k] = d12[k] * i1;
        e[6 + k] = w[k] * i3;
    }
    cross3(e + 6, e, e + 3);
    return true;
}

// the pose of the depth ratios p = s2 / s1, q = s3 / s1 written at out[(12 ns + .) * S]; false: no pose (a depth that is not finite
// and > 0, no triangle, a non-finite pose)
template <int S>
MSFM_FHD bool p3p_pose(double p, double q, double b2, double cos_b, const double j[9], const double X[9], const double ew[9], double* out, int ns) {
    const double Dq = (q - 2.0 * cos_b) * q + 1.0;
    const double s1 = sqrt(b2 / Dq);
    const double s2 = p * s1, s3 = q * s1;
    if (!(q > 0.0 && p > 0.0 && s1 > 0.0 && msfm_pose::finite(s1) && msfm_pose::finite(s2) && msfm_pose::finite(s3))) return false;
    const double Y1[3] = {s1 * j[0], s1 * j[1], s1 * j[2]}, Y2[3] = {s2 * j[3], s2 * j[4], s2 * j[5]}, Y3[3] = {s3 * j[6], s3 * j[7], s3 * j[8]};
    double ec[9];
    if (!frame(Y1, Y2, Y3, ec)) return false;
    double R[9], t[3];
    bool ok = true;
MSFM_UNROLL
    for (int r = 0; r < 3; ++r)
MSFM_UNROLL
        for (int c = 0; c < 3; ++c) {
            R[3 * r + c] = ec[r] * ew[c] + ec[3 + r] * ew[3 + c] + ec[6 + r] * ew[6 + c];
            ok = ok && msfm_pose::finite(R[3 * r + c]);
        }
MSFM_UNROLL
    for (int r = 0; r < 3; ++r) {
        t[r] = Y1[r] - (R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2]);
        ok = ok && msfm_pose::finite(t[r]);
    }
    if (!ok) return false;
MSFM_UNROLL
    for (int e = 0; e < 9; ++e) out[(12 * ns + e) * S] = R[e];
MSFM_UNROLL
    for (int e = 0; e < 3; ++e) out[(12 * ns + 9 + e) * S] = t[e];
    return true;
}

// Grunert's P3P.  (u, v): the normalised observations, X: the points (3 x 3, row k = point k).  Writes up to 4 poses R[9] | t[3] at
// out[(12 s + q) * S] in ascending order of the root; returns their number.
template <int S>
MSFM_FHD int p3p(const double u[3], const double v[3], const double X[9], double* out) {
    double j[9];
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) {
        const double inv = 1.0 / sqrt(u[k] * u[k] + v[k] * v[k] + 1.0);
        j[3 * k] = u[k] * inv;
        j[3 * k + 1] = v[k] * inv;
        j[3 * k + 2] = inv;
    }
    const double cos_a = j[3] * j[6] + j[4] * j[7] + j[5] * j[8];
    const double cos_b = j[0] * j[6] + j[1] * j[7] + j[2] * j[8];
    const double cos_g = j[0] * j[3] + j[1] * j[4] + j[2] * j[5];
    double ew[9];
    if (!frame(X, X + 3, X + 6, ew)) return 0;
    double a2 = 0.0, b2 = 0.0, c2 = 0.0;
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) {
        a2 = a2 + (X[3 + k] - X[6 + k]) * (X[3 + k] - X[6 + k]);
        b2 = b2 + (X[k] - X[6 + k]) * (X[k] - X[6 + k]);
        c2 = c2 + (X[k] - X[3 + k]) * (X[k] - X[3 + k]);
    }
    const double A = a2 / b2, Cc = c2 / b2;
    // first quadratic  p^2 + p1(q) p + p0(q),  p1 = m1 q,  second  p^2 + q1 p + q0(q);  D(q) = 1 - 2 cos_b q + q^2
    const double m1 = -2.0 * cos_a, q1 = -2.0 * cos_g;
    const double p0[3] = {-A, 2.0 * A * cos_b, 1.0 - A};
    const double q0[3] = {1.0 - Cc, 2.0 * Cc * cos_b, -Cc};
    const double d[3] = {q0[0] - p0[0], q0[1] - p0[1], q0[2] - p0[2]};   // q0 - p0
    const double l[2] = {q1, -m1};                                        // q1 - p1
    // k = p1 q0 - p0 q1 (degree 3)
    const double kk[4] = {-p0[0] * q1, m1 * q0[0] - p0[1] * q1, m1 * q0[1] - p0[2] * q1, m1 * q0[2]};
    // g = d^2 - l k
    double g[5];
    g[0] = d[0] * d[0] - l[0] * kk[0];
    g[1] = 2.0 * d[0] * d[1] - (l[0] * kk[1] + l[1] * kk[0]);
    g[2] = (2.0 * d[0] * d[2] + d[1] * d[1]) - (l[0] * kk[2] + l[1] * kk[1]);
    g[3] = 2.0 * d[1] * d[2] - (l[0] * kk[3] + l[1] * kk[2]);
    g[4] = d[2] * d[2] - l[1] * kk[3];
    double big = 0.0;
MSFM_UNROLL
    for (int k = 0; k < 4; ++k) {
        double r = g[k] / g[4];
        r = r < 0.0 ? -r : r;
        big = r > big ? r : big;
    }
    const double B = 1.0 + big;
    if (!msfm_pose::finite(B)) return 0;   // (g4 = 0, a non-finite coefficient)
    const double g1[4] = {g[1], 2.0 * g[2], 3.0 * g[3], 4.0 * g[4]};
    const double g2[3] = {2.0 * g[2], 6.0 * g[3], 12.0 * g[4]};
    // the roots of g'' (none: both 0), clamped into [0, B], ascending
    double r1 = 0.0, r2 = 0.0;
    const double disc = g2[1] * g2[1] - 4.0 * g2[2] * g2[0];
    if (disc > 0.0) {
        const double sq = sqrt(disc);
        const double x1 = (-g2[1] - sq) / (2.0 * g2[2]), x2 = (-g2[1] + sq) / (2.0 * g2[2]);
        r1 = clamp(x1 < x2 ? x1 : x2, 0.0, B);
        r2 = clamp(x1 < x2 ? x2 : x1, 0.0, B);
    }
    // the critical points of g in [0, B]: an interval without one contributes its upper end (the break points stay ascending)
    double c0 = r1, c1 = r2, c2b = B, root = 0.0;
    if (bracket_root<3>(g1, 0.0, r1, &root)) c0 = root;
    if (bracket_root<3>(g1, r1, r2, &root)) c1 = root;
    if (bracket_root<3>(g1, r2, B, &root)) c2b = root;
    const double bp[5] = {0.0, c0, c1, c2b, B};
    // Coincident quadratics: at qs = -l0 / l1 the linear equation is 0 p = d(qs); where d(qs) and k(qs) vanish too (to kRegCoincide of
    // their terms' size) the two quadratics are THE SAME there, qs is a double root of g -- no sign change, or a pair of roots split
    // by rounding whose p is 0 / 0 -- and both roots p of the second quadratic are solutions (a triangle seen along its axis of
    // symmetry).  Then the roots of g within kRegCoincideRadius of qs are not used and those two poses come last.
    bool coincide = false;
    double qs = 0.0;
    if (l[1] != 0.0) {
        qs = -l[0] / l[1];
        const double ds = (d[2] * qs + d[1]) * qs + d[0], ks = ((kk[3] * qs + kk[2]) * qs + kk[1]) * qs + kk[0];
        const double sd = (absd(d[2]) * qs + absd(d[1])) * qs + absd(d[0]);
        const double sk = ((absd(kk[3]) * qs + absd(kk[2])) * qs + absd(kk[1])) * qs + absd(kk[0]);
        coincide = qs > 0.0 && msfm_pose::finite(qs) && sd > 0.0 && absd(ds) <= kRegCoincide * sd && absd(ks) <= kRegCoincide * sk;
    }
    int ns = 0;
MSFM_UNROLL
    for (int k = 0; k < 4; ++k) {
        double q = 0.0;
        if (!bracket_root<4>(g, bp[k], bp[k + 1], &q)) continue;
        if (coincide && absd(q - qs) <= kRegCoincideRadius * qs) continue;
        const double p = -((d[2] * q + d[1]) * q + d[0]) / (l[1] * q + l[0]);
        if (p3p_pose<S>(p, q, b2, cos_b, j, X, ew, out, ns)) ns += 1;
    }
    if (coincide) {
        const double q0s = (q0[2] * qs + q0[1]) * qs + q0[0];
        const double dp = q1 * q1 - 4.0 * q0s;
        if (dp >= 0.0) {
            const double sq = sqrt(dp);
            if (ns < 4 && p3p_pose<S>((-q1 - sq) / 2.0, qs, b2, cos_b, j, X, ew, out, ns)) ns += 1;
            if (sq > 0.0 && ns < 4 && p3p_pose<S>((-q1 + sq) / 2.0, qs, b2, cos_b, j, X, ew, out, ns)) ns += 1;
        }
    }
    return ns;
}

// the squared normalised error of one correspondence under (R, t); false: behind the camera (err2 is then not meaningful)
MSFM_FHD bool project_error(const double R[9], const double t[3], double u, double v, double X, double Y, double Z, double* err2) {
    const double P[3] = {X, Y, Z};
    double y[3];
    msfm_tri::transform(R, t, P, y);
    const double dx = y[0] / y[2] - u, dy = y[1] / y[2] - v;
    *err2 = dx * dx + dy * dy;
    return y[2] > msfm_pose::kDepthEps;
}

MSFM_FHD bool inlier(const double R[9], const double t[3], double u, double v, double X, double Y, double Z, double f2, double thr2) {
    double e2;
    const bool front = project_error(R, t, u, v, X, Y, Z, &e2);
    return front && e2 * f2 <= thr2;   // (false for a NaN)
}

MSFM_FHD double residual(const double R[9], const double t[3], double u, double v, double X, double Y, double Z, double f) {
    double e2;
    (void)project_error(R, t, u, v, X, Y, Z, &e2);
    return sqrt(e2) * f;
}

// ---- refinement -----------------------------------------------------------------------------------------------------------------
constexpr int kRegSums = 27;   // 21 of J^T J (upper triangle, row by row), then 6 of J^T r

// one inlier's terms added to a partial sum
MSFM_FHD void gn_add(const double R[9], const double t[3], double u, double v, double X, double Y, double Z, double acc[kRegSums]) {
    const double P[3] = {X, Y, Z};
    double Yv[3];
    msfm_tri::transform(R, t, P, Yv);
    const double iz = 1.0 / Yv[2], px = Yv[0] * iz, py = Yv[1] * iz;
    const double rx = px - u, ry = py - v;
    // d(pi)/dY = [iz 0 -px iz; 0 iz -py iz];  dY/da = -2 [Y]x,  dY/d(dt) = I
    const double a0[3] = {iz, 0.0, -px * iz}, a1[3] = {0.0, iz, -py * iz};
    double J0[6], J1[6];
    // (row) . (-2 [Y]x):  columns  -2 (row x ... ) = 2 (Y x row)^T ... written out: row . (a x Y) = a . (Y x row)
    double w0[3], w1[3];
    cross3(Yv, a0, w0);
    cross3(Yv, a1, w1);
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) {
        J0[k] = 2.0 * w0[k];
        J1[k] = 2.0 * w1[k];
        J0[3 + k] = a0[k];
        J1[3 + k] = a1[k];
    }
    int at = 0;
MSFM_UNROLL
    for (int r = 0; r < 6; ++r)
MSFM_UNROLL
        for (int c = r; c < 6; ++c) {
            acc[at] = acc[at] + (J0[r] * J0[c] + J1[r] * J1[c]);
            ++at;
        }
MSFM_UNROLL
    for (int r = 0; r < 6; ++r) acc[21 + r] = acc[21 + r] + (J0[r] * rx + J1[r] * ry);
}

// A x = -g by a 6 x 6 Cholesky: L holds the lower triangle of A (L[r][c], c <= r) and is overwritten by its factor; then L y = -g,
// L^T x = y.  False: a pivot is not > 0 or x is not finite.
MSFM_FHD bool cholesky6_solve(double L[6][6], const double g[6], double x[6]) {
MSFM_UNROLL
    for (int k = 0; k < 6; ++k) {
        double dd = L[k][k];
MSFM_UNROLL
        for (int m = 0; m < k; ++m) dd = dd - L[k][m] * L[k][m];
        if (!(dd > 0.0)) return false;
        dd = sqrt(dd);
        L[k][k] = dd;
MSFM_UNROLL
        for (int r = k + 1; r < 6; ++r) {
            double s = L[r][k];
MSFM_UNROLL
            for (int m = 0; m < k; ++m) s = s - L[r][m] * L[k][m];
            L[r][k] = s / dd;
        }
    }
MSFM_UNROLL
    for (int k = 0; k < 6; ++k) {   // L y = -g
        double s = -g[k];
MSFM_UNROLL
        for (int m = 0; m < k; ++m) s = s - L[k][m] * x[m];
        x[k] = s / L[k][k];
    }
MSFM_UNROLL
    for (int k = 5; k >= 0; --k) {   // L^T x = y
        double s = x[k];
MSFM_UNROLL
        for (int m = k + 1; m < 6; ++m) s = s - L[m][k] * x[m];
        x[k] = s / L[k][k];
    }
    bool ok = true;
MSFM_UNROLL
    for (int k = 0; k < 6; ++k) ok = ok && msfm_pose::finite(x[k]);
    return ok;
}

// the step x = (a, dt) applied to (R, t):  Rn = C(a) R,  tn = C(a) t + dt  with Cayley's C.  False: the new pose is not finite.
MSFM_FHD bool cayley_update(const double x[6], const double R[9], const double t[3], double Rn[9], double tn[3]) {
    const double a0 = x[0], a1 = x[1], a2 = x[2];
    const double aa = a0 * a0 + a1 * a1 + a2 * a2, inv = 1.0 / (1.0 + aa), dg = 1.0 - aa;
    const double C[9] = {(dg + 2.0 * a0 * a0) * inv,       (2.0 * a0 * a1 - 2.0 * a2) * inv, (2.0 * a0 * a2 + 2.0 * a1) * inv,
                         (2.0 * a0 * a1 + 2.0 * a2) * inv, (dg + 2.0 * a1 * a1) * inv,       (2.0 * a1 * a2 - 2.0 * a0) * inv,
                         (2.0 * a0 * a2 - 2.0 * a1) * inv, (2.0 * a1 * a2 + 2.0 * a0) * inv, (dg + 2.0 * a2 * a2) * inv};
    bool ok = true;
MSFM_UNROLL
    for (int r = 0; r < 3; ++r) {
MSFM_UNROLL
        for (int c = 0; c < 3; ++c) {
            Rn[3 * r + c] = C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c] + C[3 * r + 2] * R[6 + c];
            ok = ok && msfm_pose::finite(Rn[3 * r + c]);
        }
        tn[r] = (C[3 * r] * t[0] + C[3 * r + 1] * t[1] + C[3 * r + 2] * t[2]) + x[3 + r];
        ok = ok && msfm_pose::finite(tn[r]);
    }
    return ok;
}

// the step from the 27 sums (H x = -g, H as summed: undamped), applied to (R, t) in place; false: no step (R, t unchanged)
MSFM_FHD bool gn_step(const double acc[kRegSums], double R[9], double t[3]) {
    double L[6][6], x[6];
    int at = 0;
MSFM_UNROLL
    for (int r = 0; r < 6; ++r)
MSFM_UNROLL
        for (int c = r; c < 6; ++c) L[c][r] = acc[at++];   // lower triangle
    double Rn[9], tn[3];
    if (!cholesky6_solve(L, acc + 21, x) || !cayley_update(x, R, t, Rn, tn)) return false;
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) R[k] = Rn[k];
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) t[k] = tn[k];
    return true;
}

// the rounds of kRegRound hypotheses the stopping rule needs before it is decided (>= 1), its winner and the winner's count
template <typename CountFn>
MSFM_FHD int rounds_needed(int n, int max_iters, double confidence, CountFn count_at, int* best_it, int* best_count) {
    for (int r = 1;; ++r) {
        const int avail = r * kRegRound < max_iters ? r * kRegRound : max_iters;
        bool decided = false;
        *best_it = msfm_fmat::replay_adaptive<3>(n, max_iters, confidence, count_at, best_count, avail, &decided);
        if (decided) return r;
    }
}

MSFM_FHD void clear_record(msfm_registration* r, int image_id, int n) {
    r->image_id = image_id;
    r->status = 0;
    r->n_correspondences = n;
    r->n_inliers = 0;
    r->hypotheses = 0;
    r->reserved = 0;
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) r->R[k] = 0.0;
    r->t[0] = r->t[1] = r->t[2] = 0.0;
    r->mean_residual = 0.0;
}

MSFM_FHD bool attempted(int n, int min_inliers) { return n >= 3 && n >= min_inliers; }

#if !defined(__HIPCC__)
// ---- the host twin ----------------------------------------------------------------------------------------------------------------
// hypothesis `it` of an image: its poses (S = 1) and its count; returns the number of poses, *best: the pose that counts
inline int host_hypothesis(const double* cu, const double* cv, const double* cX, const double* cY, const double* cZ, int n,
                           unsigned long long seed, int it, double f2, double thr2, double poses[48], int* count, int* best) {
    int idx[3];
    sample3(seed, it, n, idx);
    double u[3], v[3], X[9];
    for (int k = 0; k < 3; ++k) {
        u[k] = cu[idx[k]];
        v[k] = cv[idx[k]];
        X[3 * k] = cX[idx[k]];
        X[3 * k + 1] = cY[idx[k]];
        X[3 * k + 2] = cZ[idx[k]];
    }
    const int ns = p3p<1>(u, v, X, poses);
    *count = 0;
    *best = 0;
    for (int s = 0; s < ns; ++s) {
        int c = 0;
        for (int i = 0; i < n; ++i) c += inlier(poses + 12 * s, poses + 12 * s + 9, cu[i], cv[i], cX[i], cY[i], cZ[i], f2, thr2) ? 1 : 0;
        if (c > *count) {
            *count = c;
            *best = s;
        }
    }
    return ns;
}

// the 27 sums over the inlier list (list == nullptr: positions are indices) in the defined order: 64 partials, then the butterfly
inline void partial_sums(const double R[9], const double t[3], const double* cu, const double* cv, const double* cX, const double* cY,
                         const double* cZ, const int* list, int ni, double part[kRegRound][kRegSums]) {
    for (int j = 0; j < kRegRound; ++j) {
        for (int k = 0; k < kRegSums; ++k) part[j][k] = 0.0;
        for (int pos = j; pos < ni; pos += kRegRound) {
            const int i = list ? list[pos] : pos;
            gn_add(R, t, cu[i], cv[i], cX[i], cY[i], cZ[i], part[j]);
        }
    }
    for (int s = kRegRound / 2; s >= 1; s >>= 1) {
        double nxt[kRegRound][kRegSums];
        for (int j = 0; j < kRegRound; ++j)
            for (int k = 0; k < kRegSums; ++k) nxt[j][k] = part[j][k] + part[j ^ s][k];
        for (int j = 0; j < kRegRound; ++j)
            for (int k = 0; k < kRegSums; ++k) part[j][k] = nxt[j][k];
    }
}

// one image from its n correspondences (cu, cv, cX, cY, cZ in correspondence order): the record, the flags and the residuals
inline void RegisterImage(int image_id, const double* cu, const double* cv, const double* cX, const double* cY, const double* cZ, int n,
                          const msfm_emat::Camera& cam, const Params& prm, msfm_registration* rec, uint8_t* flags, double* residuals) {
    clear_record(rec, image_id, n);
    for (int i = 0; i < n; ++i) {
        flags[i] = 0;
        residuals[i] = -1.0;
    }
    if (!attempted(n, prm.min_inliers)) return;
    rec->status = MSFM_REG_ATTEMPTED;
    const double f = (cam.fx + cam.fy) / 2.0, f2 = f * f, thr2 = prm.max_error * prm.max_error;
    const unsigned long long seed = reg_seed(image_id);
    std::vector<int> counts((size_t)prm.max_iters, -1);
    double poses[48];
    auto count_at = [&](int it) {
        if (counts[(size_t)it] < 0) {
            int c, b;
            host_hypothesis(cu, cv, cX, cY, cZ, n, seed, it, f2, thr2, poses, &c, &b);
            counts[(size_t)it] = c;
        }
        return counts[(size_t)it];
    };
    int best_it = -1, best_count = 0;
    const int rounds = rounds_needed(n, prm.max_iters, prm.confidence, count_at, &best_it, &best_count);
    rec->hypotheses = rounds * kRegRound < prm.max_iters ? rounds * kRegRound : prm.max_iters;
    if (best_it < 0) return;
    int c, b;
    host_hypothesis(cu, cv, cX, cY, cZ, n, seed, best_it, f2, thr2, poses, &c, &b);
    double R[9], t[3];
    for (int k = 0; k < 9; ++k) R[k] = poses[12 * b + k];
    for (int k = 0; k < 3; ++k) t[k] = poses[12 * b + 9 + k];
    std::vector<int> list;
    for (int i = 0; i < n; ++i)
        if (inlier(R, t, cu[i], cv[i], cX[i], cY[i], cZ[i], f2, thr2)) list.push_back(i);
    int status = MSFM_REG_ATTEMPTED | MSFM_REG_POSE;
    if (prm.refine_iters > 0) {
        double Rr[9], tr[3];
        for (int k = 0; k < 9; ++k) Rr[k] = R[k];
        for (int k = 0; k < 3; ++k) tr[k] = t[k];
        const int ni = (int)list.size();
        for (int step = 0; step < prm.refine_iters; ++step) {
            double part[kRegRound][kRegSums];
            partial_sums(Rr, tr, cu, cv, cX, cY, cZ, list.data(), ni, part);
            if (!gn_step(part[0], Rr, tr)) break;
        }
        int cr = 0;
        for (int i = 0; i < n; ++i) cr += inlier(Rr, tr, cu[i], cv[i], cX[i], cY[i], cZ[i], f2, thr2) ? 1 : 0;
        if (cr >= ni) {
            for (int k = 0; k < 9; ++k) R[k] = Rr[k];
            for (int k = 0; k < 3; ++k) t[k] = tr[k];
            status |= MSFM_REG_REFINED;
        }
    }
    int ni = 0;
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const bool in = inlier(R, t, cu[i], cv[i], cX[i], cY[i], cZ[i], f2, thr2);
        const double e = residual(R, t, cu[i], cv[i], cX[i], cY[i], cZ[i], f);
        flags[i] = in ? 1 : 0;
        residuals[i] = msfm_pose::canonical(e);
        if (in) {
            ni += 1;
            sum = sum + e;
        }
    }
    if (ni >= prm.min_inliers) status |= MSFM_REG_SUCCEEDED;
    rec->status = status;
    rec->n_inliers = ni;
    for (int k = 0; k < 9; ++k) rec->R[k] = R[k];
    for (int k = 0; k < 3; ++k) rec->t[k] = t[k];
    rec->mean_residual = ni > 0 ? sum / (double)ni : 0.0;
}

// ---- RegisterImages over a finished, triangulated track result ---------------------------------------------------------------------
// tracks as msfm_fetch_tracks returns them, points as msfm_fetch_points3d; pos_of_id: per image id the position in the list or -1.
inline bool usable(const msfm_point3d& p) {
    const int want = MSFM_TRI_POINT | MSFM_TRI_ERROR_OK | MSFM_TRI_ANGLE_OK;
    return (p.status & want) == want;
}

// the number of correspondences of every listed image
inline void CountCorrespondences(const int64_t* offsets, const int32_t* image_ids, int64_t n_tracks, const msfm_point3d* points,
                                 const int* pos_of_id, int n_list, int64_t* counts) {
    for (int k = 0; k < n_list; ++k) counts[k] = 0;
    std::vector<int64_t> seen((size_t)std::max(n_list, 1), -1);   // (a triangulated track is consistent: the guard never fires there)
    for (int64_t t = 0; t < n_tracks; ++t) {
        if (!usable(points[t])) continue;
        for (int64_t e = offsets[t]; e < offsets[t + 1]; ++e) {
            const int k = pos_of_id[image_ids[e]];
            if (k < 0 || seen[(size_t)k] == t) continue;
            seen[(size_t)k] = t;
            counts[k] += 1;
        }
    }
}

// the images [first, first + count) of the list; out_offsets (n_list + 1, from CountCorrespondences) says where each image's
// correspondences go in out_tid / out_flags / out_residuals.  kxy[k]: the (x, y) fp32 pairs of the image at list position k.
inline void RegisterImages(const int64_t* offsets, const int32_t* image_ids, const int32_t* point_idx, int64_t n_tracks,
                           const msfm_point3d* points, const int32_t* list_ids, const int* pos_of_id, const float* const* kxy,
                           const msfm_emat::Camera& cam, const Params& prm, const int64_t* out_offsets, int first, int count,
                           msfm_registration* records, int32_t* out_tid, uint8_t* out_flags, double* out_residuals) {
    if (count <= 0) return;
    const int64_t base = out_offsets[first], total = out_offsets[first + count] - base;
    std::vector<double> cu((size_t)total), cv((size_t)total), cX((size_t)total), cY((size_t)total), cZ((size_t)total);
    std::vector<int64_t> fill((size_t)count, 0), seen((size_t)count, -1);
    for (int64_t t = 0; t < n_tracks; ++t) {
        if (!usable(points[t])) continue;
        for (int64_t e = offsets[t]; e < offsets[t + 1]; ++e) {
            const int k = pos_of_id[image_ids[e]] - first;
            if (k < 0 || k >= count || seen[(size_t)k] == t) continue;
            seen[(size_t)k] = t;
            const int64_t at = out_offsets[first + k] - base + fill[(size_t)k]++;
            const float* q = kxy[first + k] + 2 * (size_t)point_idx[e];
            msfm_emat::undistort(cam, (double)q[0], (double)q[1], &cu[(size_t)at], &cv[(size_t)at]);
            cX[(size_t)at] = points[t].X[0];
            cY[(size_t)at] = points[t].X[1];
            cZ[(size_t)at] = points[t].X[2];
            out_tid[base + at] = (int32_t)t;
        }
    }
    for (int k = 0; k < count; ++k) {
        const int64_t o = out_offsets[first + k] - base;
        RegisterImage(list_ids[first + k], cu.data() + o, cv.data() + o, cX.data() + o, cY.data() + o, cZ.data() + o,
                      (int)(out_offsets[first + k + 1] - out_offsets[first + k]), cam, prm, records + first + k, out_flags + base + o,
                      out_residuals + base + o);
    }
}
#endif

}  // namespace msfm_reg
