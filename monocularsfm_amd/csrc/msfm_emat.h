// msfm_emat.h -- essential-matrix arithmetic shared by the device kernels (msfm_verify_e.hip.h, hipcc) and the host twin
// (host/GeometricVerification.cpp, g++): the calibrated geometric verification (msfm_set_verification_model(.., 1, camera)),
// the check the reference leaves as a TODO next to its F-only verification (src/Feature/FeatureMatching.cpp:59) and runs
// itself later with cv::findEssentialMat on the same camera (src/Reconstruction/Initializer.cpp:310).
//
// The contract of msfm_fmat.h holds here too: fp64 with +, -, *, /, sqrt only (and det_log), static loop structure,
// -ffp-contract=off on both sides -> the host twin and the device produce the SAME bits.
//
//   normalised coordinates  ((u - cx) / fx, (v - cy) / fy), then the Brown model (k1, k2, p1, p2) inverted by
//                           kUndistortIters fixed-point iterations of the undistortPoints kind (skipped when all four are 0:
//                           exact).  tests/test_emat_reference.py checks <= 1e-12 relative against a Newton solve to 1e-15
//                           up to the image corners for |k1| <= 0.2, |k2| <= 0.05, |p| <= 2e-3.
//   sample                  5 distinct indices from the counter-based stream of sample8 (sample5).
//   minimal solver          Nister's 5-point: null space of the 5 x 9 constraints (Householder QR of A^T), the 10 cubic
//                           constraints det E = 0 and 2 E E^T E - tr(E E^T) E = 0 by polynomial arithmetic, Gauss-Jordan with
//                           partial pivoting on the 10 x 20 system, the degree-10 polynomial det B(z), its real roots by
//                           Sturm-sequence counting + bisection (kSturmSteps per root) + kNewtonSteps Newton steps inside the
//                           bracket; x, y from the null vector of B(z); kPolishSteps Gauss-Newton steps of (x, y, z) on the
//                           cubic constraints; up to 10 E of unit Frobenius norm.
//   error                   Sampson error in normalised coordinates, inlier when <= (threshold / ((fx + fy) / 2))^2.
//   stopping rule           msfm_fmat::replay_adaptive<5>.
//
// The solver's work arrays live in a per-hypothesis workspace of kWork doubles addressed with a compile-time stride S:
// S = 1 on the host, S = the workgroup size on the device, where the workspace is in LDS (one hypothesis per lane, lane-
// interleaved so that the lanes of a wave touch consecutive 8-byte words).  Runtime-indexed arrays therefore never land in
// scratch memory, and the arithmetic -- hence the bits -- does not depend on S.
#pragma once

#include "msfm_fmat.h"

namespace msfm_emat {

using msfm_fmat::mix64;

constexpr int kUndistortIters = 40;   // fixed-point iterations of the Brown-model inversion
constexpr int kSturmSteps = 64;       // count-bisection steps per real root (then Newton inside what is left of the bracket)
constexpr int kNewtonSteps = 4;       // Newton steps inside the final bracket
constexpr int kPolishSteps = 3;      // Gauss-Newton steps of each solution on the cubic constraints
constexpr int kMaxSolutions = 10;

// workspace layout (doubles, each multiplied by the stride S)
constexpr int kWsNull = 0;       // 4 x 9 null basis X, Y, Z, W (orthonormal)
constexpr int kWsG = 36;         // 10 x 20 cubic constraints (Householder scratch before, solutions after)
constexpr int kWsQ = 236;        // 6 x 10 quadratic entries of E E^T (then the 3 x 13 coefficients of B(z))
constexpr int kWork = 296;
constexpr int kWsSol = kWsG;         // 10 x 9 solutions (the G rows are dead by then)
constexpr int kWsRoots = kWsSol + 90; // 10 roots

struct Camera {
    double fx, fy, cx, cy, k1, k2, p1, p2;
};

// pixel -> normalised, undistorted camera coordinates
MSFM_FHD void undistort(const Camera& c, double u, double v, double* xo, double* yo) {
    const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
    double x = x0, y = y0;
    if (c.k1 != 0.0 || c.k2 != 0.0 || c.p1 != 0.0 || c.p2 != 0.0) {
        for (int k = 0; k < kUndistortIters; ++k) {
            const double r2 = x * x + y * y;
            const double icdist = 1.0 / (1.0 + (c.k2 * r2 + c.k1) * r2);
            const double dx = 2.0 * c.p1 * x * y + c.p2 * (r2 + 2.0 * x * x);
            const double dy = c.p1 * (r2 + 2.0 * y * y) + 2.0 * c.p2 * x * y;
            x = (x0 - dx) * icdist;
            y = (y0 - dy) * icdist;
        }
    }
    *xo = x;
    *yo = y;
}

// the 5 distinct match indices of hypothesis `it` (n >= 5): sample8's stream, k < 5
MSFM_FHD void sample5(unsigned long long seed, int it, int n, int idx[5]) {
MSFM_UNROLL
    for (int k = 0; k < 5; ++k) idx[k] = -1;
MSFM_UNROLL
    for (int k = 0; k < 5; ++k) {
        int c = 0;
        for (int attempt = 0;; ++attempt) {
            c = attempt < 32 ? (int)(mix64(seed ^ mix64(((unsigned long long)it << 20) ^ ((unsigned long long)k << 8) ^ (unsigned long long)attempt)) % (unsigned long long)n)
                             : (c + 1) % n;  // linear probe: terminates because n >= 5
            bool dup = false;
MSFM_UNROLL
            for (int j = 0; j < 5; ++j) dup |= (idx[j] == c);
            if (!dup) break;
        }
        idx[k] = c;
    }
}

// Sampson error of (x1, y1) <-> (x2, y2) under E (row-major, x2^T E x1 = 0)
MSFM_FHD double sampson(const double E[9], double x1, double y1, double x2, double y2) {
    const double a0 = E[0] * x1 + E[1] * y1 + E[2], a1 = E[3] * x1 + E[4] * y1 + E[5], a2 = E[6] * x1 + E[7] * y1 + E[8];
    const double b0 = E[0] * x2 + E[3] * y2 + E[6], b1 = E[1] * x2 + E[4] * y2 + E[7];
    const double num = x2 * a0 + y2 * a1 + a2;
    return num * num / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);  // 0 / 0 = NaN fails the <= test
}

// ---- polynomials in (x, y, z).  Quadratic monomials: x2 xy xz y2 yz z2 x y z 1.  Cubic monomials in Nister's order:
// x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1 -- the first ten are eliminated by the Gauss-Jordan step.
// quadratic monomial i times linear monomial j (x y z 1) -> cubic monomial index (a literal table: on the device every use is
// in an unrolled loop, so it folds to constants; tests/test_emat_reference.py checks the constraints it builds)
constexpr int kQC[10][4] = {{0, 2, 4, 5}, {2, 3, 8, 9}, {4, 8, 10, 11}, {3, 1, 6, 7}, {8, 6, 13, 14}, {10, 13, 16, 17}, {5, 9, 11, 12}, {9, 7, 14, 15}, {11, 14, 17, 18}, {12, 15, 18, 19}};

// linear entry k of E = x X + y Y + z Z + W as (x, y, z, 1) coefficients
template <int S>
MSFM_FHD void lin(const double* ws, int k, double a[4]) {
MSFM_UNROLL
    for (int j = 0; j < 4; ++j) a[j] = ws[(kWsNull + 9 * j + k) * S];
}
// product of two linear polynomials
MSFM_FHD void lin_mul(const double a[4], const double b[4], double q[10]) {
    q[0] = a[0] * b[0];
    q[1] = a[0] * b[1] + a[1] * b[0];
    q[2] = a[0] * b[2] + a[2] * b[0];
    q[3] = a[1] * b[1];
    q[4] = a[1] * b[2] + a[2] * b[1];
    q[5] = a[2] * b[2];
    q[6] = a[0] * b[3] + a[3] * b[0];
    q[7] = a[1] * b[3] + a[3] * b[1];
    q[8] = a[2] * b[3] + a[3] * b[2];
    q[9] = a[3] * b[3];
}
// cubic row r of G += s * (quadratic q) * (linear a)
template <int S>
MSFM_FHD void qa_add(double* ws, int r, double s, const double q[10], const double a[4]) {
MSFM_UNROLL
    for (int i = 0; i < 10; ++i)
MSFM_UNROLL
        for (int j = 0; j < 4; ++j) {
            double& g = ws[(kWsG + 20 * r + kQC[i][j]) * S];
            g = g + s * (q[i] * a[j]);
        }
}

// ascending-power polynomial product c[0 .. na + nb - 2] = a[0 .. na - 1] * b[0 .. nb - 1]
template <int NA, int NB>
MSFM_FHD void pmul(const double* a, const double* b, double* c) {
MSFM_UNROLL
    for (int k = 0; k < NA + NB - 1; ++k) c[k] = 0.0;
MSFM_UNROLL
    for (int i = 0; i < NA; ++i)
MSFM_UNROLL
        for (int j = 0; j < NB; ++j) c[i + j] = c[i + j] + a[i] * b[j];
}

// Sturm chain st (degrees 10 .. 0, ascending coefficients, 66 in all) evaluated at t: number of sign changes (zeros skipped).
// Unrolled, so the chain stays in registers on the device: it is read 11 times per bisection step.
MSFM_FHD int sturm_changes(const double st[66], double t) {
    int changes = 0, prev = 0, off = 0;
MSFM_UNROLL
    for (int d = 10; d >= 0; --d) {
        double v = st[off + d];
MSFM_UNROLL
        for (int i = d - 1; i >= 0; --i) v = v * t + st[off + i];
        const int sg = v > 0.0 ? 1 : (v < 0.0 ? -1 : 0);
        if (sg != 0) {
            if (prev != 0 && sg != prev) ++changes;
            prev = sg;
        }
        off += d + 1;
    }
    return changes;
}

// kPolishSteps Gauss-Newton steps of (x, y, z) on the 10 cubic constraints themselves, evaluated from E = x X + y Y + z Z + W
// (the degree-10 polynomial is worse conditioned than the system it comes from: a root exact to the last bit of the polynomial
// can be 1e-8 away from the system's); a step is taken only when it is small, so a solution never jumps to another one.
template <int S>
MSFM_FHD void gauss_newton(const double* ws, double& x, double& y, double& z) {
    for (int step = 0; step < kPolishSteps; ++step) {
        double E[9], D[3][9];
MSFM_UNROLL
        for (int k = 0; k < 9; ++k) {
            D[0][k] = ws[(kWsNull + k) * S];
            D[1][k] = ws[(kWsNull + 9 + k) * S];
            D[2][k] = ws[(kWsNull + 18 + k) * S];
            E[k] = x * D[0][k] + y * D[1][k] + z * D[2][k] + ws[(kWsNull + 27 + k) * S];
        }
        double EEt[9], EtE[9], tr = 0.0;
MSFM_UNROLL
        for (int i = 0; i < 3; ++i)
MSFM_UNROLL
            for (int j = 0; j < 3; ++j) {
                EEt[3 * i + j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
                EtE[3 * i + j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
            }
        tr = EEt[0] + EEt[4] + EEt[8];
        const double cof[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                               E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                               E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
        double r[10], J[10][3];
        r[0] = E[0] * cof[0] + E[1] * cof[1] + E[2] * cof[2];
MSFM_UNROLL
        for (int i = 0; i < 3; ++i)
MSFM_UNROLL
            for (int j = 0; j < 3; ++j)
                r[1 + 3 * i + j] = 2.0 * (EEt[3 * i] * E[j] + EEt[3 * i + 1] * E[3 + j] + EEt[3 * i + 2] * E[6 + j]) - tr * E[3 * i + j];
MSFM_UNROLL
        for (int v = 0; v < 3; ++v) {
            const double* Dv = D[v];
            double dd = 0.0, ed = 0.0;
MSFM_UNROLL
            for (int k = 0; k < 9; ++k) {
                dd += cof[k] * Dv[k];
                ed += E[k] * Dv[k];
            }
            J[0][v] = dd;
            // d(E E^T E) = D E^T E + E D^T E + E E^T D;  d tr(E E^T) = 2 <E, D>
            double EDt[9];
MSFM_UNROLL
            for (int i = 0; i < 3; ++i)
MSFM_UNROLL
                for (int j = 0; j < 3; ++j) EDt[3 * i + j] = E[3 * i] * Dv[3 * j] + E[3 * i + 1] * Dv[3 * j + 1] + E[3 * i + 2] * Dv[3 * j + 2];
MSFM_UNROLL
            for (int i = 0; i < 3; ++i)
MSFM_UNROLL
                for (int j = 0; j < 3; ++j) {
                    const double a = Dv[3 * i] * EtE[j] + Dv[3 * i + 1] * EtE[3 + j] + Dv[3 * i + 2] * EtE[6 + j];
                    const double b = EDt[3 * i] * E[j] + EDt[3 * i + 1] * E[3 + j] + EDt[3 * i + 2] * E[6 + j];
                    const double c = EEt[3 * i] * Dv[j] + EEt[3 * i + 1] * Dv[3 + j] + EEt[3 * i + 2] * Dv[6 + j];
                    J[1 + 3 * i + j][v] = 2.0 * (a + b + c) - 2.0 * ed * E[3 * i + j] - tr * Dv[3 * i + j];
                }
        }
        double A[3][3], g[3];
MSFM_UNROLL
        for (int a = 0; a < 3; ++a) {
            g[a] = 0.0;
MSFM_UNROLL
            for (int b = 0; b < 3; ++b) A[a][b] = 0.0;
        }
MSFM_UNROLL
        for (int k = 0; k < 10; ++k)
MSFM_UNROLL
            for (int a = 0; a < 3; ++a) {
                g[a] += J[k][a] * r[k];
MSFM_UNROLL
                for (int b = 0; b < 3; ++b) A[a][b] += J[k][a] * J[k][b];
            }
        const double c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2],
                     c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0];
        const double det = A[0][0] * c00 + A[0][1] * c01 + A[0][2] * c02;
        if (!(det > 0.0 || det < 0.0)) return;
        const double d0 = (g[0] * c00 + g[1] * (A[0][2] * A[2][1] - A[0][1] * A[2][2]) + g[2] * (A[0][1] * A[1][2] - A[0][2] * A[1][1])) / det;
        const double d1 = (g[0] * c01 + g[1] * (A[0][0] * A[2][2] - A[0][2] * A[2][0]) + g[2] * (A[0][2] * A[1][0] - A[0][0] * A[1][2])) / det;
        const double d2 = (g[0] * c02 + g[1] * (A[0][1] * A[2][0] - A[0][0] * A[2][1]) + g[2] * (A[0][0] * A[1][1] - A[0][1] * A[1][0])) / det;
        const double size = (x >= 0.0 ? x : -x) + (y >= 0.0 ? y : -y) + (z >= 0.0 ? z : -z) + 1.0;
        const double step_size = (d0 >= 0.0 ? d0 : -d0) + (d1 >= 0.0 ? d1 : -d1) + (d2 >= 0.0 ? d2 : -d2);
        if (!(step_size <= 1e-2 * size)) return;
        x -= d0;
        y -= d1;
        z -= d2;
    }
}

// Five-point solver: the up-to-10 essential matrices (unit Frobenius norm, row-major) of the 5 correspondences
// (x1[i], y1[i]) <-> (x2[i], y2[i]) in normalised coordinates; they are left at ws[(kWsSol + 9 s + k) * S].  Returns the count.
template <int S>
MSFM_FHD int five_point(const double x1[5], const double y1[5], const double x2[5], const double y2[5], double* ws) {
    // --- null space: Householder QR of A^T (9 x 5, column j = constraint j), kept in G as H[r + 9 j]; betas after it
    double* H = ws + kWsG * S;
MSFM_UNROLL
    for (int j = 0; j < 5; ++j) {
        const double r[9] = {x2[j] * x1[j], x2[j] * y1[j], x2[j], y2[j] * x1[j], y2[j] * y1[j], y2[j], x1[j], y1[j], 1.0};
MSFM_UNROLL
        for (int i = 0; i < 9; ++i) H[(i + 9 * j) * S] = r[i];
    }
    for (int j = 0; j < 5; ++j) {
        double nn = 0.0;
        for (int i = j; i < 9; ++i) nn += H[(i + 9 * j) * S] * H[(i + 9 * j) * S];
        const double a0 = H[(j + 9 * j) * S];
        const double nrm = sqrt(nn);
        const double alpha = a0 >= 0.0 ? -nrm : nrm;
        const double v0 = a0 - alpha;
        const double vv = nn - a0 * a0 + v0 * v0;
        const double beta = vv > 0.0 ? 2.0 / vv : 0.0;
        H[(j + 9 * j) * S] = v0;
        H[(45 + j) * S] = beta;
        for (int c = j + 1; c < 5; ++c) {
            double d = 0.0;
            for (int i = j; i < 9; ++i) d += H[(i + 9 * j) * S] * H[(i + 9 * c) * S];
            d *= beta;
            for (int i = j; i < 9; ++i) H[(i + 9 * c) * S] -= d * H[(i + 9 * j) * S];
        }
    }
    // Q e_{5+f} = H_0 H_1 .. H_4 e_{5+f}
    for (int f = 0; f < 4; ++f) {
        double v[9];
MSFM_UNROLL
        for (int i = 0; i < 9; ++i) v[i] = (i == 5 + f) ? 1.0 : 0.0;
        for (int j = 4; j >= 0; --j) {
            double d = 0.0;
MSFM_UNROLL
            for (int i = 0; i < 9; ++i)
                if (i >= j) d += H[(i + 9 * j) * S] * v[i];
            d *= H[(45 + j) * S];
MSFM_UNROLL
            for (int i = 0; i < 9; ++i)
                if (i >= j) v[i] -= d * H[(i + 9 * j) * S];
        }
MSFM_UNROLL
        for (int i = 0; i < 9; ++i) ws[(kWsNull + 9 * f + i) * S] = v[i];
    }
    // --- the 10 cubic constraints
    for (int k = 0; k < 200; ++k) ws[(kWsG + k) * S] = 0.0;
    {   // det E by the first row: E0 (E4 E8 - E5 E7) - E1 (E3 E8 - E5 E6) + E2 (E3 E7 - E4 E6)
        double a[4], b[4], q[10], t[10];
        const int mi[3][4] = {{4, 8, 5, 7}, {3, 8, 5, 6}, {3, 7, 4, 6}};
MSFM_UNROLL
        for (int c = 0; c < 3; ++c) {
            lin<S>(ws, mi[c][0], a);
            lin<S>(ws, mi[c][1], b);
            lin_mul(a, b, q);
            lin<S>(ws, mi[c][2], a);
            lin<S>(ws, mi[c][3], b);
            lin_mul(a, b, t);
MSFM_UNROLL
            for (int i = 0; i < 10; ++i) q[i] = q[i] - t[i];
            lin<S>(ws, c, a);
            qa_add<S>(ws, 0, c == 1 ? -1.0 : 1.0, q, a);
        }
    }
    // E E^T (symmetric; entries (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) at Q + 10 s)
    {
        const int sr[6] = {0, 0, 0, 1, 1, 2}, sc[6] = {0, 1, 2, 1, 2, 2};
MSFM_UNROLL
        for (int s = 0; s < 6; ++s) {
            double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
MSFM_UNROLL
            for (int k = 0; k < 3; ++k) {
                double a[4], b[4], q[10];
                lin<S>(ws, 3 * sr[s] + k, a);
                lin<S>(ws, 3 * sc[s] + k, b);
                lin_mul(a, b, q);
MSFM_UNROLL
                for (int i = 0; i < 10; ++i) acc[i] = acc[i] + q[i];
            }
MSFM_UNROLL
            for (int i = 0; i < 10; ++i) ws[(kWsQ + 10 * s + i) * S] = acc[i];
        }
    }
    // (E E^T - tr(E E^T) / 2 I) E: rows 1 .. 9 (entry (i, j) -> row 1 + 3 i + j)
    {
        double half_tr[10];
MSFM_UNROLL
        for (int m = 0; m < 10; ++m) half_tr[m] = 0.5 * (ws[(kWsQ + m) * S] + ws[(kWsQ + 30 + m) * S] + ws[(kWsQ + 50 + m) * S]);
        const int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
MSFM_UNROLL
        for (int i = 0; i < 3; ++i)
MSFM_UNROLL
            for (int j = 0; j < 3; ++j)
MSFM_UNROLL
                for (int k = 0; k < 3; ++k) {
                    double q[10], a[4];
MSFM_UNROLL
                    for (int m = 0; m < 10; ++m) q[m] = ws[(kWsQ + 10 * sym[i][k] + m) * S] - (i == k ? half_tr[m] : 0.0);
                    lin<S>(ws, 3 * k + j, a);
                    qa_add<S>(ws, 1 + 3 * i + j, 1.0, q, a);
                }
    }
    // --- Gauss-Jordan with partial pivoting on the 10 x 20 system
    double* G = ws + kWsG * S;
    for (int c = 0; c < 10; ++c) {
        int piv = c;
        double best = G[(20 * c + c) * S] >= 0.0 ? G[(20 * c + c) * S] : -G[(20 * c + c) * S];
        for (int r = c + 1; r < 10; ++r) {
            const double v = G[(20 * r + c) * S] >= 0.0 ? G[(20 * r + c) * S] : -G[(20 * r + c) * S];
            if (v > best) {
                best = v;
                piv = r;
            }
        }
        if (!(best > 0.0) || !(best < 1e300)) return 0;   // degenerate sample (or NaN)
        if (piv != c)
            for (int k = c; k < 20; ++k) {
                const double t = G[(20 * c + k) * S];
                G[(20 * c + k) * S] = G[(20 * piv + k) * S];
                G[(20 * piv + k) * S] = t;
            }
        const double inv = 1.0 / G[(20 * c + c) * S];
        for (int k = c + 1; k < 20; ++k) G[(20 * c + k) * S] *= inv;
        G[(20 * c + c) * S] = 1.0;
        for (int r = 0; r < 10; ++r) {
            if (r == c) continue;
            const double f = G[(20 * r + c) * S];
            for (int k = c + 1; k < 20; ++k) G[(20 * r + k) * S] -= f * G[(20 * c + k) * S];
            G[(20 * r + c) * S] = 0.0;
        }
    }
    // --- B(z): rows <e> - z <f>, <g> - z <h>, <i> - z <j> (G rows 4 .. 9); columns x (deg 3), y (deg 3), 1 (deg 4), ascending
    double* Bz = ws + kWsQ * S;
MSFM_UNROLL
    for (int row = 0; row < 3; ++row) {
        const int ra = 4 + 2 * row, rb = 5 + 2 * row;
        // x: columns xz2 (10), xz (11), x (12); y: yz2 (13), yz (14), y (15); 1: z3 (16), z2 (17), z (18), 1 (19)
MSFM_UNROLL
        for (int v = 0; v < 2; ++v) {
            const int c0 = 10 + 3 * v;   // z^2, z, 1 columns: c0, c0 + 1, c0 + 2
            const int o = 13 * row + 4 * v;
            Bz[(o + 0) * S] = G[(20 * ra + c0 + 2) * S];
            Bz[(o + 1) * S] = G[(20 * ra + c0 + 1) * S] - G[(20 * rb + c0 + 2) * S];
            Bz[(o + 2) * S] = G[(20 * ra + c0) * S] - G[(20 * rb + c0 + 1) * S];
            Bz[(o + 3) * S] = -G[(20 * rb + c0) * S];
        }
        const int o = 13 * row + 8;
        Bz[(o + 0) * S] = G[(20 * ra + 19) * S];
        Bz[(o + 1) * S] = G[(20 * ra + 18) * S] - G[(20 * rb + 19) * S];
        Bz[(o + 2) * S] = G[(20 * ra + 17) * S] - G[(20 * rb + 18) * S];
        Bz[(o + 3) * S] = G[(20 * ra + 16) * S] - G[(20 * rb + 17) * S];
        Bz[(o + 4) * S] = -G[(20 * rb + 16) * S];
    }
    // --- det B(z), degree 10
    double p[11];
    {
        double b[3][13];
MSFM_UNROLL
        for (int r = 0; r < 3; ++r)
MSFM_UNROLL
            for (int k = 0; k < 13; ++k) b[r][k] = Bz[(13 * r + k) * S];
        // cofactors along the first row: b0x (b1y b2c - b1c b2y) - b0y (b1x b2c - b1c b2x) + b0c (b1x b2y - b1y b2x)
        double t1[8], t2[8], m[8], u[7], w[7], mc[7];
        pmul<4, 5>(b[1] + 4, b[2] + 8, t1);
        pmul<5, 4>(b[1] + 8, b[2] + 4, t2);
MSFM_UNROLL
        for (int k = 0; k < 8; ++k) m[k] = t1[k] - t2[k];
        double d0[11], d1[11], d2[11];
        pmul<4, 8>(b[0], m, d0);
        pmul<4, 5>(b[1], b[2] + 8, t1);
        pmul<5, 4>(b[1] + 8, b[2], t2);
MSFM_UNROLL
        for (int k = 0; k < 8; ++k) m[k] = t1[k] - t2[k];
        pmul<4, 8>(b[0] + 4, m, d1);
        pmul<4, 4>(b[1], b[2] + 4, u);
        pmul<4, 4>(b[1] + 4, b[2], w);
MSFM_UNROLL
        for (int k = 0; k < 7; ++k) mc[k] = u[k] - w[k];
        pmul<5, 7>(b[0] + 8, mc, d2);
MSFM_UNROLL
        for (int k = 0; k < 11; ++k) p[k] = d0[k] - d1[k] + d2[k];
    }
    // --- Sturm chain of the monic polynomial: s0 = p / p10, s1 = s0', s_{k+1} = -rem(s_{k-1}, s_k)
    if (!(p[10] > 0.0 || p[10] < 0.0) || !(p[10] < 1e300 && p[10] > -1e300)) return 0;
    double bound = 0.0, st[66];
    {
        const double inv = 1.0 / p[10];
MSFM_UNROLL
        for (int k = 0; k < 10; ++k) {
            const double m = p[k] * inv;
            st[k] = m;
            const double am = m >= 0.0 ? m : -m;
            bound = am > bound ? am : bound;
        }
        st[10] = 1.0;
        if (!(bound < 1e300)) return 0;
        bound = bound + 1.0;   // Cauchy: every root lies in (-bound, bound)
MSFM_UNROLL
        for (int k = 0; k < 10; ++k) st[11 + k] = (double)(k + 1) * st[k + 1];
    }
    {
        int oa = 0, ob = 11;   // s_{k-1} (degree d + 1), s_k (degree d)
MSFM_UNROLL
        for (int d = 9; d >= 1; --d) {
            const int oc = ob + d + 1;
            const double lead = st[ob + d];
            if (!(lead > 0.0 || lead < 0.0)) return 0;   // a non-generic chain: no model from this sample
            const double q1 = st[oa + d + 1] / lead;
            const double q0 = (st[oa + d] - q1 * st[ob + d - 1]) / lead;
MSFM_UNROLL
            for (int i = 0; i < d; ++i) {
                const double r = st[oa + i] - q0 * st[ob + i] - (i > 0 ? q1 * st[ob + i - 1] : 0.0);
                st[oc + i] = -r;
            }
            oa = ob;
            ob = oc;
        }
    }
    // sign changes at -inf and +inf from the leading coefficients (degree of s_k is 10 - k)
    int v_neg = 0, v_pos = 0;
    {
        int prev_n = 0, prev_p = 0, off = 0;
MSFM_UNROLL
        for (int d = 10; d >= 0; --d) {
            const double l = st[off + d];
            const int sp = l > 0.0 ? 1 : (l < 0.0 ? -1 : 0);
            const int sn = (d & 1) ? -sp : sp;
            if (sp != 0) {
                if (prev_p != 0 && sp != prev_p) ++v_pos;
                prev_p = sp;
                if (prev_n != 0 && sn != prev_n) ++v_neg;
                prev_n = sn;
            }
            off += d + 1;
        }
    }
    int nroots = v_neg - v_pos;
    if (nroots < 0) nroots = 0;
    if (nroots > kMaxSolutions) nroots = kMaxSolutions;
    int ns = 0;
    for (int j = 0; j < kMaxSolutions; ++j) {
        if (j >= nroots) break;
        // root j (ascending): the number of roots <= t is v_neg - V(t)
        double lo = -bound, hi = bound;
        for (int step = 0; step < kSturmSteps; ++step) {
            const double mid = 0.5 * (lo + hi);
            if (v_neg - sturm_changes(st, mid) > j) hi = mid;
            else lo = mid;
        }
        double z = 0.5 * (lo + hi);
        for (int step = 0; step < kNewtonSteps; ++step) {
            double f = 1.0, df = 0.0;
MSFM_UNROLL
            for (int i = 9; i >= 0; --i) {
                df = df * z + f;
                f = f * z + st[i];
            }
            if (df > 0.0 || df < 0.0) {   // (the counts of the bisection are themselves rounded near the root: the step may leave the bracket, by little)
                const double zn = z - f / df, dz = zn - z, az = z >= 0.0 ? z : -z;
                if ((dz >= 0.0 ? dz : -dz) <= 1e-6 * (1.0 + az)) z = zn;
            }
        }
        // B(z) and its null vector (x, y, 1): the cross product of the pair of rows with the largest last component
        double b[3][3];
MSFM_UNROLL
        for (int r = 0; r < 3; ++r)
MSFM_UNROLL
            for (int c = 0; c < 3; ++c) {
                const int o = 13 * r + 4 * c, deg = c < 2 ? 3 : 4;
                double v = Bz[(o + deg) * S];
MSFM_UNROLL
                for (int i = deg - 1; i >= 0; --i) v = v * z + Bz[(o + i) * S];
                b[r][c] = v;
            }
        double cx = 0.0, cy = 0.0, cz = 0.0, acz = -1.0;
MSFM_UNROLL
        for (int pr = 0; pr < 3; ++pr) {
            const int ra = pr == 2 ? 1 : 0, rb = pr == 0 ? 1 : 2;
            const double X = b[ra][1] * b[rb][2] - b[ra][2] * b[rb][1];
            const double Y = b[ra][2] * b[rb][0] - b[ra][0] * b[rb][2];
            const double Z = b[ra][0] * b[rb][1] - b[ra][1] * b[rb][0];
            const double a = Z >= 0.0 ? Z : -Z;
            if (a > acz) {
                acz = a;
                cx = X;
                cy = Y;
                cz = Z;
            }
        }
        if (!(acz > 0.0)) continue;
        double x = cx / cz, y = cy / cz;
        gauss_newton<S>(ws, x, y, z);
        double E[9], nn = 0.0;
MSFM_UNROLL
        for (int k = 0; k < 9; ++k) {
            E[k] = x * ws[(kWsNull + k) * S] + y * ws[(kWsNull + 9 + k) * S] + z * ws[(kWsNull + 18 + k) * S] + ws[(kWsNull + 27 + k) * S];
            nn += E[k] * E[k];
        }
        if (!(nn > 0.0) || !(nn < 1e300)) continue;
        nn = 1.0 / sqrt(nn);
MSFM_UNROLL
        for (int k = 0; k < 9; ++k) ws[(kWsSol + 9 * ns + k) * S] = E[k] * nn;
        ws[(kWsRoots + ns) * S] = z;
        ++ns;
    }
    return ns;
}

// hypothesis `it` of a pair with n >= 5 matches in normalised coordinates: its solutions in the workspace; returns the count
template <int S>
MSFM_FHD int hypothesis(const double* x1, const double* y1, const double* x2, const double* y2, int n, unsigned long long seed,
                        int it, double* ws) {
    int idx[5];
    sample5(seed, it, n, idx);
    double a[5], b[5], c[5], d[5];
MSFM_UNROLL
    for (int k = 0; k < 5; ++k) {
        a[k] = x1[idx[k]];
        b[k] = y1[idx[k]];
        c[k] = x2[idx[k]];
        d[k] = y2[idx[k]];
    }
    return five_point<S>(a, b, c, d, ws);
}

}  // namespace msfm_emat
