// msfm_triangulate.h -- track triangulation arithmetic shared by the device kernels (msfm_triangulate.hip.h, hipcc) and the host twin
// (host/HostTestApi.cpp, TriangulateTracks, g++): what the reference's MapBuilder::Triangulate -> Triangulator::Triangulate computes
// for one multi-view correspondence under known poses (src/Reconstruction/Triangulator.cpp:15-117, MapBuilder.cpp:516-560): the
// multi-view DLT point, the reprojection test in every view, the parallax test.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides -> the host
// twin and the device produce the SAME bits.  onesided_jacobi<4, 4>, acos and kDepthEps are msfm_pose.h's, undistort is msfm_emat.h's.
//
//   preconditions   a track is ATTEMPTED iff it is consistent (the track session's flag) and at least max(2, min_views) of its
//                   elements belong to an image with a valid pose.  Those elements are the USED OBSERVATIONS, in the track's element
//                   order (ascending (image id, keypoint index)); elements of unposed images are skipped.  Otherwise status = 0 and
//                   every other field 0.
//   observation     the pixel (x, y) of the uploaded keypoints, fp32 -> fp64, to normalised undistorted (u, v) by msfm_emat::undistort
//                   with the call's camera: the convention of the two-view records -- the error is measured
//                   against the undistorted observation and scaled by f = (fx + fy) / 2.  THE REFERENCE folds K into P = K [R | t] and
//                   compares with the distorted pixel; for a camera without distortion and fx = fy the two agree up to rounding.
//   DLT             P = [R | t] (x_cam = R X + t; R is taken as given, NOT re-orthogonalised).  A (4 x 4) starts at 0; per used
//                   observation, in order:  A += r1^T r1;  A += r2^T r2  with r1 = u P.row(2) - P.row(0), r2 = v P.row(2) - P.row(1)
//                   (two separate additions per entry).  onesided_jacobi<4, 4> on the columns of A; h = the column of V whose rotated
//                   column of A has the smallest norm, the lowest index among equal norms; X = h[0..2] / h[3].  h[3] == 0 or a
//                   non-finite X: no point (status = ATTEMPTED alone, every residual slot -1).
//   per observation Y = R X + t;  depth_ok: Y.z > kDepthEps;  err = sqrt((Y.x / Y.z - u)^2 + (Y.y / Y.z - v)^2) * f.  EVERY error is
//                   computed and reported (the reference stops at the first failure: the same verdict).  ERROR_OK iff err <= max_error
//                   holds for every used observation (a NaN fails).  mean_residual = (the errors summed in observation order from 0.0)
//                   / count, reported whenever a point exists.
//   parallax        camera centres O = -R^T t, once per pose, by centre() below (Projection.cpp:149-194).  parallax_scan() below, THE
//                   scan of this stage: pairs in the reference's loop order, for i: for j < i over the used observations; the scan
//                   stops at the first pair with angle >= min_angle and tri_angle is that pair's angle (ANGLE_OK set); if none
//                   reaches it tri_angle is the largest angle seen (ANGLE_OK clear).  Angle as msfm_pose::evaluate: law of cosines,
//                   |acos|, NaN -> 0, min(a, pi - a), degrees.
//   status bits     MSFM_TRI_ATTEMPTED 1, _POINT 2, _ERROR_OK 4, _ANGLE_OK 8, _DEPTH_OK 16 (every used view in front).  The
//                   reference's is_succeed is POINT & ERROR_OK & ANGLE_OK.  THE REFERENCE HAS NO DEPTH TEST: DEPTH_OK is extra
//                   information and not part of the verdict.
#pragma once

#include "msfm_pose.h"

namespace msfm_tri {

// a pose as the kernels and the twin read it: the caller's [R | t] plus the centre (128 bytes)
struct Pose {
    double R[9], t[3], O[3];
    int32_t valid, reserved;
};

struct Params {
    double max_error, min_angle;
    int32_t min_views, reserved;
};

// O = -R^T t
MSFM_FHD void centre(const double R[9], const double t[3], double O[3]) {
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) O[k] = -(R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]);
}

// the caller's pose -> the table entry: valid iff flagged valid and every number finite
MSFM_FHD void prepare_pose(const msfm_pose_rt& in, Pose* out) {
    bool ok = in.valid != 0;
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) {
        out->R[k] = in.R[k];
        ok = ok && msfm_pose::finite(in.R[k]);
    }
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) {
        out->t[k] = in.t[k];
        ok = ok && msfm_pose::finite(in.t[k]);
    }
    centre(in.R, in.t, out->O);
    out->valid = ok ? 1 : 0;
    out->reserved = 0;
}

// the parallax angle at X between the centres Oi and Oj, degrees (Projection::CalculateParallaxAngle; msfm_pose::evaluate's form)
MSFM_FHD double parallax(const double X[3], const double Oi[3], const double Oj[3]) {
    const double b0 = Oi[0] - Oj[0], b1 = Oi[1] - Oj[1], b2 = Oi[2] - Oj[2];
    const double baseline = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    const double d0 = X[0] - Oi[0], d1 = X[1] - Oi[1], d2 = X[2] - Oi[2];
    const double ray1 = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
    const double e0 = X[0] - Oj[0], e1 = X[1] - Oj[1], e2 = X[2] - Oj[2];
    const double ray2 = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
    double ang = msfm_pose::acos((ray1 * ray1 + ray2 * ray2 - baseline * baseline) / (2.0 * ray1 * ray2));
    if (ang < 0.0) ang = -ang;
    if (!(ang == ang)) return 0.0;   // NaN -> 0
    const double other = msfm_pose::kPi - ang;
    return (ang < other ? ang : other) * 180.0 / msfm_pose::kPi;
}

MSFM_FHD void clear_point(msfm_point3d* r) {
    r->status = 0;
    r->n_views = 0;
    r->X[0] = r->X[1] = r->X[2] = 0.0;
    r->mean_residual = 0.0;
    r->tri_angle = 0.0;
}

// The parallax scan at X over the elements k = 0 .. n - 1.  centre_of(k) -> the camera centre of element k (const double*), nullptr:
// the element takes no part.  Pairs in the order  for i: for j < i;  the scan stops at the first pair whose angle is >= min_angle:
// true, *angle = that pair's angle.  No such pair: false, *angle = the largest angle seen (0.0 without a pair).
template <class C>
MSFM_FHD bool parallax_scan(const double X[3], int n, double min_angle, C centre_of, double* angle_out) {
    bool angle_ok = false;
    double angle = 0.0;
    for (int i = 1; i < n && !angle_ok; ++i) {
        const double* ci = centre_of(i);
        if (!ci) continue;
        const double Oi[3] = {ci[0], ci[1], ci[2]};
        for (int j = 0; j < i; ++j) {
            const double* cj = centre_of(j);
            if (!cj) continue;
            const double Oj[3] = {cj[0], cj[1], cj[2]};
            const double g = parallax(X, Oi, Oj);
            if (g >= min_angle) {
                angle = g;
                angle_ok = true;
                break;
            }
            if (g > angle) angle = g;
        }
    }
    *angle_out = angle;
    return angle_ok;
}

// Y = R X + t
MSFM_FHD void transform(const double R[9], const double t[3], const double X[3], double Y[3]) {
    Y[0] = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
    Y[1] = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
    Y[2] = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
}

// triangulate_track's DLT in pieces: the normal matrix (m[j][i]: column j, row i) of no observation, one observation added, the point
MSFM_FHD void dlt_clear(double m[4][4]) {
MSFM_UNROLL
    for (int j = 0; j < 4; ++j)
MSFM_UNROLL
        for (int i = 0; i < 4; ++i) m[j][i] = 0.0;
}

MSFM_FHD void dlt_add(double m[4][4], const double R[9], const double t[3], double u, double w) {
    double r1[4], r2[4];
MSFM_UNROLL
    for (int j = 0; j < 4; ++j) {
        const double p0 = j < 3 ? R[j] : t[0], p1 = j < 3 ? R[3 + j] : t[1], p2 = j < 3 ? R[6 + j] : t[2];
        r1[j] = u * p2 - p0;
        r2[j] = w * p2 - p1;
    }
MSFM_UNROLL
    for (int j = 0; j < 4; ++j)
MSFM_UNROLL
        for (int i = 0; i < 4; ++i) {
            m[j][i] = m[j][i] + r1[i] * r1[j];
            m[j][i] = m[j][i] + r2[i] * r2[j];
        }
}

// (m is destroyed.)  False: no point.
MSFM_FHD bool dlt_solve(double m[4][4], double X[3]) {
    double v[4][4];
    msfm_pose::onesided_jacobi<4, 4>(m, v);
    double best = 0.0, h[4] = {0.0, 0.0, 0.0, 0.0};
MSFM_UNROLL
    for (int j = 0; j < 4; ++j) {
        const double nn = m[j][0] * m[j][0] + m[j][1] * m[j][1] + m[j][2] * m[j][2] + m[j][3] * m[j][3];
        if (j == 0 || nn < best) {
            best = nn;
MSFM_UNROLL
            for (int k = 0; k < 4; ++k) h[k] = v[j][k];
        }
    }
    X[0] = X[1] = X[2] = 0.0;
    if (!(h[3] > 0.0 || h[3] < 0.0)) return false;
    X[0] = h[0] / h[3];
    X[1] = h[1] / h[3];
    X[2] = h[2] / h[3];
    return msfm_pose::finite(X[0]) && msfm_pose::finite(X[1]) && msfm_pose::finite(X[2]);
}

// the reprojection error of X in one view, pixels (f = (fx + fy) / 2), and whether X lies in front of it
MSFM_FHD double obs_error(const double R[9], const double t[3], double u, double w, const double X[3], double f, bool* depth) {
    double Y[3];
    transform(R, t, X, Y);
    *depth = Y[2] > msfm_pose::kDepthEps;
    const double dx = Y[0] / Y[2] - u, dy = Y[1] / Y[2] - w;
    return sqrt(dx * dx + dy * dy) * f;
}

MSFM_FHD bool obs_inlier(const double R[9], const double t[3], double u, double w, const double X[3], double f, double max_error) {
    bool depth;
    const double err = obs_error(R, t, u, w, X, f, &depth);
    return depth && err <= max_error;   // (false for a NaN)
}

// the elements of `a` whose mask byte is set (the mask is element-aligned; a set byte belongs to a posed element)
template <class A>
struct Masked {
    const A& a;
    const uint8_t* mask;
    MSFM_FHD const Pose* pose(int k) const { return mask[k] ? a.pose(k) : nullptr; }
    MSFM_FHD void pixel(int k, double* x, double* y) const { a.pixel(k, x, y); }
};

// the DLT point over the posed elements of `a`, in element order
template <class A>
MSFM_FHD bool dlt_point(const A& a, int n, const msfm_emat::Camera& cam, double X[3]) {
    double m[4][4];
    dlt_clear(m);
    for (int k = 0; k < n; ++k) {
        const Pose* p = a.pose(k);
        if (!p) continue;
        double x, y, u, w;
        a.pixel(k, &x, &y);
        msfm_emat::undistort(cam, x, y, &u, &w);
        dlt_add(m, p->R, p->t, u, w);
    }
    return dlt_solve(m, X);
}

// (The DLT, the error pass and the scan are written out here, not called: tri_track_kernel measured 1 .. 1.5 % slower at the bench's
// default setting with this function built from dlt_clear / dlt_add / dlt_solve, obs_error and parallax_scan, which are the same
// arithmetic and what every other site calls -- DESIGN.md section 15.)
// One track.  `a` gives the track's elements k = 0 .. n - 1:  a.pose(k) -> const Pose* (nullptr: the element's image has no valid
// pose),  a.pixel(k, &x, &y) -> the keypoint's pixel as fp64 (asked for posed elements only).  residuals: n slots, element-aligned;
// -1.0 where no error was computed.  The arithmetic does not depend on where `a` reads from.
template <class A>
MSFM_FHD void triangulate_track(const A& a, int n, bool consistent, const msfm_emat::Camera& cam, const Params& prm, msfm_point3d* rec,
                                double* residuals) {
    clear_point(rec);
    const int need = prm.min_views > 2 ? prm.min_views : 2;
    int used = 0;
    if (consistent)
        for (int k = 0; k < n; ++k) used += a.pose(k) ? 1 : 0;
    if (!consistent || used < need) {
        for (int k = 0; k < n; ++k) residuals[k] = -1.0;
        return;
    }
    rec->status = MSFM_TRI_ATTEMPTED;
    rec->n_views = used;
    double m[4][4], v[4][4];   // m[j][i]: column j, row i of A
MSFM_UNROLL
    for (int j = 0; j < 4; ++j)
MSFM_UNROLL
        for (int i = 0; i < 4; ++i) m[j][i] = 0.0;
    for (int k = 0; k < n; ++k) {
        const Pose* p = a.pose(k);
        if (!p) continue;
        double x, y, u, w;
        a.pixel(k, &x, &y);
        msfm_emat::undistort(cam, x, y, &u, &w);
        double r1[4], r2[4];
MSFM_UNROLL
        for (int j = 0; j < 4; ++j) {
            const double p0 = j < 3 ? p->R[j] : p->t[0], p1 = j < 3 ? p->R[3 + j] : p->t[1], p2 = j < 3 ? p->R[6 + j] : p->t[2];
            r1[j] = u * p2 - p0;
            r2[j] = w * p2 - p1;
        }
MSFM_UNROLL
        for (int j = 0; j < 4; ++j)
MSFM_UNROLL
            for (int i = 0; i < 4; ++i) {
                m[j][i] = m[j][i] + r1[i] * r1[j];
                m[j][i] = m[j][i] + r2[i] * r2[j];
            }
    }
    msfm_pose::onesided_jacobi<4, 4>(m, v);
    double best = 0.0, h[4] = {0.0, 0.0, 0.0, 0.0};
MSFM_UNROLL
    for (int j = 0; j < 4; ++j) {
        const double nn = m[j][0] * m[j][0] + m[j][1] * m[j][1] + m[j][2] * m[j][2] + m[j][3] * m[j][3];
        if (j == 0 || nn < best) {
            best = nn;
MSFM_UNROLL
            for (int k = 0; k < 4; ++k) h[k] = v[j][k];
        }
    }
    double X[3] = {0.0, 0.0, 0.0};
    bool point = h[3] > 0.0 || h[3] < 0.0;
    if (point) {
        X[0] = h[0] / h[3];
        X[1] = h[1] / h[3];
        X[2] = h[2] / h[3];
        point = msfm_pose::finite(X[0]) && msfm_pose::finite(X[1]) && msfm_pose::finite(X[2]);
    }
    if (!point) {
        for (int k = 0; k < n; ++k) residuals[k] = -1.0;
        return;
    }
    const double f = (cam.fx + cam.fy) / 2.0;
    bool error_ok = true, depth_ok = true;
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
        const Pose* p = a.pose(k);
        if (!p) {
            residuals[k] = -1.0;
            continue;
        }
        double x, y, u, w;
        a.pixel(k, &x, &y);
        msfm_emat::undistort(cam, x, y, &u, &w);
        const double Y0 = p->R[0] * X[0] + p->R[1] * X[1] + p->R[2] * X[2] + p->t[0];
        const double Y1 = p->R[3] * X[0] + p->R[4] * X[1] + p->R[5] * X[2] + p->t[1];
        const double Y2 = p->R[6] * X[0] + p->R[7] * X[1] + p->R[8] * X[2] + p->t[2];
        depth_ok = depth_ok && Y2 > msfm_pose::kDepthEps;
        const double dx = Y0 / Y2 - u, dy = Y1 / Y2 - w;
        const double err = sqrt(dx * dx + dy * dy) * f;
        error_ok = error_ok && err <= prm.max_error;   // (false for a NaN)
        sum = sum + err;
        residuals[k] = msfm_pose::canonical(err);
    }
    // the parallax scan: for i: for j < i over the used observations, to the first pair that reaches min_angle
    bool angle_ok = false;
    double angle = 0.0;
    for (int i = 1; i < n && !angle_ok; ++i) {
        const Pose* pi = a.pose(i);
        if (!pi) continue;
        const double Oi[3] = {pi->O[0], pi->O[1], pi->O[2]};
        for (int j = 0; j < i; ++j) {
            const Pose* pj = a.pose(j);
            if (!pj) continue;
            const double Oj[3] = {pj->O[0], pj->O[1], pj->O[2]};
            const double g = parallax(X, Oi, Oj);
            if (g >= prm.min_angle) {
                angle = g;
                angle_ok = true;
                break;
            }
            if (g > angle) angle = g;
        }
    }
    rec->status = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | (error_ok ? MSFM_TRI_ERROR_OK : 0) | (angle_ok ? MSFM_TRI_ANGLE_OK : 0) |
                  (depth_ok ? MSFM_TRI_DEPTH_OK : 0);
    rec->X[0] = X[0];
    rec->X[1] = X[1];
    rec->X[2] = X[2];
    rec->mean_residual = sum / (double)used;
    rec->tri_angle = angle;
}

// ---- robust triangulation: a per-track consensus over two-view hypotheses -------------------------------------
// For one consistent track with the used observations 0 .. m - 1 (the posed elements, in element order), need = max(2, min_views):
//   plain pass      P0 = triangulate_track.  Not ATTEMPTED, or POINT & ERROR_OK, or m < 3: the record is P0 bit for bit, the mask is 1
//                   on every used observation, ROBUST is clear (retry() below is the test).
//   hypotheses      H = min(m (m - 1) / 2, max_hypotheses).  All pairs fit: hypothesis h is the h-th pair of  for i: for j < i
//                   (pair_of).  Otherwise two distinct positions from sample2 under tri_seed(track number), the larger one i.  X_h: the
//                   DLT over the two observations alone (dlt_add of j, then of i; dlt_solve).  Valid iff it has a point, both depths
//                   are > kDepthEps and parallax(X_h, O_i, O_j) >= min_angle.  count_h: the used observations with depth > kDepthEps
//                   and err <= max_error (obs_error; a NaN fails).  Best: the largest count, the lowest h among equals.  No valid
//                   hypothesis or a best count < need: status = ATTEMPTED | ROBUST, every other field 0, residuals -1, mask 0.
//   refit, once     mask1 = the inliers of X_best;  R1 = the DLT over mask1 (dlt_point on Masked);  mask2 = the inliers of R1 among all
//                   used observations;  R1 stands iff it has a point and |mask2| >= max(|mask1|, need), else X_best with mask1.
//   record          evaluate_point: an error for EVERY used observation (-1 for unposed elements), n_views = |mask|, mean_residual =
//                   the inliers' errors summed in element order from 0.0 / |mask|, parallax_scan over the inliers, ERROR_OK set,
//                   DEPTH_OK over the inliers, ROBUST set.
constexpr unsigned long long kTriSeed = 0x547269616e67756cULL;

struct RobustParams {
    double max_error, min_angle;
    int32_t min_views, max_hypotheses;
};

MSFM_FHD unsigned long long tri_seed(long long track) { return msfm_fmat::mix64(kTriSeed ^ (unsigned long long)track); }

// the 2 distinct positions of hypothesis `it` (n >= 2): sample8's stream, k < 2
MSFM_FHD void sample2(unsigned long long seed, int it, int n, int idx[2]) {
    using msfm_fmat::mix64;
    idx[0] = idx[1] = -1;
MSFM_UNROLL
    for (int k = 0; k < 2; ++k) {
        int c = 0;
        for (int attempt = 0;; ++attempt) {
            c = attempt < 32 ? (int)(mix64(seed ^ mix64(((unsigned long long)it << 20) ^ ((unsigned long long)k << 8) ^ (unsigned long long)attempt)) % (unsigned long long)n)
                             : (c + 1) % n;  // linear probe: terminates because n >= 2
            if (!(idx[0] == c || idx[1] == c)) break;
        }
        idx[k] = c;
    }
}

// the h-th pair (i, j), j < i, of the scan order  for i in 1 ..: for j < i
MSFM_FHD void pair_of(int h, int* i, int* j) {
    int a = 1;
    while ((a + 1) * a / 2 <= h) ++a;
    *i = a;
    *j = h - a * (a - 1) / 2;
}

MSFM_FHD long long hypotheses_of(int m, int max_hypotheses) {
    const long long pairs = (long long)m * (m - 1) / 2;
    return pairs < max_hypotheses ? pairs : max_hypotheses;
}

// the two positions of hypothesis h of a track with m used observations: *j < *i
MSFM_FHD void hypothesis_pair(unsigned long long seed, int h, int m, int max_hypotheses, int* i, int* j) {
    if ((long long)m * (m - 1) / 2 <= max_hypotheses) {
        pair_of(h, i, j);
        return;
    }
    int idx[2];
    sample2(seed, h, m, idx);
    *i = idx[0] > idx[1] ? idx[0] : idx[1];
    *j = idx[0] > idx[1] ? idx[1] : idx[0];
}

// step 1's verdict on the plain record of a track with m used observations
MSFM_FHD bool retry(const msfm_point3d& p0, int m) {
    const int done = MSFM_TRI_POINT | MSFM_TRI_ERROR_OK;
    return (p0.status & MSFM_TRI_ATTEMPTED) && (p0.status & done) != done && m >= 3;
}

// the record of a retried track without a consensus
MSFM_FHD void robust_failed(int n, msfm_point3d* rec, double* residuals, uint8_t* mask) {
    clear_point(rec);
    rec->status = MSFM_TRI_ATTEMPTED | MSFM_TRI_ROBUST;
    for (int k = 0; k < n; ++k) {
        residuals[k] = -1.0;
        mask[k] = 0;
    }
}

// the record of X under the inlier mask (at least one byte set)
template <class A>
MSFM_FHD void evaluate_point(const A& a, int n, const double X[3], const uint8_t* mask, const msfm_emat::Camera& cam, double min_angle,
                             msfm_point3d* rec, double* residuals) {
    const double f = (cam.fx + cam.fy) / 2.0;
    bool depth_ok = true;
    double sum = 0.0;
    int count = 0;
    for (int k = 0; k < n; ++k) {
        const Pose* p = a.pose(k);
        if (!p) {
            residuals[k] = -1.0;
            continue;
        }
        double x, y, u, w;
        a.pixel(k, &x, &y);
        msfm_emat::undistort(cam, x, y, &u, &w);
        bool depth;
        const double err = obs_error(p->R, p->t, u, w, X, f, &depth);
        residuals[k] = msfm_pose::canonical(err);
        if (mask[k]) {
            depth_ok = depth_ok && depth;
            sum = sum + err;
            count += 1;
        }
    }
    double angle;
    const bool angle_ok = parallax_scan(X, n, min_angle, [&](int k) -> const double* { return mask[k] ? a.pose(k)->O : nullptr; }, &angle);
    rec->status = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | MSFM_TRI_ERROR_OK | (angle_ok ? MSFM_TRI_ANGLE_OK : 0) |
                  (depth_ok ? MSFM_TRI_DEPTH_OK : 0) | MSFM_TRI_ROBUST;
    rec->n_views = count;
    rec->X[0] = X[0];
    rec->X[1] = X[1];
    rec->X[2] = X[2];
    rec->mean_residual = sum / (double)count;
    rec->tri_angle = angle;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: TriangulateTracks over a finished track result ---------------------------------------------------------------
// tracks as msfm_fetch_tracks returns them; kxy[rank]: the (x, y) fp32 pairs of the image of that rank (may be null for an image
// without a valid pose); poses[rank]: prepared by prepare_pose; rank_of_id: per image id the rank or -1.
struct HostTrack {
    const int32_t* img;
    const int32_t* idx;
    const int* rank_of_id;
    const float* const* kxy;
    const Pose* poses;
    const Pose* pose(int k) const {
        const int r = rank_of_id[img[k]];
        return (r >= 0 && poses[r].valid) ? poses + r : nullptr;
    }
    void pixel(int k, double* x, double* y) const {
        const float* q = kxy[rank_of_id[img[k]]] + 2 * (size_t)idx[k];
        *x = (double)q[0];
        *y = (double)q[1];
    }
};

inline void TriangulateTracks(const int64_t* offsets, const int32_t* image_ids, const int32_t* point_idx, const uint8_t* consistent,
                              int64_t first_track, int64_t n_tracks, const int* rank_of_id, const float* const* kxy, const Pose* poses,
                              const msfm_emat::Camera& cam, const Params& prm, msfm_point3d* out_points, double* out_residuals) {
    for (int64_t t = first_track; t < first_track + n_tracks; ++t) {
        const int64_t b = offsets[t], e = offsets[t + 1];
        const HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
        triangulate_track(a, (int)(e - b), consistent[t] != 0, cam, prm, out_points + t, out_residuals + b);
    }
}

// the used observations of one track by position, as the hypotheses read them
struct HostObs {
    std::vector<int> elem;
    std::vector<double> u, w;
    std::vector<const Pose*> p;
};

struct RobustCounts {
    long long retried, rescued, observations_rejected, hypotheses;
};

// Which route one track took through the definition above: what the tests assert before they trust a byte comparison to have met a
// branch.  Twelve int32.  A track that is not retried: retried 0, m, everything else as set by trace_clear.
struct RobustTrace {
    int32_t retried;               // 1: the track went through the hypotheses
    int32_t m;                     // used observations
    int32_t hypotheses;            // H
    int32_t winner;                // the winning hypothesis, -1: none was valid
    int32_t best;                  // its count, -1: none was valid
    int32_t valid;                 // hypotheses that were valid
    int32_t depth_rejected;        // hypotheses with a point and parallax >= min_angle whose sampled views fail the depth test
    int32_t depth_rejected_best;   // the largest count_h among those (over ALL used observations), -1: none
    int32_t mask1;                 // |mask1|, -1: no consensus
    int32_t mask2;                 // |mask2|, -1: no consensus or the refit had no point
    int32_t refit_stood;           // 1: R1 stands
    int32_t flipped;               // bytes that differ between mask1 and the final mask
};

inline void trace_clear(RobustTrace* tr, int m) {
    *tr = RobustTrace{0, m, 0, -1, -1, 0, 0, -1, -1, -1, 0, 0};
}

// One track, literally the definition above.  mask: n bytes, element-aligned.  `counts` (may be null) is added to.  `trace` (may be
// null) is filled; nothing the function computes depends on it.
template <class A>
inline void robust_track(const A& a, int n, bool consistent, long long track, const msfm_emat::Camera& cam, const RobustParams& prm,
                         msfm_point3d* rec, double* residuals, uint8_t* mask, RobustCounts* counts, RobustTrace* trace = nullptr) {
    const Params plain = {prm.max_error, prm.min_angle, prm.min_views, 0};
    triangulate_track(a, n, consistent, cam, plain, rec, residuals);
    HostObs o;
    const bool attempted = (rec->status & MSFM_TRI_ATTEMPTED) != 0;
    for (int k = 0; k < n; ++k) {
        const Pose* p = attempted ? a.pose(k) : nullptr;
        mask[k] = p ? 1 : 0;
        if (!p) continue;
        double x, y, u, w;
        a.pixel(k, &x, &y);
        msfm_emat::undistort(cam, x, y, &u, &w);
        o.elem.push_back(k);
        o.u.push_back(u);
        o.w.push_back(w);
        o.p.push_back(p);
    }
    const int m = (int)o.elem.size();
    if (trace) trace_clear(trace, m);
    if (!retry(*rec, m)) return;
    const int need = prm.min_views > 2 ? prm.min_views : 2;
    const double f = (cam.fx + cam.fy) / 2.0;
    const int H = (int)hypotheses_of(m, prm.max_hypotheses);
    const unsigned long long seed = tri_seed(track);
    int best = -1;
    double Xb[3] = {0.0, 0.0, 0.0};
    for (int h = 0; h < H; ++h) {
        int i, j;
        hypothesis_pair(seed, h, m, prm.max_hypotheses, &i, &j);
        double A4[4][4], X[3];
        dlt_clear(A4);
        dlt_add(A4, o.p[(size_t)j]->R, o.p[(size_t)j]->t, o.u[(size_t)j], o.w[(size_t)j]);
        dlt_add(A4, o.p[(size_t)i]->R, o.p[(size_t)i]->t, o.u[(size_t)i], o.w[(size_t)i]);
        const bool point = dlt_solve(A4, X);
        bool valid = point;
        int count = 0;
        for (int k = 0; k < m && valid; ++k) {
            const bool in = obs_inlier(o.p[(size_t)k]->R, o.p[(size_t)k]->t, o.u[(size_t)k], o.w[(size_t)k], X, f, prm.max_error);
            if (k == i || k == j) {
                bool depth;
                (void)obs_error(o.p[(size_t)k]->R, o.p[(size_t)k]->t, o.u[(size_t)k], o.w[(size_t)k], X, f, &depth);
                valid = depth;
            }
            count += in ? 1 : 0;
        }
        valid = valid && parallax(X, o.p[(size_t)i]->O, o.p[(size_t)j]->O) >= prm.min_angle;
        if (trace) {
            trace->valid += valid ? 1 : 0;
            if (valid && count > best) trace->winner = h;
            bool di, dj;
            (void)obs_error(o.p[(size_t)i]->R, o.p[(size_t)i]->t, o.u[(size_t)i], o.w[(size_t)i], X, f, &di);
            (void)obs_error(o.p[(size_t)j]->R, o.p[(size_t)j]->t, o.u[(size_t)j], o.w[(size_t)j], X, f, &dj);
            if (point && !(di && dj) && parallax(X, o.p[(size_t)i]->O, o.p[(size_t)j]->O) >= prm.min_angle) {
                int full = 0;
                for (int k = 0; k < m; ++k)
                    full += obs_inlier(o.p[(size_t)k]->R, o.p[(size_t)k]->t, o.u[(size_t)k], o.w[(size_t)k], X, f, prm.max_error) ? 1 : 0;
                trace->depth_rejected += 1;
                if (full > trace->depth_rejected_best) trace->depth_rejected_best = full;
            }
        }
        if (valid && count > best) {
            best = count;
            Xb[0] = X[0];
            Xb[1] = X[1];
            Xb[2] = X[2];
        }
    }
    if (counts) {
        counts->retried += 1;
        counts->hypotheses += H;
    }
    if (trace) {
        trace->retried = 1;
        trace->hypotheses = H;
        trace->best = best;
    }
    if (best < need) {
        robust_failed(n, rec, residuals, mask);
        return;
    }
    int n1 = 0;
    for (int k = 0; k < m; ++k) {
        const bool in = obs_inlier(o.p[(size_t)k]->R, o.p[(size_t)k]->t, o.u[(size_t)k], o.w[(size_t)k], Xb, f, prm.max_error);
        mask[o.elem[(size_t)k]] = in ? 1 : 0;
        n1 += in ? 1 : 0;
    }
    std::vector<uint8_t> first;
    if (trace) {
        trace->mask1 = n1;
        first.assign(mask, mask + n);
    }
    double X1[3];
    const Masked<A> masked{a, mask};
    if (dlt_point(masked, n, cam, X1)) {
        int n2 = 0;
        for (int k = 0; k < m; ++k) n2 += obs_inlier(o.p[(size_t)k]->R, o.p[(size_t)k]->t, o.u[(size_t)k], o.w[(size_t)k], X1, f, prm.max_error) ? 1 : 0;
        if (trace) trace->mask2 = n2;
        if (n2 >= (n1 > need ? n1 : need)) {
            if (trace) trace->refit_stood = 1;
            for (int k = 0; k < m; ++k)
                mask[o.elem[(size_t)k]] = obs_inlier(o.p[(size_t)k]->R, o.p[(size_t)k]->t, o.u[(size_t)k], o.w[(size_t)k], X1, f, prm.max_error) ? 1 : 0;
            n1 = n2;
            Xb[0] = X1[0];
            Xb[1] = X1[1];
            Xb[2] = X1[2];
        }
    }
    if (trace)
        for (int k = 0; k < n; ++k) trace->flipped += first[(size_t)k] != mask[k] ? 1 : 0;
    evaluate_point(a, n, Xb, mask, cam, prm.min_angle, rec, residuals);
    if (counts) {
        counts->rescued += (rec->status & MSFM_TRI_ANGLE_OK) ? 1 : 0;
        counts->observations_rejected += m - n1;
    }
}

inline void TriangulateTracksRobust(const int64_t* offsets, const int32_t* image_ids, const int32_t* point_idx, const uint8_t* consistent,
                                    int64_t first_track, int64_t n_tracks, const int* rank_of_id, const float* const* kxy,
                                    const Pose* poses, const msfm_emat::Camera& cam, const RobustParams& prm, msfm_point3d* out_points,
                                    double* out_residuals, uint8_t* out_mask, RobustCounts* counts, RobustTrace* out_trace = nullptr) {
    for (int64_t t = first_track; t < first_track + n_tracks; ++t) {
        const int64_t b = offsets[t], e = offsets[t + 1];
        const HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
        robust_track(a, (int)(e - b), consistent[t] != 0, (long long)t, cam, prm, out_points + t, out_residuals + b, out_mask + b, counts,
                     out_trace ? out_trace + t : nullptr);
    }
}
#endif

}  // namespace msfm_tri
