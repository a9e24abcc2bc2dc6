// msfm_refine_poses.h -- pose refinement arithmetic shared by the device kernels (msfm_refine_poses.hip.h, hipcc) and the host twin
// (host/HostTestApi.cpp, RefinePoses, g++): every posed image is moved to the minimum of its reprojection error under FIXED points by
// Levenberg-Marquardt, one 6 x 6 system per image.  The pose block of a bundle adjustment and nothing more:
// msfm_refine.h is the point block, a caller alternates the two.  Points' X, tracks and inlier bytes never change.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides -> the host
// twin and the device produce the SAME bits.  Obs, prepare_obs, eligible, the LM constants and STOP_* are msfm_refine.h's, gn_add and
// kRegSums msfm_register.h's (used as they are), obs_error, parallax, centre msfm_triangulate.h's, kDepthEps msfm_pose.h's.
//
//   listed image    an image of the pose list of the triangulation call that made the points.
//   fitting set     of a listed image I with a valid pose that is not held fixed: every OBS_FIT observation in I of a track whose
//                   record has ATTEMPTED | POINT | ERROR_OK | ANGLE_OK (the points register_images trusts), by ascending track number
//                   (such a track is consistent: at most one observation per image).  An entry is (u, w) of the Obs and X of the record.
//   eligible        a valid pose, not fixed, and a fitting set of at least min_observations entries.
//   cost            c(R, t) = sum of rx^2 + ry^2,  Y = R X + t,  rx = (Y.x / Y.z - u) f,  ry = (Y.y / Y.z - w) f,  f = (fx + fy) / 2:
//                   the cost of msfm_refine.h, in pixels (rx^2 is added before ry^2).
//   normal system   the 27 sums of msfm_reg::gn_add (normalised units: the damped step is invariant under that scale).
//   summation       for the 27 sums and the cost alike: partial j < 64 sums the list positions j, j + 64, .. from 0.0, then the
//                   butterfly v_j <- v_j + v_(j xor s) for s = 32, 16, .., 1 (every j ends with the same bits).
//   step            (H + lambda diag H) delta = -g by the 6 x 6 Cholesky of gn_step's shape; delta = (a, dt) applied as R <- C(a) R,
//                   t <- C(a) t + dt with Cayley's C.  A pivot that is not > 0, a non-finite delta or a non-finite new pose: the step is
//                   rejected without a cost evaluation.
//   LM              lambda = kLambda0; c = c(R, t).  While fewer than max_iters steps have been evaluated:
//                     (the 27 sums are recomputed only after the pose changed.)  One step is evaluated.
//                     ACCEPTED iff its cost is finite, strictly lower and every fitting observation keeps Y.z > kDepthEps:
//                       lambda = max(lambda / 10, kLambdaFloor);  stop (STEP) iff a.a + dt.dt <= step_tol^2 (1 + t.t), t the new one
//                       (the 1: a camera at the origin must be able to stop).
//                     REJECTED otherwise:  lambda = 10 lambda;  stop (CEILING) iff lambda > kLambdaCeiling.
//                   Leaving the loop at max_iters evaluated steps: MAX_ITERS (also for max_iters = 0).
//   standing        the refined pose STANDS iff a step was accepted and the number of fitting observations with Y.z > kDepthEps and
//                   err <= max_error (obs_error, the triangulation's threshold) is not lower under it than under the old pose: the rule
//                   of MSFM_REG_REFINED.  It then replaces the pose (the centre by msfm_tri::centre); otherwise nothing changes.
//   re-verdict      every eligible track (ATTEMPTED | POINT) with a USED observation in an image whose pose changed, at its unchanged X
//                   under the new poses: the verdict block of msfm_ref::refine_track -- err of every USED observation; over the fitting
//                   set, in observation order, the errors' sum, ERROR_OK, DEPTH_OK, the parallax scan.  status = ATTEMPTED | POINT | the
//                   three bits | the record's ROBUST and REFINED bits | REPOSED; mean_residual, tri_angle and the residual slots of the
//                   USED observations are rewritten; n_views and X are kept.
#pragma once

#include "msfm_refine.h"
#include "msfm_register.h"

namespace msfm_rp {

constexpr int kLanes = 64;   // partial sums = lanes of the wave that owns an image
enum { NOT_ELIGIBLE = 1, NO_ACCEPTED_STEP = 2, LOST_INLIERS = 3 };   // why a pose did not stand (Trace::verdict); 0: it stands

struct Params {
    double step_tol;
    int32_t max_iters, min_observations;
};

// what refine_image leaves besides the pose
struct Result {
    int32_t stands, iterations, stop, inliers_before, inliers_after, accepted;
    double cost_before, cost_after;
};

// what one re-verdict adds to the call's statistics
struct Tally {
    int32_t reposed, lost, gained;
};

// The route one image took: host only (the device passes nullptr).  Six int32 and two doubles, 40 bytes.
struct Trace {
    int32_t steps;                    // evaluated steps
    int32_t accepted;                 // ... of which accepted
    int32_t stop;                     // msfm_ref::STOP_*
    int32_t verdict;                  // 0: stands; NOT_ELIGIBLE; NO_ACCEPTED_STEP; LOST_INLIERS
    int32_t accepted_after_rejected;  // accepted steps that directly follow a rejected one
    int32_t depth_rejected;           // steps rejected although their cost was finite and lower: an observation lost its depth
    double lambda;                    // the final damping
    double cost;                      // c at the final pose of the loop (whether or not it stands)
};

MSFM_FHD bool succeeded(const msfm_point3d& r) {
    const int want = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | MSFM_TRI_ERROR_OK | MSFM_TRI_ANGLE_OK;
    return (r.status & want) == want;
}

// ---- one lane's share of the three passes over an image's list (cu, cw, cX, cY, cZ: n entries) ------------------------------------
// partial j of the cost; *depth: every entry of the partial has Y.z > kDepthEps
MSFM_FHD double lane_cost(const double R[9], const double t[3], const double* cu, const double* cw, const double* cX, const double* cY,
                          const double* cZ, int n, int j, double f, bool* depth) {
    double c = 0.0;
    bool d = true;
    for (int i = j; i < n; i += kLanes) {
        const double X = cX[i], Y = cY[i], Z = cZ[i];
        const double Y0 = R[0] * X + R[1] * Y + R[2] * Z + t[0];
        const double Y1 = R[3] * X + R[4] * Y + R[5] * Z + t[1];
        const double Y2 = R[6] * X + R[7] * Y + R[8] * Z + t[2];
        d = d && Y2 > msfm_pose::kDepthEps;
        const double rx = (Y0 / Y2 - cu[i]) * f, ry = (Y1 / Y2 - cw[i]) * f;
        c = c + rx * rx;
        c = c + ry * ry;
    }
    *depth = d;
    return c;
}

// partial j of the 27 sums
MSFM_FHD void lane_sums(const double R[9], const double t[3], const double* cu, const double* cw, const double* cX, const double* cY,
                        const double* cZ, int n, int j, double acc[msfm_reg::kRegSums]) {
MSFM_UNROLL
    for (int k = 0; k < msfm_reg::kRegSums; ++k) acc[k] = 0.0;
    for (int i = j; i < n; i += kLanes) msfm_reg::gn_add(R, t, cu[i], cw[i], cX[i], cY[i], cZ[i], acc);
}

// the entries of partial j with positive depth and err <= max_error
MSFM_FHD int lane_inliers(const double R[9], const double t[3], const double* cu, const double* cw, const double* cX, const double* cY,
                          const double* cZ, int n, int j, double f, double max_error) {
    int c = 0;
    for (int i = j; i < n; i += kLanes) {
        const double X[3] = {cX[i], cY[i], cZ[i]};
        c += msfm_tri::obs_inlier(R, t, cu[i], cw[i], X, f, max_error) ? 1 : 0;
    }
    return c;
}

// gn_step's Cholesky with the damped diagonal: (H + lambda diag H) x = -g from the 27 sums, the new pose in Rn, tn.  False: no step.
MSFM_FHD bool lm_step(const double acc[msfm_reg::kRegSums], double lambda, const double R[9], const double t[3], double Rn[9], double tn[3],
                      double x[6]) {
    double L[6][6];
    int at = 0;
MSFM_UNROLL
    for (int r = 0; r < 6; ++r)
MSFM_UNROLL
        for (int c = r; c < 6; ++c) {
            L[c][r] = c == r ? acc[at] + lambda * acc[at] : acc[at];   // lower triangle
            ++at;
        }
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
        double s = -acc[21 + k];
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
    if (!ok) return false;
    const double a0 = x[0], a1 = x[1], a2 = x[2];
    const double aa = a0 * a0 + a1 * a1 + a2 * a2, inv = 1.0 / (1.0 + aa), dg = 1.0 - aa;
    const double C[9] = {(dg + 2.0 * a0 * a0) * inv,       (2.0 * a0 * a1 - 2.0 * a2) * inv, (2.0 * a0 * a2 + 2.0 * a1) * inv,
                         (2.0 * a0 * a1 + 2.0 * a2) * inv, (dg + 2.0 * a1 * a1) * inv,       (2.0 * a1 * a2 - 2.0 * a0) * inv,
                         (2.0 * a0 * a2 - 2.0 * a1) * inv, (2.0 * a1 * a2 + 2.0 * a0) * inv, (dg + 2.0 * a2 * a2) * inv};
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

// One eligible image.  `ev` owns the image's list and gives the three REDUCED passes, the same bits wherever it runs:
//   ev.cost(R, t, &depth) -> c(R, t), depth: every entry has Y.z > kDepthEps;   ev.sums(R, t, acc) -> the 27 sums;
//   ev.inliers(R, t) -> the standing rule's count.
// (R, t): read, and rewritten iff the refined pose stands.  res is always filled; trace may be null and changes nothing.
template <class E>
MSFM_FHD void refine_image(const E& ev, const Params& prm, double R[9], double t[3], Result* res, Trace* trace) {
    using namespace msfm_ref;
    double Rc[9], tc[3];
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) Rc[k] = R[k];
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) tc[k] = t[k];
    bool depth;
    double c = ev.cost(Rc, tc, &depth);
    const double c0 = c;
    double lambda = kLambda0, acc[msfm_reg::kRegSums];
    bool fresh = false, last_rejected = false;
    int steps = 0, accepted = 0, stop = STOP_MAX_ITERS, after_rejected = 0, depth_rejected = 0;
    while (steps < prm.max_iters) {
        if (!fresh) {
            ev.sums(Rc, tc, acc);
            fresh = true;
        }
        steps += 1;
        double Rn[9], tn[3], x[6];
        bool accept = lm_step(acc, lambda, Rc, tc, Rn, tn, x);
        if (accept) {
            bool dn;
            const double cn = ev.cost(Rn, tn, &dn);
            const bool lower = msfm_pose::finite(cn) && cn < c;
            depth_rejected += (lower && !dn) ? 1 : 0;
            accept = lower && dn;
            if (accept) c = cn;
        }
        if (accept) {
MSFM_UNROLL
            for (int k = 0; k < 9; ++k) Rc[k] = Rn[k];
MSFM_UNROLL
            for (int k = 0; k < 3; ++k) tc[k] = tn[k];
            fresh = false;
            accepted += 1;
            after_rejected += last_rejected ? 1 : 0;
            last_rejected = false;
            lambda = lambda / 10.0;
            if (lambda < kLambdaFloor) lambda = kLambdaFloor;
            const double d2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] + x[4] * x[4] + x[5] * x[5];
            const double t2 = tc[0] * tc[0] + tc[1] * tc[1] + tc[2] * tc[2];
            if (d2 <= prm.step_tol * prm.step_tol * (1.0 + t2)) {
                stop = STOP_STEP;
                break;
            }
        } else {
            last_rejected = true;
            lambda = lambda * 10.0;
            if (lambda > kLambdaCeiling) {
                stop = STOP_CEILING;
                break;
            }
        }
    }
    const int before = ev.inliers(R, t);
    const int after = accepted > 0 ? ev.inliers(Rc, tc) : before;
    const bool stands = accepted > 0 && after >= before;
    res->stands = stands ? 1 : 0;
    res->iterations = steps;
    res->stop = stop;
    res->inliers_before = before;
    res->inliers_after = after;
    res->accepted = accepted;
    res->cost_before = c0;
    res->cost_after = stands ? c : c0;
    if (trace) *trace = Trace{steps, accepted, stop, stands ? 0 : (accepted > 0 ? LOST_INLIERS : NO_ACCEPTED_STEP), after_rejected, depth_rejected, lambda, c};
    if (stands) {
MSFM_UNROLL
        for (int k = 0; k < 9; ++k) R[k] = Rc[k];
MSFM_UNROLL
        for (int k = 0; k < 3; ++k) t[k] = tc[k];
    }
}

// the record of a listed image before anything is known about it
MSFM_FHD void clear_record(msfm_pose_refinement* r, int image_id) {
    r->image_id = image_id;
    r->status = 0;
    r->n_observations = 0;
    r->iterations = 0;
    r->stop = msfm_ref::STOP_NONE;
    r->inliers_before = 0;
    r->inliers_after = 0;
    r->reserved = 0;
    r->cost_before = 0.0;
    r->cost_after = 0.0;
}

MSFM_FHD void fill_record(msfm_pose_refinement* r, const Result& res) {
    r->status |= MSFM_POSE_ATTEMPTED | (res.stands ? MSFM_POSE_REFINED : 0);
    r->iterations = res.iterations;
    r->stop = res.stop;
    r->inliers_before = res.inliers_before;
    r->inliers_after = res.inliers_after;
    r->cost_before = res.cost_before;
    r->cost_after = res.cost_after;
}

// One eligible track with an observation in an image whose pose changed: obs, residuals: its n element-aligned slots; poses: the NEW
// table; rec: read and rewritten.  The verdict block of msfm_ref::refine_track at the record's X.
MSFM_FHD void reverdict_track(const msfm_ref::Obs* obs, int n, const msfm_tri::Pose* poses, double f, const msfm_ref::Verdict& vd,
                              msfm_point3d* rec, double* residuals, Tally* tally) {
    using namespace msfm_ref;
    const msfm_point3d old = *rec;
    const double X[3] = {old.X[0], old.X[1], old.X[2]};
    bool error_ok = true, depth_ok = true;
    double sum = 0.0;
    int count = 0;
    for (int k = 0; k < n; ++k) {
        const Obs o = obs[k];
        if (!(o.flags & OBS_USED)) continue;
        const msfm_tri::Pose* p = poses + o.rank;
        bool d;
        const double err = msfm_tri::obs_error(p->R, p->t, o.u, o.w, X, f, &d);
        residuals[k] = err;
        if (!(o.flags & OBS_FIT)) continue;
        depth_ok = depth_ok && d;
        error_ok = error_ok && err <= vd.max_error;   // (false for a NaN)
        sum = sum + err;
        count += 1;
    }
    bool angle_ok = false;
    double angle = 0.0;
    for (int i = 1; i < n && !angle_ok; ++i) {
        const Obs oi = obs[i];
        if (!(oi.flags & OBS_FIT)) continue;
        const msfm_tri::Pose* pi = poses + oi.rank;
        const double Oi[3] = {pi->O[0], pi->O[1], pi->O[2]};
        for (int j = 0; j < i; ++j) {
            const Obs oj = obs[j];
            if (!(oj.flags & OBS_FIT)) continue;
            const msfm_tri::Pose* pj = poses + oj.rank;
            const double Oj[3] = {pj->O[0], pj->O[1], pj->O[2]};
            const double a = msfm_tri::parallax(X, Oi, Oj);
            if (a >= vd.min_angle) {
                angle = a;
                angle_ok = true;
                break;
            }
            if (a > angle) angle = a;
        }
    }
    msfm_point3d r = old;
    r.status = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | (error_ok ? MSFM_TRI_ERROR_OK : 0) | (angle_ok ? MSFM_TRI_ANGLE_OK : 0) |
               (depth_ok ? MSFM_TRI_DEPTH_OK : 0) | (old.status & (MSFM_TRI_ROBUST | MSFM_TRI_REFINED)) | MSFM_TRI_REPOSED;
    r.mean_residual = sum / (double)count;
    r.tri_angle = angle;
    *rec = r;
    tally->reposed = 1;
    tally->lost = (succeeded(old) && !succeeded(r)) ? 1 : 0;
    tally->gained = (!succeeded(old) && succeeded(r)) ? 1 : 0;
}

// does the track have a USED observation in an image whose pose changed (changed: one byte per pose rank)
MSFM_FHD bool touches_changed(const msfm_ref::Obs* obs, int n, const unsigned char* changed) {
    for (int k = 0; k < n; ++k) {
        const msfm_ref::Obs o = obs[k];
        if ((o.flags & msfm_ref::OBS_USED) && changed[o.rank]) return true;
    }
    return false;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: RefinePoses over the outputs of TriangulateTracks / TriangulateTracksRobust / RefinePoints -----------------------
struct Counts {
    long long images, eligible, refined, rejected_by_inliers, iterations, observations, points_reposed, points_lost, points_gained;
    double cost_before, cost_after;   // the records' costs summed in list order
};

// the three reduced passes over one image's list: 64 partials, then the butterfly
struct HostEval {
    const double *cu, *cw, *cX, *cY, *cZ;
    int n;
    double f, max_error;
    static void butterfly(double v[kLanes]) {
        for (int s = kLanes / 2; s >= 1; s >>= 1) {
            double nxt[kLanes];
            for (int j = 0; j < kLanes; ++j) nxt[j] = v[j] + v[j ^ s];
            for (int j = 0; j < kLanes; ++j) v[j] = nxt[j];
        }
    }
    double cost(const double R[9], const double t[3], bool* depth) const {
        double v[kLanes];
        bool all = true;
        for (int j = 0; j < kLanes; ++j) {
            bool d;
            v[j] = lane_cost(R, t, cu, cw, cX, cY, cZ, n, j, f, &d);
            all = all && d;
        }
        butterfly(v);
        *depth = all;
        return v[0];
    }
    void sums(const double R[9], const double t[3], double acc[msfm_reg::kRegSums]) const {
        double part[kLanes][msfm_reg::kRegSums];
        for (int j = 0; j < kLanes; ++j) lane_sums(R, t, cu, cw, cX, cY, cZ, n, j, part[j]);
        for (int k = 0; k < msfm_reg::kRegSums; ++k) {
            double v[kLanes];
            for (int j = 0; j < kLanes; ++j) v[j] = part[j][k];
            butterfly(v);
            acc[k] = v[0];
        }
    }
    int inliers(const double R[9], const double t[3]) const {
        int c = 0;
        for (int j = 0; j < kLanes; ++j) c += lane_inliers(R, t, cu, cw, cX, cY, cZ, n, j, f, max_error);
        return c;
    }
};

// tracks, rank_of_id, kxy, mask as RefinePoints takes them; poses: the table by rank, REWRITTEN where a refined pose stands;
// list_rank / list_ids: the pose list's images in its order (rank -1 never occurs: the list's images are declared); fixed: one byte per
// rank; points / residuals: read, and rewritten by the re-verdict.  records: one per listed image; changed: one byte per rank (output);
// `counts` (may be null) is added to; out_trace (may be null): one Trace per listed image.
inline void RefinePoses(const int64_t* offsets, const int32_t* image_ids, const int32_t* point_idx, int64_t n_tracks, const int* rank_of_id,
                        const float* const* kxy, msfm_tri::Pose* poses, int n_ranks, const uint8_t* mask, const msfm_emat::Camera& cam,
                        const msfm_ref::Verdict& vd, const Params& prm, const int* list_rank, const int32_t* list_ids, int n_list,
                        const uint8_t* fixed, msfm_point3d* points, double* residuals, msfm_pose_refinement* records, uint8_t* changed,
                        Counts* counts, Trace* out_trace = nullptr) {
    const double f = (cam.fx + cam.fy) / 2.0;
    const int64_t O = offsets[n_tracks];
    std::vector<msfm_ref::Obs> obs((size_t)std::max<int64_t>(O, 1));
    for (int64_t t = 0; t < n_tracks; ++t) {
        const int64_t b = offsets[t], e = offsets[t + 1];
        const msfm_tri::HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
        for (int k = 0; k < (int)(e - b); ++k) {
            const msfm_tri::Pose* p = a.pose(k);
            double x = 0.0, y = 0.0;
            if (p) a.pixel(k, &x, &y);
            msfm_ref::prepare_obs(p, p ? (int)(p - poses) : -1, x, y, mask ? mask[b + k] != 0 : true, cam, &obs[(size_t)(b + k)]);
        }
    }
    // the image-major lists: per rank, by ascending track number
    std::vector<char> candidate((size_t)std::max(n_ranks, 1), 0);
    for (int k = 0; k < n_list; ++k) candidate[(size_t)list_rank[k]] = poses[list_rank[k]].valid && !fixed[list_rank[k]];
    std::vector<std::vector<double>> cu((size_t)std::max(n_ranks, 1)), cw(cu.size()), cX(cu.size()), cY(cu.size()), cZ(cu.size());
    for (int64_t t = 0; t < n_tracks; ++t) {
        if (!succeeded(points[t])) continue;
        for (int64_t e = offsets[t]; e < offsets[t + 1]; ++e) {
            const msfm_ref::Obs o = obs[(size_t)e];
            if (!(o.flags & msfm_ref::OBS_FIT) || !candidate[(size_t)o.rank]) continue;
            cu[(size_t)o.rank].push_back(o.u);
            cw[(size_t)o.rank].push_back(o.w);
            cX[(size_t)o.rank].push_back(points[t].X[0]);
            cY[(size_t)o.rank].push_back(points[t].X[1]);
            cZ[(size_t)o.rank].push_back(points[t].X[2]);
        }
    }
    for (int r = 0; r < n_ranks; ++r) changed[r] = 0;
    Counts c = {n_list, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0};
    for (int k = 0; k < n_list; ++k) {
        const int r = list_rank[k];
        msfm_pose_refinement rec;
        clear_record(&rec, list_ids[k]);
        if (fixed[r]) rec.status = MSFM_POSE_FIXED;
        if (out_trace) out_trace[k] = Trace{0, 0, msfm_ref::STOP_NONE, NOT_ELIGIBLE, 0, 0, 0.0, 0.0};
        if (candidate[(size_t)r]) {
            const int n = (int)cu[(size_t)r].size();
            rec.n_observations = n;
            c.observations += n;
            if (n >= prm.min_observations) {
                const HostEval ev{cu[(size_t)r].data(), cw[(size_t)r].data(), cX[(size_t)r].data(), cY[(size_t)r].data(), cZ[(size_t)r].data(),
                                  n, f, vd.max_error};
                Result res;
                refine_image(ev, prm, poses[r].R, poses[r].t, &res, out_trace ? out_trace + k : nullptr);
                fill_record(&rec, res);
                if (res.stands) {
                    msfm_tri::centre(poses[r].R, poses[r].t, poses[r].O);
                    changed[r] = 1;
                }
                c.eligible += 1;
                c.refined += res.stands;
                c.rejected_by_inliers += (res.accepted > 0 && !res.stands) ? 1 : 0;
                c.iterations += res.iterations;
            }
        }
        c.cost_before = c.cost_before + rec.cost_before;
        c.cost_after = c.cost_after + rec.cost_after;
        records[k] = rec;
    }
    for (int64_t t = 0; t < n_tracks; ++t) {
        if (!msfm_ref::eligible(points[t])) continue;
        const int64_t b = offsets[t];
        const int n = (int)(offsets[t + 1] - b);
        if (!touches_changed(obs.data() + b, n, changed)) continue;
        Tally tl;
        reverdict_track(obs.data() + b, n, poses, f, vd, points + t, residuals + b, &tl);
        c.points_reposed += tl.reposed;
        c.points_lost += tl.lost;
        c.points_gained += tl.gained;
    }
    if (counts) {
        counts->images += c.images;
        counts->eligible += c.eligible;
        counts->refined += c.refined;
        counts->rejected_by_inliers += c.rejected_by_inliers;
        counts->iterations += c.iterations;
        counts->observations += c.observations;
        counts->points_reposed += c.points_reposed;
        counts->points_lost += c.points_lost;
        counts->points_gained += c.points_gained;
        counts->cost_before += c.cost_before;
        counts->cost_after += c.cost_after;
    }
}
#endif

}  // namespace msfm_rp
