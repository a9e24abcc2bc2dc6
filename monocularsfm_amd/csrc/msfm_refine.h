// msfm_refine.h -- point refinement arithmetic shared by the device kernels (msfm_refine.hip.h, hipcc) and the host twin
// (host/HostTestApi.cpp, RefinePoints, g++): every triangulated point is moved to the minimum of its reprojection error under FIXED
// poses by Levenberg-Marquardt, one 3 x 3 system per point.  Poses, tracks and inlier bytes never change.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides, every
// sum in observation order -> the host twin and the device produce the SAME bits.  Pose, parallax_scan, transform, obs_error are
// msfm_triangulate.h's, undistort is msfm_emat.h's, kDepthEps is msfm_pose.h's.
//
//   observations    one Obs per kept observation, aligned with the track CSR (prepare_obs): the undistorted (u, v) of
//                   msfm_triangulate.h, the rank of the image's pose, USED (the image has a valid pose) and FIT (USED, and the inlier
//                   byte is 1 where the points are a robust call's).  An unposed element: rank -1, flags 0.
//   eligible        a track whose record has ATTEMPTED | POINT.  Its FITTING SET is its FIT observations (>= 2 by construction).
//   cost            c(X) = sum over the fitting set, in observation order from 0.0, of rx^2 + ry^2 with
//                   Y = R X + t,  rx = (Y.x / Y.z - u) f,  ry = (Y.y / Y.z - v) f,  f = (fx + fy) / 2  (pixels).
//   normal system   per fitting observation the 2 x 3 Jacobian  J = (f / Y.z) [[1, 0, -x], [0, 1, -y]] R  (x = Y.x / Y.z, y = Y.y / Y.z);
//                   H += J^T J (upper triangle, the row of rx before the row of ry), g += J^T r, in observation order from 0.0.
//   step            A = H + lambda diag(H);  A = L L^T by a 3 x 3 Cholesky;  L y = -g;  L^T delta = y.  A pivot that is not > 0 or a
//                   non-finite delta: the step is rejected without a cost evaluation.
//   LM              lm_minimise below over PointProblem:  lambda = kLambda0; c = c(X) at the record's X.  While fewer than max_iters
//                   steps have been evaluated:
//                     (H, g at X are recomputed only after X changed.)  One step is evaluated:  Xn = X + delta.
//                     ACCEPTED iff c(Xn) is finite, c(Xn) < c, and every fitting view has Y.z > kDepthEps at Xn:
//                       X = Xn, c = c(Xn), lambda = max(lambda / 10, kLambdaFloor);
//                       stop (STEP) iff |delta|^2 <= step_tol^2 (|X|^2 + step_tol), X the new point.
//                     REJECTED otherwise:  lambda = 10 lambda;  stop (CEILING) iff lambda > kLambdaCeiling.
//                   Leaving the loop at max_iters evaluated steps: MAX_ITERS (also for max_iters = 0).
//   verdict         nothing accepted: the record stays.  Otherwise, at the final X with the thresholds of the triangulation that made
//                   the points: err (obs_error) of every USED observation; over the fitting set, in observation order: the errors'
//                   sum, ERROR_OK iff every err <= max_error (a NaN fails), DEPTH_OK iff every Y.z > kDepthEps, ANGLE_OK and the
//                   angle by msfm_tri::parallax_scan over the fitting set (point_verdict below).  The refined point STANDS iff none
//                   of ERROR_OK, ANGLE_OK, DEPTH_OK that the record had is cleared (its cost is strictly lower: a step was accepted).
//   record          stands: X, mean_residual = sum / |fitting set|, tri_angle, status = ATTEMPTED | POINT | the three bits | the
//                   record's ROBUST bit | REFINED; the residual slot of every USED observation gets its new error.  n_views and the
//                   slots of unposed elements are not written.  Does not stand: nothing is written.
#pragma once

#include "msfm_triangulate.h"

namespace msfm_ref {

constexpr double kLambda0 = 1e-3;         // the starting damping
constexpr double kLambdaFloor = 1e-12;    // accepted steps do not lower it further
constexpr double kLambdaCeiling = 1e4;    // a rejected step that raises it past this ends the track

enum { OBS_USED = 1, OBS_FIT = 2 };
enum { STOP_NONE = 0, STOP_STEP = 1, STOP_MAX_ITERS = 2, STOP_CEILING = 3 };
// why a result did not stand (Trace::verdict): 0 = it stands; the three status bits mean "this bit would have been cleared"
enum { NOT_ELIGIBLE = 1, NO_ACCEPTED_STEP = 2 };

struct Obs {   // 24 bytes
    double u, w;
    int32_t rank, flags;
};

struct Params {
    double step_tol;
    int32_t max_iters, reserved;
};

// the thresholds the verdict is recomputed with: those of the triangulation call that made the points
struct Verdict {
    double max_error, min_angle;
};

// what one track adds to the call's statistics
struct Tally {
    int32_t eligible, refined, gained_error_ok, rejected_by_verdict, iterations;
    double cost_before, cost_after;
};

// The route one track took: host only (the device passes nullptr).  Six int32 and two doubles, 40 bytes.
struct Trace {
    int32_t steps;                    // evaluated steps
    int32_t accepted;                 // ... of which accepted
    int32_t stop;                     // STOP_*
    int32_t verdict;                  // 0: stands; NOT_ELIGIBLE; NO_ACCEPTED_STEP; else the status bits that would have been cleared
    int32_t accepted_after_rejected;  // accepted steps that directly follow a rejected one
    int32_t depth_rejected;           // steps rejected although their cost was finite and lower: a fitting view lost its depth
    double lambda;                    // the final damping
    double cost;                      // c at the final X of the loop (whether or not the result stands)
};

MSFM_FHD bool eligible(const msfm_point3d& r) {
    const int need = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT;
    return (r.status & need) == need;
}

// one kept observation -> its Obs.  p: the pose of the element's image (nullptr: none), rank: its index in the pose table,
// (x, y): the keypoint's pixel (read for posed elements only), inlier: the robust call's byte (1 after the plain call)
MSFM_FHD void prepare_obs(const msfm_tri::Pose* p, int rank, double x, double y, bool inlier, const msfm_emat::Camera& cam, Obs* out) {
    Obs o = {0.0, 0.0, -1, 0};
    if (p) {
        msfm_emat::undistort(cam, x, y, &o.u, &o.w);
        o.rank = rank;
        o.flags = OBS_USED | (inlier ? OBS_FIT : 0);
    }
    *out = o;
}

// c(X) over the fitting set; *depth: every fitting view has X in front of it
MSFM_FHD double cost(const Obs* obs, int n, const msfm_tri::Pose* poses, double f, const double X[3], bool* depth) {
    double c = 0.0;
    bool d = true;
    for (int k = 0; k < n; ++k) {
        const Obs o = obs[k];
        if (!(o.flags & OBS_FIT)) continue;
        const msfm_tri::Pose* p = poses + o.rank;
        double Y[3];
        msfm_tri::transform(p->R, p->t, X, Y);
        d = d && Y[2] > msfm_pose::kDepthEps;
        const double rx = (Y[0] / Y[2] - o.u) * f, ry = (Y[1] / Y[2] - o.w) * f;
        c = c + rx * rx;
        c = c + ry * ry;
    }
    *depth = d;
    return c;
}

// H (upper triangle: 00 01 02 11 12 22) and g at X over the fitting set
MSFM_FHD void normal_system(const Obs* obs, int n, const msfm_tri::Pose* poses, double f, const double X[3], double H[6], double g[3]) {
    double h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (int k = 0; k < n; ++k) {
        const Obs o = obs[k];
        if (!(o.flags & OBS_FIT)) continue;
        const msfm_tri::Pose* p = poses + o.rank;
        double Y[3];
        msfm_tri::transform(p->R, p->t, X, Y);
        const double x = Y[0] / Y[2], y = Y[1] / Y[2], s = f / Y[2];
        const double rx = (x - o.u) * f, ry = (y - o.w) * f;
        const double a0 = (p->R[0] - x * p->R[6]) * s, a1 = (p->R[1] - x * p->R[7]) * s, a2 = (p->R[2] - x * p->R[8]) * s;
        const double b0 = (p->R[3] - y * p->R[6]) * s, b1 = (p->R[4] - y * p->R[7]) * s, b2 = (p->R[5] - y * p->R[8]) * s;
        h00 = h00 + a0 * a0;
        h00 = h00 + b0 * b0;
        h01 = h01 + a0 * a1;
        h01 = h01 + b0 * b1;
        h02 = h02 + a0 * a2;
        h02 = h02 + b0 * b2;
        h11 = h11 + a1 * a1;
        h11 = h11 + b1 * b1;
        h12 = h12 + a1 * a2;
        h12 = h12 + b1 * b2;
        h22 = h22 + a2 * a2;
        h22 = h22 + b2 * b2;
        g0 = g0 + a0 * rx;
        g0 = g0 + b0 * ry;
        g1 = g1 + a1 * rx;
        g1 = g1 + b1 * ry;
        g2 = g2 + a2 * rx;
        g2 = g2 + b2 * ry;
    }
    H[0] = h00;
    H[1] = h01;
    H[2] = h02;
    H[3] = h11;
    H[4] = h12;
    H[5] = h22;
    g[0] = g0;
    g[1] = g1;
    g[2] = g2;
}

// (H + lambda diag H) delta = -g by Cholesky.  False: a pivot is not > 0 or delta is not finite.
MSFM_FHD bool solve_step(const double H[6], const double g[3], double lambda, double delta[3]) {
    const double a00 = H[0] + lambda * H[0], a11 = H[3] + lambda * H[3], a22 = H[5] + lambda * H[5];
    if (!(a00 > 0.0)) return false;
    const double l00 = sqrt(a00);
    const double l10 = H[1] / l00, l20 = H[2] / l00;
    const double d1 = a11 - l10 * l10;
    if (!(d1 > 0.0)) return false;
    const double l11 = sqrt(d1);
    const double l21 = (H[4] - l20 * l10) / l11;
    const double d2 = a22 - l20 * l20 - l21 * l21;
    if (!(d2 > 0.0)) return false;
    const double l22 = sqrt(d2);
    const double y0 = -g[0] / l00;
    const double y1 = (-g[1] - l10 * y0) / l11;
    const double y2 = (-g[2] - l20 * y0 - l21 * y1) / l22;
    const double z2 = y2 / l22;
    const double z1 = (y1 - l21 * z2) / l11;
    const double z0 = (y0 - l10 * z1 - l20 * z2) / l00;
    delta[0] = z0;
    delta[1] = z1;
    delta[2] = z2;
    return msfm_pose::finite(z0) && msfm_pose::finite(z1) && msfm_pose::finite(z2);
}

// ---- the Levenberg-Marquardt loop (the LM paragraphs above and of msfm_refine_poses.h) ------------------------------------------------
// What one run leaves; the two trace counters are dead code where nobody reads them.
struct LmRun {
    int32_t steps, accepted, stop, accepted_after_rejected, depth_rejected;
    double lambda, cost_before, cost;   // the final damping, c at the start, c at the final state
};

// `pb` is the problem:  typename P::State (copyable), typename P::System;
//   pb.cost(s, &depth) -> c at the state s, depth: every fitting view has Y.z > kDepthEps;
//   pb.linearise(s, &sys): the normal system at s;
//   pb.step(sys, lambda, s, &sn, &d2) -> the damped step from s to the candidate sn, d2 = |delta|^2; false: no step;
//   pb.stop_scale(s): an accepted step ends the run (STEP) iff d2 <= step_tol^2 stop_scale(s), s the new state.
// s: the start, and the final state of the loop.
template <class P>
MSFM_FHD void lm_minimise(const P& pb, int max_iters, double step_tol, typename P::State* s, LmRun* run) {
    bool depth;
    double c = pb.cost(*s, &depth);
    const double c0 = c;
    double lambda = kLambda0;
    typename P::System sys;
    bool fresh = false, last_rejected = false;
    int steps = 0, accepted = 0, stop = STOP_MAX_ITERS, after_rejected = 0, depth_rejected = 0;
    while (steps < max_iters) {
        if (!fresh) {
            pb.linearise(*s, &sys);
            fresh = true;
        }
        steps += 1;
        typename P::State sn;
        double d2;
        bool accept = pb.step(sys, lambda, *s, &sn, &d2);
        if (accept) {
            bool dn;
            const double cn = pb.cost(sn, &dn);
            const bool lower = msfm_pose::finite(cn) && cn < c;
            depth_rejected += (lower && !dn) ? 1 : 0;
            accept = lower && dn;
            if (accept) c = cn;
        }
        if (accept) {
            *s = sn;
            fresh = false;
            accepted += 1;
            after_rejected += last_rejected ? 1 : 0;
            last_rejected = false;
            lambda = lambda / 10.0;
            if (lambda < kLambdaFloor) lambda = kLambdaFloor;
            if (d2 <= step_tol * step_tol * pb.stop_scale(*s)) {
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
    *run = LmRun{steps, accepted, stop, after_rejected, depth_rejected, lambda, c0, c};
}

MSFM_FHD void trace_of(const LmRun& run, int verdict, Trace* trace) {
    *trace = Trace{run.steps, run.accepted, run.stop, verdict, run.accepted_after_rejected, run.depth_rejected, run.lambda, run.cost};
}

// one point under fixed poses: the 3 x 3 problem of lm_minimise
struct PointProblem {
    struct State {
        double X[3];
    };
    struct System {
        double H[6], g[3];
    };
    const Obs* obs;
    int n;
    const msfm_tri::Pose* poses;
    double f, step_tol;
    MSFM_FHD double cost(const State& s, bool* depth) const { return msfm_ref::cost(obs, n, poses, f, s.X, depth); }
    MSFM_FHD void linearise(const State& s, System* sys) const { normal_system(obs, n, poses, f, s.X, sys->H, sys->g); }
    MSFM_FHD bool step(const System& sys, double lambda, const State& s, State* sn, double* d2) const {
        double delta[3];
        if (!solve_step(sys.H, sys.g, lambda, delta)) return false;
        sn->X[0] = s.X[0] + delta[0];
        sn->X[1] = s.X[1] + delta[1];
        sn->X[2] = s.X[2] + delta[2];
        *d2 = delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2];
        return true;
    }
    MSFM_FHD double stop_scale(const State& s) const { return (s.X[0] * s.X[0] + s.X[1] * s.X[1] + s.X[2] * s.X[2]) + step_tol; }
};

// ---- the verdict of a point at X over its Obs ----------------------------------------------------------------------------------------
struct PointVerdict {
    int32_t bits, count;   // ERROR_OK | ANGLE_OK | DEPTH_OK as they hold over the fitting set; |fitting set|
    double sum, angle;     // the fitting set's errors summed in observation order from 0.0; the parallax scan's angle
};

// err (obs_error) over the fitting set, in observation order: the sum, ERROR_OK iff every err <= max_error (a NaN fails), DEPTH_OK iff
// every Y.z > kDepthEps; ANGLE_OK and the angle by msfm_tri::parallax_scan over the fitting set.  Two modes, the same sums in both:
//   residuals != nullptr  the loop visits every USED observation, writes its error to its slot, and lets only the FIT ones (the second
//                         filter) into the sums: reverdict_track.
//   residuals == nullptr  the loop visits the FIT observations alone and NO slot is written: refine_track, which may not touch a slot
//                         before it knows that the point stands, and then writes the USED observations' errors in a loop of its own.
MSFM_FHD void point_verdict(const Obs* obs, int n, const msfm_tri::Pose* poses, double f, const Verdict& vd, const double X[3],
                            double* residuals, PointVerdict* out) {
    bool error_ok = true, depth_ok = true;
    double sum = 0.0;
    int count = 0;
    for (int k = 0; k < n; ++k) {
        const Obs o = obs[k];
        if (!(o.flags & (residuals ? OBS_USED : OBS_FIT))) continue;
        const msfm_tri::Pose* p = poses + o.rank;
        bool d;
        const double err = msfm_tri::obs_error(p->R, p->t, o.u, o.w, X, f, &d);
        if (residuals) residuals[k] = msfm_pose::canonical(err);
        if (!(o.flags & OBS_FIT)) continue;
        depth_ok = depth_ok && d;
        error_ok = error_ok && err <= vd.max_error;   // (false for a NaN)
        sum = sum + err;
        count += 1;
    }
    double angle;
    const bool angle_ok = msfm_tri::parallax_scan(X, n, vd.min_angle, [&](int k) -> const double* {
        const Obs o = obs[k];
        return (o.flags & OBS_FIT) ? poses[o.rank].O : nullptr;
    }, &angle);
    out->bits = (error_ok ? MSFM_TRI_ERROR_OK : 0) | (angle_ok ? MSFM_TRI_ANGLE_OK : 0) | (depth_ok ? MSFM_TRI_DEPTH_OK : 0);
    out->count = count;
    out->sum = sum;
    out->angle = angle;
}

// One track: obs, residuals: its n element-aligned slots; rec: its record (read, and rewritten iff the refined point stands).
// tally is always filled; trace may be null and changes nothing.
MSFM_FHD void refine_track(const Obs* obs, int n, const msfm_tri::Pose* poses, double f, const Verdict& vd, const Params& prm,
                           msfm_point3d* rec, double* residuals, Tally* tally, Trace* trace) {
    *tally = Tally{0, 0, 0, 0, 0, 0.0, 0.0};
    if (trace) *trace = Trace{0, 0, STOP_NONE, NOT_ELIGIBLE, 0, 0, 0.0, 0.0};
    const msfm_point3d old = *rec;
    if (!eligible(old)) return;
    const PointProblem pb{obs, n, poses, f, prm.step_tol};
    PointProblem::State s = {{old.X[0], old.X[1], old.X[2]}};
    LmRun run;
    lm_minimise(pb, prm.max_iters, prm.step_tol, &s, &run);
    tally->eligible = 1;
    tally->iterations = run.steps;
    tally->cost_before = run.cost_before;
    tally->cost_after = run.cost_before;
    if (trace) trace_of(run, NO_ACCEPTED_STEP, trace);
    if (run.accepted == 0) return;
    PointVerdict v;
    point_verdict(obs, n, poses, f, vd, s.X, nullptr, &v);
    const int cleared = old.status & ~v.bits & (MSFM_TRI_ERROR_OK | MSFM_TRI_ANGLE_OK | MSFM_TRI_DEPTH_OK);
    if (trace) trace->verdict = cleared;
    if (cleared) {
        tally->rejected_by_verdict = 1;
        return;
    }
    for (int k = 0; k < n; ++k) {
        const Obs o = obs[k];
        if (!(o.flags & OBS_USED)) continue;
        const msfm_tri::Pose* p = poses + o.rank;
        bool d;
        residuals[k] = msfm_pose::canonical(msfm_tri::obs_error(p->R, p->t, o.u, o.w, s.X, f, &d));
    }
    msfm_point3d r = old;
    r.status = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | v.bits | (old.status & MSFM_TRI_ROBUST) | MSFM_TRI_REFINED;
    r.X[0] = s.X[0];
    r.X[1] = s.X[1];
    r.X[2] = s.X[2];
    r.mean_residual = v.sum / (double)v.count;
    r.tri_angle = v.angle;
    *rec = r;
    tally->refined = 1;
    tally->gained_error_ok = ((v.bits & MSFM_TRI_ERROR_OK) && !(old.status & MSFM_TRI_ERROR_OK)) ? 1 : 0;
    tally->cost_after = run.cost;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: RefinePoints over the outputs of TriangulateTracks / TriangulateTracksRobust ---------------------------------
struct Counts {
    long long eligible, refined, gained_error_ok, rejected_by_verdict, iterations;
    double cost_before, cost_after;   // summed in track order
};

// the n Obs of one track: mask: the track's inlier bytes (element-aligned), or null = every byte 1
inline void host_obs(const msfm_tri::HostTrack& a, int n, const uint8_t* mask, const msfm_emat::Camera& cam, Obs* out) {
    for (int k = 0; k < n; ++k) {
        const msfm_tri::Pose* p = a.pose(k);
        double x = 0.0, y = 0.0;
        if (p) a.pixel(k, &x, &y);
        prepare_obs(p, p ? (int)(p - a.poses) : -1, x, y, mask ? mask[k] != 0 : true, cam, out + k);
    }
}

// tracks, rank_of_id, kxy, poses as TriangulateTracks takes them; mask: the robust call's inlier bytes, or null after the plain call;
// points / residuals: read and rewritten in place.  `counts` (may be null) is added to; out_trace (may be null): one Trace per track
// at the track's own position.
inline void RefinePoints(const int64_t* offsets, const int32_t* image_ids, const int32_t* point_idx, int64_t first_track, int64_t n_tracks,
                         const int* rank_of_id, const float* const* kxy, const msfm_tri::Pose* poses, const uint8_t* mask,
                         const msfm_emat::Camera& cam, const Verdict& vd, const Params& prm, msfm_point3d* points, double* residuals,
                         Counts* counts, Trace* out_trace = nullptr) {
    const double f = (cam.fx + cam.fy) / 2.0;
    std::vector<Obs> obs;
    for (int64_t t = first_track; t < first_track + n_tracks; ++t) {
        const int64_t b = offsets[t], e = offsets[t + 1];
        const int n = (int)(e - b);
        const msfm_tri::HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
        obs.resize((size_t)n);
        host_obs(a, n, mask ? mask + b : nullptr, cam, obs.data());
        Tally tl;
        refine_track(obs.data(), n, poses, f, vd, prm, points + t, residuals + b, &tl, out_trace ? out_trace + t : nullptr);
        if (counts) {
            counts->eligible += tl.eligible;
            counts->refined += tl.refined;
            counts->gained_error_ok += tl.gained_error_ok;
            counts->rejected_by_verdict += tl.rejected_by_verdict;
            counts->iterations += tl.iterations;
            counts->cost_before += tl.cost_before;
            counts->cost_after += tl.cost_after;
        }
    }
}
#endif

}  // namespace msfm_ref
