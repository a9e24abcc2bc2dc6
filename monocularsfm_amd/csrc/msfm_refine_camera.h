// msfm_refine_camera.h -- camera refinement arithmetic shared by the device kernels (msfm_refine_camera.hip.h, hipcc) and the host twin
// (host/HostTestApi.cpp, RefineCamera, g++): the session's ONE camera is moved to the minimum of the map's reprojection error under
// FIXED poses and FIXED points by Levenberg-Marquardt, one dense 6 x 6 system per call.  The third block of the
// block-coordinate scheme: msfm_refine.h is the point block, msfm_refine_poses.h the pose block, a caller alternates the three.
// Points' X, poses, tracks and inlier bytes never change.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides -> the host
// twin and the device produce the SAME bits.  Obs, prepare_obs, eligible, lm_minimise (the LM loop, its constants, STOP_*, Trace) and
// point_verdict are msfm_refine.h's, succeeded msfm_refine_poses.h's, cholesky6_solve msfm_register.h's, transform msfm_triangulate.h's,
// undistort msfm_emat.h's, kDepthEps msfm_pose.h's.
//
//   unknowns        x[0 .. 5] selected by `mask`:  MSFM_CAM_FX_FY: x[0] = dfx, x[1] = dfy;  MSFM_CAM_F (exclusive with FX_FY): x[0] = s
//                   with fx <- fx (1 + s), fy <- fy (1 + s);  MSFM_CAM_CX_CY: x[2] = dcx, x[3] = dcy;  MSFM_CAM_K1_K2: x[4] = dk1,
//                   x[5] = dk2.  p1 and p2 never move.  An unknown that is not selected has a zero Jacobian column; its H_ii is set to
//                   1, its g_i and off-diagonals to 0, so its delta is exactly +-0 and the system stays 6 x 6.
//   slot            one per kept observation in the tracks' CSR order, s = 0 .. O - 1 (prepare_slot).  A slot CONTRIBUTES iff its Obs is
//                   OBS_FIT, its track's record has ATTEMPTED | POINT | ERROR_OK | ANGLE_OK and Y.z > kDepthEps with Y = R X + t; it
//                   then holds the raw keypoint pixel (px, py) and the reprojection (qx, qy) = (Y.x / Y.z, Y.y / Y.z).  Neither depends
//                   on the camera: the contributing set is fixed for the whole call.  BEHIND: otherwise fitting, left out by depth.
//   cost            c(theta) = sum over the contributing slots of rx^2 + ry^2,  rx = (qx - u) f,  ry = (qy - w) f,  (u, w) =
//                   msfm_emat::undistort(theta; px, py),  f = (fx + fy) / 2: the cost of msfm_refine.h with the camera as the variable.
//   Jacobian        closed form, by the implicit function theorem on the Brown model  distort(u, w; k) = d(theta),
//                   d = ((px - cx) / fx, (py - cy) / fy):   d(u, w)/dtheta = A^-1 (dd/dtheta - ddistort/dtheta),  A = ddistort/d(u, w)
//                   (2 x 2, symmetric) evaluated at the undistorted point;  drx/dtheta = -f du/dtheta + (qx - u) df/dtheta.  This is
//                   the Jacobian of the EXACT inverse, not of undistort's 40 fixed-point steps (nor of its all-zero shortcut): the
//                   difference is far below the step, and the LM accepts a step only on the TRUE cost, strictly lower, so a slightly
//                   inexact Jacobian can cost an iteration and never a wrong result.
//   the 28 sums     21 upper entries of J^T J (row-major; per slot Jx_r Jx_c + Jy_r Jy_c, the rx row before the ry row), 6 of J^T r
//                   (Jx_r rx + Jy_r ry), and the cost (rx rx + ry ry).  A slot that does not contribute adds 0.0 to every sum.
//   summation       an order fixed by the DATA, never by the grid or the CU count (tree256 / the two levels):
//                     level 1  chunk c = slots 256 c .. 256 c + 255 (slots >= O are 0.0).  Inside each group of 64 consecutive slots
//                              v_j <- v_j + v_(j xor m) for m = 32, 16, .., 1 (the butterfly of msfm_refine_poses.h), which leaves
//                              w0 .. w3; the chunk's sum is ((w0 + w1) + w2) + w3.
//                     level 2  256 partials p_j = the sums of the chunks c = j, j + 256, j + 512, .. added in that order from 0.0;
//                              then the same 256-element tree over p.
//                   The standing rule's inlier count is an integer: its order does not matter.
//   step            (H + lambda diag H) delta = -g by msfm_reg::cholesky6_solve (cam_step).  A pivot that is not > 0, a non-finite delta
//                   or camera, or fx or fy not > 0: the step is rejected without a cost evaluation.  There are no box constraints:
//                   strict descent on the true cost and the standing rule are the protection.
//   LM              msfm_ref::lm_minimise over CameraProblem (lambda 1e-3, / 10 on accept with floor 1e-12, x 10 on reject, ceiling
//                   1e4).  ACCEPTED iff the cost is finite and strictly lower (depth cannot change: Y does not depend on the camera).
//                   stop (STEP) after an accepted step with  (dfx / fx)^2 + (dfy / fy)^2 + (dcx / f)^2 + (dcy / f)^2 + dk1^2 + dk2^2
//                   <= step_tol^2,  fx, fy, f of the NEW camera (under MSFM_CAM_F: dfx = fx s, dfy = fy s of the old one).
//   eligible        the call is attempted iff at least min_observations slots contribute (else stop = STOP_FEW) and the starting cost
//                   is finite (else STOP_NONFINITE: msfm_pose.h's NaN rule -- a non-finite keypoint makes the cost NaN and every
//                   comparison on it fails).  Otherwise nothing changes.
//   standing        the refined camera STANDS iff a step was accepted and the number of contributing slots with err <= max_error
//                   (err = sqrt((qx - u)^2 + (qy - w)^2) f: obs_error) is not lower under it than under the old camera: the rule of
//                   msfm_refine_poses.h over the whole map.  Otherwise nothing changes.
//   re-verdict      when it stands, EVERY track with ATTEMPTED | POINT at its unchanged X under the unchanged poses and the NEW camera
//                   (the Obs are prepared again: they hold the undistorted point): msfm_ref::point_verdict with the residual slots.
//                   status = ATTEMPTED | POINT | the three bits | the record's ROBUST, REFINED, REPOSED, EXTENDED, FILTERED, COMPLETED
//                   bits | RECALIBRATED; mean_residual, tri_angle and the residual slots of the USED observations are rewritten;
//                   n_views and X are kept.
#pragma once

#include "msfm_refine_poses.h"

namespace msfm_rc {

constexpr int kChunk = 256;   // slots per level-1 chunk = partials of level 2 = the workgroup of the kernels
constexpr int kWave = 64;
constexpr int kSums = 28;     // 21 of J^T J, 6 of J^T r, the cost
constexpr int kCost = 27;     // ... the cost's place
enum { SLOT_IN = 1, SLOT_BEHIND = 2 };
enum { STOP_FEW = 4, STOP_NONFINITE = 5 };                            // beside msfm_ref::STOP_*: why nothing was attempted
enum { NOT_ELIGIBLE = 1, NO_ACCEPTED_STEP = 2, LOST_INLIERS = 3 };   // why a camera did not stand (Trace::verdict); 0: it stands
constexpr int kKeptBits = MSFM_TRI_ROBUST | MSFM_TRI_REFINED | MSFM_TRI_REPOSED | MSFM_TRI_EXTENDED | MSFM_TRI_FILTERED | MSFM_TRI_COMPLETED;

struct Slot {   // 40 bytes
    double px, py, qx, qy;
    int32_t flags, pad;
};

struct Params {
    double step_tol;
    int32_t mask, max_iters, min_observations, reserved;
};

// what refine_camera leaves besides the camera
struct Result {
    int32_t stands, iterations, accepted, stop;
    long long inliers_before, inliers_after;
    double cost_before, cost_after;
};

// what one re-verdict adds to the call's statistics
struct Tally {
    int32_t recalibrated, lost, gained;
};

MSFM_FHD bool mask_ok(int mask) {
    return mask != 0 && (mask & ~15) == 0 && !((mask & MSFM_CAM_FX_FY) && (mask & MSFM_CAM_F));
}

// is unknown i selected
MSFM_FHD bool selected(int mask, int i) {
    return i == 0 ? (mask & (MSFM_CAM_FX_FY | MSFM_CAM_F)) != 0
         : i == 1 ? (mask & MSFM_CAM_FX_FY) != 0
         : i <= 3 ? (mask & MSFM_CAM_CX_CY) != 0
                  : (mask & MSFM_CAM_K1_K2) != 0;
}

// one kept observation -> its Slot.  o: its Obs; standing: its track's record has ATTEMPTED | POINT | ERROR_OK | ANGLE_OK; X: the record's
// point; (px, py): the keypoint's raw pixel (read for FIT observations of standing tracks only)
MSFM_FHD void prepare_slot(const msfm_ref::Obs& o, bool standing, const msfm_tri::Pose* poses, const double X[3], double px, double py,
                           Slot* out) {
    Slot s = {0.0, 0.0, 0.0, 0.0, 0, 0};
    if ((o.flags & msfm_ref::OBS_FIT) && standing) {
        const msfm_tri::Pose* p = poses + o.rank;
        double Y[3];
        msfm_tri::transform(p->R, p->t, X, Y);
        if (Y[2] > msfm_pose::kDepthEps) {   // (false for a NaN)
            s.px = px;
            s.py = py;
            s.qx = Y[0] / Y[2];
            s.qy = Y[1] / Y[2];
            s.flags = SLOT_IN;
        } else {
            s.flags = SLOT_BEHIND;
        }
    }
    *out = s;
}

// what slot s adds to the cost under camera c (0.0 if it does not contribute); *inlier: it contributes and err <= max_error
MSFM_FHD double slot_cost(const Slot& s, const msfm_emat::Camera& c, double max_error, int* inlier) {
    *inlier = 0;
    if (!(s.flags & SLOT_IN)) return 0.0;
    double u, w;
    msfm_emat::undistort(c, s.px, s.py, &u, &w);
    const double f = (c.fx + c.fy) / 2.0;
    const double dx = s.qx - u, dy = s.qy - w;
    const double rx = dx * f, ry = dy * f;
    const double err = sqrt(dx * dx + dy * dy) * f;   // (msfm_tri::obs_error)
    *inlier = err <= max_error ? 1 : 0;               // (false for a NaN)
    return rx * rx + ry * ry;
}

// what slot s adds to the 28 sums under camera c
MSFM_FHD void slot_sums(const Slot& s, const msfm_emat::Camera& c, int mask, double acc[kSums]) {
MSFM_UNROLL
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    if (!(s.flags & SLOT_IN)) return;
    double u, w;
    msfm_emat::undistort(c, s.px, s.py, &u, &w);
    const double f = (c.fx + c.fy) / 2.0;
    const double ex = s.qx - u, ey = s.qy - w;
    const double rx = ex * f, ry = ey * f;
    // A = ddistort/d(u, w) at (u, w), and its inverse
    const double r2 = u * u + w * w, r4 = r2 * r2;
    const double radial = 1.0 + (c.k2 * r2 + c.k1) * r2, dr = c.k1 + 2.0 * c.k2 * r2;
    const double a00 = radial + 2.0 * u * u * dr + 2.0 * c.p1 * w + 6.0 * c.p2 * u;
    const double a01 = 2.0 * u * w * dr + 2.0 * c.p1 * u + 2.0 * c.p2 * w;
    const double a11 = radial + 2.0 * w * w * dr + 6.0 * c.p1 * w + 2.0 * c.p2 * u;
    const double det = a00 * a11 - a01 * a01;
    const double i00 = a11 / det, i01 = -a01 / det, i11 = a00 / det;
    // b = dd/dtheta - ddistort/dtheta per parameter, (du, dw) = A^-1 b
    const double dx0 = (s.px - c.cx) / c.fx, dy0 = (s.py - c.cy) / c.fy;
    const double bfx = -dx0 / c.fx, bfy = -dy0 / c.fy, bcx = -1.0 / c.fx, bcy = -1.0 / c.fy;
    double du[6], dw[6], df[6];
    du[0] = i00 * bfx;
    dw[0] = i01 * bfx;
    du[1] = i01 * bfy;
    dw[1] = i11 * bfy;
    du[2] = i00 * bcx;
    dw[2] = i01 * bcx;
    du[3] = i01 * bcy;
    dw[3] = i11 * bcy;
    du[4] = i00 * (-r2 * u) + i01 * (-r2 * w);
    dw[4] = i01 * (-r2 * u) + i11 * (-r2 * w);
    du[5] = i00 * (-r4 * u) + i01 * (-r4 * w);
    dw[5] = i01 * (-r4 * u) + i11 * (-r4 * w);
    df[0] = 0.5;
    df[1] = 0.5;
    df[2] = df[3] = df[4] = df[5] = 0.0;
    if (mask & MSFM_CAM_F) {   // s: fx (1 + s), fy (1 + s) -> d/ds = fx d/dfx + fy d/dfy at s = 0
        du[0] = c.fx * du[0] + c.fy * du[1];
        dw[0] = c.fx * dw[0] + c.fy * dw[1];
        df[0] = f;
    }
    double jx[6], jy[6];
MSFM_UNROLL
    for (int i = 0; i < 6; ++i) {
        const bool sel = selected(mask, i);
        jx[i] = sel ? ex * df[i] - f * du[i] : 0.0;
        jy[i] = sel ? ey * df[i] - f * dw[i] : 0.0;
    }
    int at = 0;
MSFM_UNROLL
    for (int r = 0; r < 6; ++r)
MSFM_UNROLL
        for (int q = r; q < 6; ++q) {
            acc[at] = jx[r] * jx[q] + jy[r] * jy[q];
            ++at;
        }
MSFM_UNROLL
    for (int r = 0; r < 6; ++r) acc[21 + r] = jx[r] * rx + jy[r] * ry;
    acc[kCost] = rx * rx + ry * ry;
}

// (H + lambda diag H) x = -g from the 28 sums, unselected unknowns pinned, and the new camera.  False: no step.  *d2: the STEP test's
// left side, with the new camera.
MSFM_FHD bool cam_step(const double acc[kSums], int mask, double lambda, const msfm_emat::Camera& c, msfm_emat::Camera* cn, double* d2) {
    double L[6][6], g[6], x[6];
    int at = 0;
MSFM_UNROLL
    for (int r = 0; r < 6; ++r) {
MSFM_UNROLL
        for (int q = r; q < 6; ++q) {
            const bool both = selected(mask, r) && selected(mask, q);
            const double h = q == r ? (both ? acc[at] : 1.0) : (both ? acc[at] : 0.0);
            L[q][r] = q == r ? h + lambda * h : h;   // lower triangle
            ++at;
        }
        g[r] = selected(mask, r) ? acc[21 + r] : 0.0;
    }
    if (!msfm_reg::cholesky6_solve(L, g, x)) return false;
    msfm_emat::Camera n = c;
    double dfx, dfy;
    if (mask & MSFM_CAM_F) {
        dfx = c.fx * x[0];
        dfy = c.fy * x[0];
        n.fx = c.fx * (1.0 + x[0]);
        n.fy = c.fy * (1.0 + x[0]);
    } else {
        dfx = x[0];
        dfy = x[1];
        n.fx = c.fx + x[0];
        n.fy = c.fy + x[1];
    }
    n.cx = c.cx + x[2];
    n.cy = c.cy + x[3];
    n.k1 = c.k1 + x[4];
    n.k2 = c.k2 + x[5];
    if (!(msfm_pose::finite(n.fx) && msfm_pose::finite(n.fy) && msfm_pose::finite(n.cx) && msfm_pose::finite(n.cy) &&
          msfm_pose::finite(n.k1) && msfm_pose::finite(n.k2)))
        return false;
    if (!(n.fx > 0.0) || !(n.fy > 0.0)) return false;
    const double fn = (n.fx + n.fy) / 2.0;
    const double e0 = dfx / n.fx, e1 = dfy / n.fy, e2 = x[2] / fn, e3 = x[3] / fn;
    *d2 = e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3 + x[4] * x[4] + x[5] * x[5];
    *cn = n;
    return true;
}

// the camera under fixed poses and points: the 6 x 6 problem of msfm_ref::lm_minimise over the reduced passes of `ev`
template <class E>
struct CameraProblem {
    struct State {
        msfm_emat::Camera cam;
    };
    struct System {
        double acc[kSums];
    };
    const E& ev;
    int mask;
    double cost(const State& s, bool* depth) const {
        long long inliers;
        *depth = true;   // (Y does not depend on the camera: the contributing set keeps its depth)
        return ev.cost(s.cam, &inliers);
    }
    void linearise(const State& s, System* sys) const { ev.sums(s.cam, sys->acc); }
    bool step(const System& sys, double lambda, const State& s, State* sn, double* d2) const {
        return cam_step(sys.acc, mask, lambda, s.cam, &sn->cam, d2);
    }
    double stop_scale(const State&) const { return 1.0; }
};

// The whole call's decision.  `ev` owns the slots and gives the REDUCED passes, the same bits wherever it runs:
//   ev.contributing() -> the number of contributing slots;   ev.cost(cam, &inliers) -> c(cam) and the standing rule's count;
//   ev.sums(cam, acc) -> the 28 sums.
// The control flow and the 6 x 6 solve run on the host on both sides (the device side launches kernels behind ev).
// *cam: read, and rewritten iff the refined camera stands.  res is always filled; trace may be null and changes nothing.
template <class E>
void refine_camera(const E& ev, const Params& prm, msfm_emat::Camera* cam, Result* res, msfm_ref::Trace* trace) {
    *res = Result{0, 0, 0, msfm_ref::STOP_NONE, 0, 0, 0.0, 0.0};
    if (trace) *trace = msfm_ref::Trace{0, 0, msfm_ref::STOP_NONE, NOT_ELIGIBLE, 0, 0, 0.0, 0.0};
    int why = msfm_ref::STOP_NONE;
    long long before = 0;
    if (ev.contributing() < (long long)prm.min_observations) why = STOP_FEW;
    else if (!msfm_pose::finite(ev.cost(*cam, &before))) why = STOP_NONFINITE;
    if (why != msfm_ref::STOP_NONE) {
        res->stop = why;
        if (trace) trace->stop = why;
        return;
    }
    const CameraProblem<E> pb{ev, prm.mask};
    typename CameraProblem<E>::State s = {*cam};
    msfm_ref::LmRun run;
    msfm_ref::lm_minimise(pb, prm.max_iters, prm.step_tol, &s, &run);
    long long after = before;
    if (run.accepted > 0) (void)ev.cost(s.cam, &after);
    const bool stands = run.accepted > 0 && after >= before;
    res->stands = stands ? 1 : 0;
    res->iterations = run.steps;
    res->accepted = run.accepted;
    res->stop = run.stop;
    res->inliers_before = before;
    res->inliers_after = after;
    res->cost_before = run.cost_before;
    res->cost_after = stands ? run.cost : run.cost_before;
    if (trace) msfm_ref::trace_of(run, stands ? 0 : (run.accepted > 0 ? LOST_INLIERS : NO_ACCEPTED_STEP), trace);
    if (stands) *cam = s.cam;
}

// One eligible track after the camera changed: obs (prepared under the NEW camera), residuals: its n element-aligned slots; rec: read and
// rewritten.  msfm_ref::point_verdict at the record's X, the residual slots included.
MSFM_FHD void recalibrate_track(const msfm_ref::Obs* obs, int n, const msfm_tri::Pose* poses, double f, const msfm_ref::Verdict& vd,
                                msfm_point3d* rec, double* residuals, Tally* tally) {
    const msfm_point3d old = *rec;
    const double X[3] = {old.X[0], old.X[1], old.X[2]};
    msfm_ref::PointVerdict v;
    msfm_ref::point_verdict(obs, n, poses, f, vd, X, residuals, &v);
    msfm_point3d r = old;
    r.status = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | v.bits | (old.status & kKeptBits) | MSFM_TRI_RECALIBRATED;
    r.mean_residual = v.sum / (double)v.count;
    r.tri_angle = v.angle;
    *rec = r;
    tally->recalibrated = 1;
    tally->lost = (msfm_rp::succeeded(old) && !msfm_rp::succeeded(r)) ? 1 : 0;
    tally->gained = (!msfm_rp::succeeded(old) && msfm_rp::succeeded(r)) ? 1 : 0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: RefineCamera over the outputs of the triangulation, refinement, extension, filter and completion twins -----------
struct Counts {
    long long observations, behind, iterations, accepted_steps, stop, refined, rejected_by_inliers, inliers_before, inliers_after,
        points_recalibrated, points_lost, points_gained;
    double cost_before, cost_after;
};

// the 256-element tree of the summation paragraph; v is overwritten
inline double tree256(double v[kChunk]) {
    double w[kChunk / kWave];
    for (int g = 0; g < kChunk / kWave; ++g) {
        double* a = v + g * kWave;
        for (int m = kWave / 2; m >= 1; m >>= 1) {
            double nxt[kWave];
            for (int j = 0; j < kWave; ++j) nxt[j] = a[j] + a[j ^ m];
            for (int j = 0; j < kWave; ++j) a[j] = nxt[j];
        }
        w[g] = a[0];
    }
    return ((w[0] + w[1]) + w[2]) + w[3];
}

// the two levels over O slots: term(s, v) fills the K contributions of slot s
template <int K, class F>
inline void reduce_slots(long long O, F term, double out[K]) {
    const long long n_chunks = (O + kChunk - 1) / kChunk;
    std::vector<double> part((size_t)kChunk * K, 0.0), val((size_t)kChunk * K);
    for (long long c = 0; c < n_chunks; ++c) {
        for (int j = 0; j < kChunk; ++j) {
            const long long s = c * kChunk + j;
            double* v = val.data() + (size_t)j * K;
            if (s < O) term(s, v);
            else
                for (int k = 0; k < K; ++k) v[k] = 0.0;
        }
        for (int k = 0; k < K; ++k) {
            double v[kChunk];
            for (int j = 0; j < kChunk; ++j) v[j] = val[(size_t)j * K + k];
            double& p = part[(size_t)(c % kChunk) * K + k];
            p = p + tree256(v);
        }
    }
    for (int k = 0; k < K; ++k) {
        double v[kChunk];
        for (int j = 0; j < kChunk; ++j) v[j] = part[(size_t)j * K + k];
        out[k] = tree256(v);
    }
}

struct HostEval {
    const Slot* slots;
    long long O, n_in;
    double max_error;
    int mask;
    long long contributing() const { return n_in; }
    double cost(const msfm_emat::Camera& c, long long* inliers) const {
        long long cnt = 0;
        double out[1];
        reduce_slots<1>(O, [&](long long s, double* v) {
            int in;
            v[0] = slot_cost(slots[s], c, max_error, &in);
            cnt += in;
        }, out);
        *inliers = cnt;
        return out[0];
    }
    void sums(const msfm_emat::Camera& c, double acc[kSums]) const {
        reduce_slots<kSums>(O, [&](long long s, double* v) { slot_sums(slots[s], c, mask, v); }, acc);
    }
};

// tracks, rank_of_id, kxy, poses, mask as RefinePoints takes them (all tracks); cam: read, and REWRITTEN iff the refined camera stands;
// points / residuals: read, and rewritten by the re-verdict.  counts is filled (not added to); trace may be null.
inline void RefineCamera(const int64_t* offsets, const int32_t* image_ids, const int32_t* point_idx, int64_t n_tracks, const int* rank_of_id,
                         const float* const* kxy, const msfm_tri::Pose* poses, const uint8_t* mask, msfm_emat::Camera* cam,
                         const msfm_ref::Verdict& vd, const Params& prm, msfm_point3d* points, double* residuals, Counts* counts,
                         msfm_ref::Trace* trace = nullptr) {
    const int64_t O = offsets[n_tracks];
    std::vector<msfm_ref::Obs> obs((size_t)std::max<int64_t>(O, 1));
    std::vector<Slot> slots((size_t)std::max<int64_t>(O, 1));
    Counts c = {};
    for (int64_t t = 0; t < n_tracks; ++t) {
        const int64_t b = offsets[t], e = offsets[t + 1];
        const msfm_tri::HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
        msfm_ref::host_obs(a, (int)(e - b), mask ? mask + b : nullptr, *cam, obs.data() + b);
        const bool standing = msfm_rp::succeeded(points[t]);
        for (int64_t o = b; o < e; ++o) {
            double px = 0.0, py = 0.0;
            if ((obs[(size_t)o].flags & msfm_ref::OBS_FIT) && standing) a.pixel((int)(o - b), &px, &py);
            prepare_slot(obs[(size_t)o], standing, poses, points[t].X, px, py, &slots[(size_t)o]);
            c.observations += (slots[(size_t)o].flags & SLOT_IN) ? 1 : 0;
            c.behind += (slots[(size_t)o].flags & SLOT_BEHIND) ? 1 : 0;
        }
    }
    const HostEval ev{slots.data(), O, c.observations, vd.max_error, prm.mask};
    Result res;
    refine_camera(ev, prm, cam, &res, trace);
    c.iterations = res.iterations;
    c.accepted_steps = res.accepted;
    c.stop = res.stop;
    c.refined = res.stands;
    c.rejected_by_inliers = (res.accepted > 0 && !res.stands) ? 1 : 0;
    c.inliers_before = res.inliers_before;
    c.inliers_after = res.inliers_after;
    c.cost_before = res.cost_before;
    c.cost_after = res.cost_after;
    if (res.stands) {
        const double f = (cam->fx + cam->fy) / 2.0;
        for (int64_t t = 0; t < n_tracks; ++t) {
            if (!msfm_ref::eligible(points[t])) continue;
            const int64_t b = offsets[t];
            const int n = (int)(offsets[t + 1] - b);
            const msfm_tri::HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
            msfm_ref::host_obs(a, n, mask ? mask + b : nullptr, *cam, obs.data() + b);
            Tally tl;
            recalibrate_track(obs.data() + b, n, poses, f, vd, points + t, residuals + b, &tl);
            c.points_recalibrated += tl.recalibrated;
            c.points_lost += tl.lost;
            c.points_gained += tl.gained;
        }
    }
    *counts = c;
}
#endif

}  // namespace msfm_rc
