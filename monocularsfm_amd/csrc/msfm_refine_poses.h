// msfm_refine_poses.h -- pose refinement arithmetic shared by the device kernels (msfm_refine_poses.hip.h, hipcc) and the host twin
// (host/HostTestApi.cpp, RefinePoses, g++): every posed image is moved to the minimum of its reprojection error under FIXED points by
// Levenberg-Marquardt, one 6 x 6 system per image.  The pose block of a bundle adjustment and nothing more:
// msfm_refine.h is the point block, a caller alternates the two.  Points' X, tracks and inlier bytes never change.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides -> the host
// twin and the device produce the SAME bits.  Obs, prepare_obs, eligible, lm_minimise (the LM loop, its constants, STOP_*, Trace) and
// point_verdict are msfm_refine.h's, gn_add, kRegSums, cholesky6_solve and cayley_update msfm_register.h's, obs_error, transform, centre
// msfm_triangulate.h's, kDepthEps msfm_pose.h's.
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
//   step            (H + lambda diag H) delta = -g by msfm_reg::cholesky6_solve (lm_step fills the damped diagonal); delta = (a, dt)
//                   applied by msfm_reg::cayley_update as R <- C(a) R, t <- C(a) t + dt with Cayley's C.  A pivot that is not > 0, a
//                   non-finite delta or a non-finite new pose: the step is rejected without a cost evaluation.
//   LM              msfm_ref::lm_minimise over ImageProblem:  lambda = kLambda0; c = c(R, t).  While fewer than max_iters steps have
//                   been evaluated:
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
//                   under the new poses: msfm_ref::point_verdict with the residual slots -- err of every USED observation; over the
//                   fitting set, in observation order, the errors' sum, ERROR_OK, DEPTH_OK, the parallax scan.  status = ATTEMPTED |
//                   POINT | the three bits | the record's ROBUST and REFINED bits | REPOSED; mean_residual, tri_angle and the residual
//                   slots of the USED observations are rewritten; n_views and X are kept.
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
        const double X[3] = {cX[i], cY[i], cZ[i]};
        double Y[3];
        msfm_tri::transform(R, t, X, Y);
        d = d && Y[2] > msfm_pose::kDepthEps;
        const double rx = (Y[0] / Y[2] - cu[i]) * f, ry = (Y[1] / Y[2] - cw[i]) * f;
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

// (H + lambda diag H) x = -g from the 27 sums by msfm_reg::cholesky6_solve, the new pose by msfm_reg::cayley_update.  False: no step.
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
    return msfm_reg::cholesky6_solve(L, acc + 21, x) && msfm_reg::cayley_update(x, R, t, Rn, tn);
}

// one pose under fixed points: the 6 x 6 problem of msfm_ref::lm_minimise over the reduced passes of `ev`
template <class E>
struct ImageProblem {
    struct State {
        double R[9], t[3];
    };
    struct System {
        double acc[msfm_reg::kRegSums];
    };
    const E& ev;
    MSFM_FHD double cost(const State& s, bool* depth) const { return ev.cost(s.R, s.t, depth); }
    MSFM_FHD void linearise(const State& s, System* sys) const { ev.sums(s.R, s.t, sys->acc); }
    MSFM_FHD bool step(const System& sys, double lambda, const State& s, State* sn, double* d2) const {
        double x[6];
        if (!lm_step(sys.acc, lambda, s.R, s.t, sn->R, sn->t, x)) return false;
        *d2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3] + x[4] * x[4] + x[5] * x[5];
        return true;
    }
    MSFM_FHD double stop_scale(const State& s) const { return 1.0 + (s.t[0] * s.t[0] + s.t[1] * s.t[1] + s.t[2] * s.t[2]); }
};

// One eligible image.  `ev` owns the image's list and gives the three REDUCED passes, the same bits wherever it runs:
//   ev.cost(R, t, &depth) -> c(R, t), depth: every entry has Y.z > kDepthEps;   ev.sums(R, t, acc) -> the 27 sums;
//   ev.inliers(R, t) -> the standing rule's count.
// (R, t): read, and rewritten iff the refined pose stands.  res is always filled; trace may be null and changes nothing.
template <class E>
MSFM_FHD void refine_image(const E& ev, const Params& prm, double R[9], double t[3], Result* res, msfm_ref::Trace* trace) {
    const ImageProblem<E> pb{ev};
    typename ImageProblem<E>::State s;
MSFM_UNROLL
    for (int k = 0; k < 9; ++k) s.R[k] = R[k];
MSFM_UNROLL
    for (int k = 0; k < 3; ++k) s.t[k] = t[k];
    msfm_ref::LmRun run;
    msfm_ref::lm_minimise(pb, prm.max_iters, prm.step_tol, &s, &run);
    const int before = ev.inliers(R, t);
    const int after = run.accepted > 0 ? ev.inliers(s.R, s.t) : before;
    const bool stands = run.accepted > 0 && after >= before;
    res->stands = stands ? 1 : 0;
    res->iterations = run.steps;
    res->stop = run.stop;
    res->inliers_before = before;
    res->inliers_after = after;
    res->accepted = run.accepted;
    res->cost_before = run.cost_before;
    res->cost_after = stands ? run.cost : run.cost_before;
    if (trace) msfm_ref::trace_of(run, stands ? 0 : (run.accepted > 0 ? LOST_INLIERS : NO_ACCEPTED_STEP), trace);
    if (stands) {
MSFM_UNROLL
        for (int k = 0; k < 9; ++k) R[k] = s.R[k];
MSFM_UNROLL
        for (int k = 0; k < 3; ++k) t[k] = s.t[k];
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
// table; rec: read and rewritten.  msfm_ref::point_verdict at the record's X, the residual slots included.
MSFM_FHD void reverdict_track(const msfm_ref::Obs* obs, int n, const msfm_tri::Pose* poses, double f, const msfm_ref::Verdict& vd,
                              msfm_point3d* rec, double* residuals, Tally* tally) {
    const msfm_point3d old = *rec;
    const double X[3] = {old.X[0], old.X[1], old.X[2]};
    msfm_ref::PointVerdict v;
    msfm_ref::point_verdict(obs, n, poses, f, vd, X, residuals, &v);
    msfm_point3d r = old;
    r.status = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | v.bits | (old.status & (MSFM_TRI_ROBUST | MSFM_TRI_REFINED)) | MSFM_TRI_REPOSED;
    r.mean_residual = v.sum / (double)v.count;
    r.tri_angle = v.angle;
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
                        Counts* counts, msfm_ref::Trace* out_trace = nullptr) {
    const double f = (cam.fx + cam.fy) / 2.0;
    const int64_t O = offsets[n_tracks];
    std::vector<msfm_ref::Obs> obs((size_t)std::max<int64_t>(O, 1));
    for (int64_t t = 0; t < n_tracks; ++t) {
        const int64_t b = offsets[t], e = offsets[t + 1];
        const msfm_tri::HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
        msfm_ref::host_obs(a, (int)(e - b), mask ? mask + b : nullptr, cam, obs.data() + b);
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
        if (out_trace) out_trace[k] = msfm_ref::Trace{0, 0, msfm_ref::STOP_NONE, NOT_ELIGIBLE, 0, 0, 0.0, 0.0};
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
