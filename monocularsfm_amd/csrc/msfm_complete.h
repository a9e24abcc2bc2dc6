// msfm_complete.h -- map completion arithmetic shared by the device kernel (msfm_complete.hip.h, hipcc) and the host twin
// (host/HostTestApi.cpp, CompletePoints, g++): the step the reference runs behind its filter after every local adjustment
// (MapBuilder::CompleteTracks -> Map::CompletePoints3D / CompletePoint3D, Map.cpp:654-760) -- observations of a standing point that
// were rejected earlier and FIT AGAIN under the current poses and X are RE-ADMITTED into its fitting set, everything else stays bit for
// bit.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides, every
// sum in element order -> the host twin and the device produce the SAME bits.  Obs, prepare_obs, point_verdict and Verdict are
// msfm_refine.h's, obs_error and parallax_scan are msfm_triangulate.h's, plain_byte and continues are msfm_extend.h's, kDepthEps and
// canonical are msfm_pose.h's.
//
//   threshold       the CALL's max_error (pixels) decides what is admitted; it is never above the SESSION's (the entry point and the
//                   twin's export refuse it), whose max_error and min_angle give a completed record its status bits, as every other
//                   call does.
//   inlier bytes    one per kept observation.  Where the session has none they are created first exactly as msfm_filter.h does it:
//                   plain_byte with an all-zero `gained`.  prepare_obs then sets OBS_FIT from them.  Such a session has no candidate.
//   candidate       an observation with OBS_USED and without OBS_FIT whose image is in scope.  scope: one byte per pose rank (nullptr:
//                   every image).  Unlike the filter's scope, which selects TRACKS by where their fitting observations lie, this one
//                   selects CANDIDATES by where they lie.  (An image without a valid pose has no OBS_USED observation: it selects
//                   nothing.)
//   eligible        a consistent track whose record has POINT | ERROR_OK | ANGLE_OK (msfm_ext::continues).  Every other track stays
//                   bit for bit: a track that does not stand is filtered or extended, not completed.
//   admission       per candidate, in element order: err = obs_error at the record's X under the current pose, f = (fx + fy) / 2.
//                   Rejected BY DEPTH iff its depth is not > kDepthEps; otherwise rejected BY ERROR iff !(err <= max_error) (a NaN is
//                   rejected); otherwise ADMITTED: OBS_FIT is set in the call's own Obs array and the byte becomes 1.  X does not
//                   move, so the candidates do not depend on each other: one pass is a fixed point.
//   untouched       nothing admitted: not one byte is written, the residual slots of the rejected candidates included.
//   completed       something admitted.  The record is re-verdicted over the enlarged fitting set K at the UNCHANGED X with the
//                   session's thresholds by point_verdict in its `residuals != nullptr` mode (the call the filter's trimmed route
//                   makes): every USED observation's slot is written, n_views = |K|, mean_residual = sum / |K|, tri_angle and
//                   ERROR_OK / ANGLE_OK / DEPTH_OK are that verdict's;  status = ATTEMPTED | POINT | the three bits | the record's
//                   ROBUST, REFINED, REPOSED, EXTENDED, FILTERED | COMPLETED.
// MSFM_TRI_COMPLETED is 1024.  The twins of the other calls are not edited and do not know the bit: they treat it as they treat
// FILTERED (msfm_filter.h) -- msfm_refine_points and msfm_refine_poses' re-verdict rebuild the status from named bits and drop it, a
// continuing msfm_extend_points keeps it, a creating msfm_extend_points replaces the record and drops it, msfm_filter_points' trimmed
// route rebuilds the status from named bits and drops it.  A record that a later call did not rewrite keeps the bit.
#pragma once

#include "msfm_extend.h"

namespace msfm_cmp {

enum { KIND_NOT_ELIGIBLE = 0, KIND_UNTOUCHED = 1, KIND_COMPLETED = 2 };

// The route one track took.  Four int32.
struct Trace {
    int32_t kind;               // KIND_*
    int32_t candidates;         // tested: in scope (0 for a track that is not eligible)
    int32_t admitted;
    int32_t rejected_by_depth;  // (rejected by error: candidates - admitted - rejected_by_depth)
};

MSFM_FHD bool is_candidate(const msfm_ref::Obs& o, const unsigned char* scope) {
    return (o.flags & (msfm_ref::OBS_USED | msfm_ref::OBS_FIT)) == msfm_ref::OBS_USED && (!scope || scope[o.rank]);
}

// One ELIGIBLE track: obs, residuals, mask: its n element-aligned slots.  obs is the call's own scratch: OBS_FIT of an admitted
// observation is set in it, so that K is "the OBS_FIT observations" for the verdict.  max_error: the call's, vd: the session's
// thresholds.  rec, residuals and mask are written as the header says; an untouched track writes nothing.
MSFM_FHD void complete_track(msfm_ref::Obs* obs, int n, const msfm_tri::Pose* poses, const unsigned char* scope, double f, double max_error,
                             const msfm_ref::Verdict& vd, msfm_point3d* rec, double* residuals, unsigned char* mask, Trace* trace) {
    using namespace msfm_ref;
    const msfm_point3d old = *rec;
    const double X[3] = {old.X[0], old.X[1], old.X[2]};
    int candidates = 0, admitted = 0, by_depth = 0;
    for (int k = 0; k < n; ++k) {
        const Obs o = obs[k];
        if (!is_candidate(o, scope)) continue;
        candidates += 1;
        const msfm_tri::Pose* p = poses + o.rank;
        bool d;
        const double err = msfm_tri::obs_error(p->R, p->t, o.u, o.w, X, f, &d);
        if (!d) {
            by_depth += 1;
            continue;
        }
        if (!(err <= max_error)) continue;   // (a NaN is rejected)
        admitted += 1;
        obs[k].flags = o.flags | OBS_FIT;
        mask[k] = 1;
    }
    *trace = Trace{KIND_UNTOUCHED, candidates, admitted, by_depth};
    if (admitted == 0) return;
    PointVerdict v;
    point_verdict(obs, n, poses, f, vd, X, residuals, &v);
    msfm_point3d r = old;
    r.status = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | v.bits |
               (old.status & (MSFM_TRI_ROBUST | MSFM_TRI_REFINED | MSFM_TRI_REPOSED | MSFM_TRI_EXTENDED | MSFM_TRI_FILTERED)) |
               MSFM_TRI_COMPLETED;
    r.n_views = v.count;
    r.mean_residual = v.sum / (double)v.count;
    r.tri_angle = v.angle;
    *rec = r;
    trace->kind = KIND_COMPLETED;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: CompletePoints over the outputs of the other twins ---------------------------------------------------------------
struct Counts {
    long long eligible, candidates, admitted, rejected_by_depth, rejected_by_error, completed;
};

// tracks, rank_of_id, kxy as TriangulateTracks takes them; poses: the session's current table by rank; scope: one byte per rank or
// nullptr; prm: the thresholds of the triangulation that made the points; max_error: the call's (not above prm.max_error).  points /
// residuals / mask: read and rewritten in place; have_mask false: the bytes of the tracks of this call are created first (plain_byte,
// nothing gained).  `counts` (may be null) is added to; out_trace (may be null): one Trace per track at the track's own position.
inline void CompletePoints(const int64_t* offsets, const int32_t* image_ids, const int32_t* point_idx, const uint8_t* consistent,
                           int64_t first_track, int64_t n_tracks, const int* rank_of_id, const float* const* kxy, const msfm_tri::Pose* poses,
                           int n_ranks, const uint8_t* scope, const msfm_emat::Camera& cam, const msfm_tri::Params& prm, double max_error,
                           bool have_mask, msfm_point3d* points, double* residuals, uint8_t* mask, Counts* counts,
                           Trace* out_trace = nullptr) {
    const double f = (cam.fx + cam.fy) / 2.0;
    const msfm_ref::Verdict vd = {prm.max_error, prm.min_angle};
    const std::vector<uint8_t> gained((size_t)(n_ranks > 0 ? n_ranks : 1), 0);
    std::vector<msfm_ref::Obs> obs;
    for (int64_t t = first_track; t < first_track + n_tracks; ++t) {
        const int64_t b = offsets[t], e = offsets[t + 1];
        const int n = (int)(e - b);
        const msfm_tri::HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
        if (!have_mask) msfm_ext::plain_bytes(a, n, points[t], gained.data(), mask + b);
        Trace tr = {KIND_NOT_ELIGIBLE, 0, 0, 0};
        if (consistent[t] && msfm_ext::continues(points[t])) {
            obs.resize((size_t)n);
            msfm_ref::host_obs(a, n, mask + b, cam, obs.data());
            complete_track(obs.data(), n, poses, scope, f, max_error, vd, points + t, residuals + b, mask + b, &tr);
            if (counts) {
                counts->eligible += 1;
                counts->candidates += tr.candidates;
                counts->admitted += tr.admitted;
                counts->rejected_by_depth += tr.rejected_by_depth;
                counts->rejected_by_error += tr.candidates - tr.admitted - tr.rejected_by_depth;
                counts->completed += tr.kind == KIND_COMPLETED ? 1 : 0;
            }
        }
        if (out_trace) out_trace[t] = tr;
    }
}
#endif

}  // namespace msfm_cmp
