// msfm_filter.h -- map filtering arithmetic shared by the device kernel (msfm_filter.hip.h, hipcc) and the host twin
// (host/HostTestApi.cpp, FilterPoints, g++): the step the reference runs after every local or global adjustment
// (MapBuilder::FilterTracks / FilterAllTracks -> Map::FilterPoints3DWithLargeReprojectionError, then ...WithSmallTriangulationAngle,
// Map.cpp:762-917) -- observations that no longer fit their point are DROPPED from its fitting set, points left with fewer than two
// observations or without a wide pair are REMOVED, everything else stays bit for bit.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides, every
// sum in element order -> the host twin and the device produce the SAME bits.  Obs, prepare_obs, point_verdict and Verdict are
// msfm_refine.h's, Pose, obs_error and parallax_scan are msfm_triangulate.h's, plain_byte is msfm_extend.h's, kDepthEps and canonical
// are msfm_pose.h's.
//
//   thresholds      the CALL's max_error (pixels) and min_angle (degrees) decide what is dropped and what is removed; the SESSION's
//                   (those of the triangulation that made the points) give a trimmed record its status bits, as every other call does.
//   inlier bytes    one per kept observation.  Where the session has none they are created first exactly as msfm_extend.h does it:
//                   plain_byte with an all-zero `gained`.  prepare_obs then sets OBS_FIT from them.
//   scope           one byte per pose rank (nullptr: every track).  A track is IN SCOPE iff one of its OBS_FIT observations lies in an
//                   image whose byte is set.  (An image without a valid pose has no OBS_FIT observation: it selects nothing.)
//   eligible        a consistent track whose record has ATTEMPTED | POINT and which is in scope.  Every other track stays bit for bit.
//   drop            per OBS_FIT observation, in element order: err = obs_error at the record's X under the current pose, f = (fx + fy)
//                   / 2.  Dropped BY DEPTH iff its depth is not > kDepthEps; otherwise dropped BY ERROR iff !(err <= max_error) (a NaN
//                   is dropped).  The reference's order: depth first.  K: the survivors.
//   removed         BY VIEWS iff |K| < 2 (the reference removes a point when all its observations, or all but one, are deleted);
//                   otherwise BY ANGLE iff parallax_scan over K in element order with the call's min_angle finds no pair -- whether or
//                   not anything was dropped.  The record becomes the robust call's "no consensus" record: status = ATTEMPTED |
//                   FILTERED, every other field 0, every residual slot of the track -1.0, every inlier byte of the track 0.  It is no
//                   longer POINT: registration and the refinements skip it, msfm_extend_points creates it afresh when a new image
//                   sees it.
//   untouched       nothing dropped, not removed: not one byte is written, the residual slots included.
//   trimmed         something dropped, not removed.  The dropped observations' bytes become 0.  The record is re-verdicted over K at
//                   the UNCHANGED X with the session's thresholds by point_verdict in its `residuals != nullptr` mode: every USED
//                   observation's slot is written (the dropped ones keep their error), n_views = |K|, mean_residual = sum / |K|,
//                   tri_angle and ERROR_OK / ANGLE_OK / DEPTH_OK are that verdict's;  status = ATTEMPTED | POINT | the three bits |
//                   the record's ROBUST, REFINED, REPOSED, EXTENDED | FILTERED.  REGAINED: it did not have POINT & ERROR_OK & ANGLE_OK
//                   and now has it.
// Information is lost on purpose: a point without ANGLE_OK that the triangulation kept as a diagnostic record is removed by the angle
// rule (under the session's own min_angle always), and a removed record no longer says why it failed.
// MSFM_TRI_FILTERED is 512.  The twins of the other calls are not edited and do not know the bit: whatever a later msfm_refine_points,
// msfm_refine_poses or msfm_extend_points does to an EXTENDED bit when it rewrites a record, it does to this one -- msfm_refine_points
// and msfm_refine_poses' re-verdict rebuild the status from named bits and drop both, a continuing msfm_extend_points keeps both, a
// creating msfm_extend_points replaces the record and drops both.  A record that a later call did not rewrite keeps the bit.
#pragma once

#include "msfm_extend.h"

namespace msfm_flt {

enum { KIND_NOT_ELIGIBLE = 0, KIND_UNTOUCHED = 1, KIND_TRIMMED = 2, KIND_REMOVED_BY_VIEWS = 3, KIND_REMOVED_BY_ANGLE = 4 };

// The route one track took.  Four int32.
struct Trace {
    int32_t kind;               // KIND_*
    int32_t dropped_by_depth;
    int32_t dropped_by_error;
    int32_t kept;               // |K| (0 for a track that is not eligible)
};

// what one eligible track adds to the call's statistics besides its Trace
struct Tally {
    Trace trace;
    int32_t regained;
};

MSFM_FHD bool succeeded(int status) {
    const int ok = MSFM_TRI_POINT | MSFM_TRI_ERROR_OK | MSFM_TRI_ANGLE_OK;
    return (status & ok) == ok;
}

// scope: one byte per rank, nullptr = every track
MSFM_FHD bool in_scope(const msfm_ref::Obs* obs, int n, const unsigned char* scope) {
    if (!scope) return true;
    bool in = false;
    for (int k = 0; k < n; ++k) {
        const msfm_ref::Obs o = obs[k];
        in = in || ((o.flags & msfm_ref::OBS_FIT) && scope[o.rank]);
    }
    return in;
}

// One ELIGIBLE track: obs, residuals, mask: its n element-aligned slots.  obs is the call's own scratch: the OBS_FIT flag of a dropped
// observation is cleared in it, so that K is "the OBS_FIT observations" for everything that follows.  flt: the call's thresholds, vd:
// the session's.  rec, residuals and mask are written as the header says; an untouched track writes nothing.
MSFM_FHD void filter_track(msfm_ref::Obs* obs, int n, const msfm_tri::Pose* poses, double f, const msfm_ref::Verdict& flt,
                           const msfm_ref::Verdict& vd, msfm_point3d* rec, double* residuals, unsigned char* mask, Tally* tally) {
    using namespace msfm_ref;
    const msfm_point3d old = *rec;
    const double X[3] = {old.X[0], old.X[1], old.X[2]};
    int by_depth = 0, by_error = 0, kept = 0;
    for (int k = 0; k < n; ++k) {
        const Obs o = obs[k];
        if (!(o.flags & OBS_FIT)) continue;
        const msfm_tri::Pose* p = poses + o.rank;
        bool d;
        const double err = msfm_tri::obs_error(p->R, p->t, o.u, o.w, X, f, &d);
        const bool keep = d && err <= flt.max_error;   // (false for a NaN)
        if (keep) {
            kept += 1;
            continue;
        }
        by_depth += d ? 0 : 1;
        by_error += d ? 1 : 0;
        obs[k].flags = o.flags & ~OBS_FIT;
        mask[k] = 0;   // (a track with a dropped observation ends trimmed or removed: the byte is 0 in both)
    }
    tally->trace = Trace{KIND_UNTOUCHED, by_depth, by_error, kept};
    tally->regained = 0;
    bool removed = kept < 2;
    if (removed) {
        tally->trace.kind = KIND_REMOVED_BY_VIEWS;
    } else {
        double angle;
        removed = !msfm_tri::parallax_scan(X, n, flt.min_angle, [&](int k) -> const double* {
            const Obs o = obs[k];
            return (o.flags & OBS_FIT) ? poses[o.rank].O : nullptr;
        }, &angle);
        if (removed) tally->trace.kind = KIND_REMOVED_BY_ANGLE;
    }
    if (removed) {
        msfm_point3d r;
        msfm_tri::clear_point(&r);
        r.status = MSFM_TRI_ATTEMPTED | MSFM_TRI_FILTERED;
        *rec = r;
        for (int k = 0; k < n; ++k) {
            residuals[k] = -1.0;
            mask[k] = 0;
        }
        return;
    }
    if (by_depth + by_error == 0) return;
    PointVerdict v;
    point_verdict(obs, n, poses, f, vd, X, residuals, &v);
    msfm_point3d r = old;
    r.status = MSFM_TRI_ATTEMPTED | MSFM_TRI_POINT | v.bits |
               (old.status & (MSFM_TRI_ROBUST | MSFM_TRI_REFINED | MSFM_TRI_REPOSED | MSFM_TRI_EXTENDED)) | MSFM_TRI_FILTERED;
    r.n_views = v.count;
    r.mean_residual = v.sum / (double)v.count;
    r.tri_angle = v.angle;
    *rec = r;
    tally->trace.kind = KIND_TRIMMED;
    tally->regained = (!succeeded(old.status) && succeeded(r.status)) ? 1 : 0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: FilterPoints over the outputs of the other twins --------------------------------------------------------------------
struct Counts {
    long long eligible, dropped_by_depth, dropped_by_error, trimmed, regained, removed_by_views, removed_by_angle;
};

// tracks, rank_of_id, kxy as TriangulateTracks takes them; poses: the session's current table by rank; scope: one byte per rank or
// nullptr; prm: the thresholds of the triangulation that made the points; flt: the call's.  points / residuals / mask: read and
// rewritten in place; have_mask false: the bytes of the tracks of this call are created first (plain_byte, nothing gained).  `counts`
// (may be null) is added to; out_trace (may be null): one Trace per track at the track's own position.
inline void FilterPoints(const int64_t* offsets, const int32_t* image_ids, const int32_t* point_idx, const uint8_t* consistent,
                         int64_t first_track, int64_t n_tracks, const int* rank_of_id, const float* const* kxy, const msfm_tri::Pose* poses,
                         int n_ranks, const uint8_t* scope, const msfm_emat::Camera& cam, const msfm_tri::Params& prm,
                         const msfm_ref::Verdict& flt, bool have_mask, msfm_point3d* points, double* residuals, uint8_t* mask,
                         Counts* counts, Trace* out_trace = nullptr) {
    const double f = (cam.fx + cam.fy) / 2.0;
    const msfm_ref::Verdict vd = {prm.max_error, prm.min_angle};
    const std::vector<uint8_t> gained((size_t)(n_ranks > 0 ? n_ranks : 1), 0);
    std::vector<msfm_ref::Obs> obs;
    for (int64_t t = first_track; t < first_track + n_tracks; ++t) {
        const int64_t b = offsets[t], e = offsets[t + 1];
        const int n = (int)(e - b);
        const msfm_tri::HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
        if (!have_mask) msfm_ext::plain_bytes(a, n, points[t], gained.data(), mask + b);
        obs.resize((size_t)n);
        msfm_ref::host_obs(a, n, mask + b, cam, obs.data());
        Tally tl = {Trace{KIND_NOT_ELIGIBLE, 0, 0, 0}, 0};
        if (consistent[t] && msfm_ref::eligible(points[t]) && in_scope(obs.data(), n, scope)) {
            filter_track(obs.data(), n, poses, f, flt, vd, points + t, residuals + b, mask + b, &tl);
            if (counts) {
                counts->eligible += 1;
                counts->dropped_by_depth += tl.trace.dropped_by_depth;
                counts->dropped_by_error += tl.trace.dropped_by_error;
                counts->trimmed += tl.trace.kind == KIND_TRIMMED ? 1 : 0;
                counts->regained += tl.regained;
                counts->removed_by_views += tl.trace.kind == KIND_REMOVED_BY_VIEWS ? 1 : 0;
                counts->removed_by_angle += tl.trace.kind == KIND_REMOVED_BY_ANGLE ? 1 : 0;
            }
        }
        if (out_trace) out_trace[t] = tl.trace;
    }
}
#endif

}  // namespace msfm_flt
