// msfm_extend.h -- map extension arithmetic shared by the device kernels (msfm_extend.hip.h, hipcc) and the host twin
// (host/HostTestApi.cpp, ExtendPoints, g++): the step of the reference's MapBuilder::TryRegisterNextImage that brings newly posed
// images into the map (MapBuilder.cpp:445-571, Map::CompletePoint3D) -- standing points are CONTINUED into the new images without
// moving, tracks that only now have enough posed views are CREATED, everything else stays bit for bit.
//
// The contract of msfm_pose.h holds: fp64 with +, -, *, /, sqrt only, static loop structure, -ffp-contract=off on both sides, every
// sum in element order -> the host twin and the device produce the SAME bits.  Obs and prepare_obs are msfm_refine.h's, Pose,
// parallax_scan, obs_error, triangulate_track, retry and robust_track are msfm_triangulate.h's, kDepthEps is msfm_pose.h's.
//
//   gained          one byte per pose rank: the image got its valid pose in this call.  A NEW OBSERVATION of a track is an element
//                   that is OBS_USED under the enlarged pose table and whose image has the byte set.
//   inlier bytes    one per kept observation.  Where the session has none (its points are the plain call's) they are created first
//                   (plain_bytes): 1 on every element of an ATTEMPTED track whose image had a valid pose BEFORE the call, else 0 --
//                   what the robust call gives a track that passes its plain test.  prepare_obs then sets OBS_FIT from them.
//   untouched       a track without a new observation, or an inconsistent one: not one byte of it is written.
//   continue        the record has POINT | ERROR_OK | ANGLE_OK (extend_track).  X never changes.  Per new observation, in element
//                   order: err = obs_error at X under the new pose, f = (fx + fy) / 2; its residual slot = err; its inlier byte = 1
//                   iff depth > kDepthEps and err <= max_error (a NaN fails), else 0.  None accepted: the record stays bit for bit.
//                   Otherwise, over the byte-1 observations in element order: n_views = their number; mean_residual = their residual
//                   SLOTS (old ones are read, never recomputed or rewritten) summed from 0.0 / n_views; tri_angle =
//                   msfm_tri::parallax_scan over them; status = every bit it had | EXTENDED.
//                   The old pairs are still scanned, so ANGLE_OK stays; every accepted observation passed the error and the depth
//                   test, so ERROR_OK and DEPTH_OK cannot be lost.
//   create          every other consistent track with a new observation: triangulate_track over all its posed elements under the
//                   enlarged table, the inlier bytes 1 on the used observations of an attempted track; with max_hypotheses >= 1 the
//                   tracks that retry() selects go through the robust consensus (robust_track / trr_retry_kernel).  The record, the
//                   residual slots and the bytes are that result | EXTENDED: apart from the bit, byte for byte what a full
//                   msfm_triangulate_tracks / _robust gives the track under the enlarged pose list.
#pragma once

#include "msfm_refine.h"

namespace msfm_ext {

enum { KIND_UNTOUCHED = 0, KIND_CONTINUE = 1, KIND_CREATE = 2 };
enum { ROUTE_NONE = 0, ROUTE_PLAIN = 1, ROUTE_ROBUST = 2 };   // ROUTE_ROBUST: a created track that went through the hypotheses

// what one continued track adds to the call's statistics
struct Tally {
    int32_t accepted, rejected;
};

// The route one track took: host only.  Four int32.
struct Trace {
    int32_t kind;               // KIND_*
    int32_t new_observations;
    int32_t accepted;           // continue: new observations with byte 1; create: 0
    int32_t route;              // ROUTE_*
};

MSFM_FHD bool continues(const msfm_point3d& r) {
    const int need = MSFM_TRI_POINT | MSFM_TRI_ERROR_OK | MSFM_TRI_ANGLE_OK;
    return (r.status & need) == need;
}

MSFM_FHD bool is_new(const msfm_ref::Obs& o, const unsigned char* gained) { return (o.flags & msfm_ref::OBS_USED) && gained[o.rank]; }

MSFM_FHD int new_observations(const msfm_ref::Obs* obs, int n, const unsigned char* gained) {
    int c = 0;
    for (int k = 0; k < n; ++k) c += is_new(obs[k], gained) ? 1 : 0;
    return c;
}

// the byte of element k on a session without bytes: p its pose under the ENLARGED table (nullptr: none)
MSFM_FHD unsigned char plain_byte(const msfm_point3d& r, const msfm_tri::Pose* p, int rank, const unsigned char* gained) {
    return ((r.status & MSFM_TRI_ATTEMPTED) && p && !gained[rank]) ? 1 : 0;
}

// One continued track: obs, residuals, mask: its n element-aligned slots (OBS_FIT: the byte was 1 before the call); rec: read, and
// rewritten iff a new observation is accepted.  tally is always filled.
MSFM_FHD void extend_track(const msfm_ref::Obs* obs, int n, const msfm_tri::Pose* poses, const unsigned char* gained, double f,
                           const msfm_ref::Verdict& vd, msfm_point3d* rec, double* residuals, unsigned char* mask, Tally* tally) {
    using namespace msfm_ref;
    const msfm_point3d old = *rec;
    const double X[3] = {old.X[0], old.X[1], old.X[2]};
    int accepted = 0, rejected = 0;
    for (int k = 0; k < n; ++k) {
        const Obs o = obs[k];
        if (!is_new(o, gained)) continue;
        const msfm_tri::Pose* p = poses + o.rank;
        bool d;
        const double err = msfm_tri::obs_error(p->R, p->t, o.u, o.w, X, f, &d);
        const bool in = d && err <= vd.max_error;   // (false for a NaN)
        residuals[k] = msfm_pose::canonical(err);
        mask[k] = in ? 1 : 0;
        accepted += in ? 1 : 0;
        rejected += in ? 0 : 1;
    }
    tally->accepted = accepted;
    tally->rejected = rejected;
    if (accepted == 0) return;
    // the byte-1 observations: those that were fitting, and the new ones just accepted (their bytes are read back)
    double sum = 0.0;
    int count = 0;
    for (int k = 0; k < n; ++k) {
        const Obs o = obs[k];
        if (!((o.flags & OBS_FIT) || (is_new(o, gained) && mask[k]))) continue;
        sum = sum + residuals[k];
        count += 1;
    }
    double angle;
    (void)msfm_tri::parallax_scan(X, n, vd.min_angle, [&](int k) -> const double* {
        const Obs o = obs[k];
        return ((o.flags & OBS_FIT) || (is_new(o, gained) && mask[k])) ? poses[o.rank].O : nullptr;
    }, &angle);
    msfm_point3d r = old;
    r.status = old.status | MSFM_TRI_EXTENDED;
    r.n_views = count;
    r.mean_residual = sum / (double)count;
    r.tri_angle = angle;
    *rec = r;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: ExtendPoints over the outputs of the triangulation / refinement twins -------------------------------------------
struct Counts {
    long long tracks_touched, continued, observations_added, observations_rejected, created_attempted, created, retried;
};

// the bytes of one track (a: its n elements) on a session without them: plain_byte of every element under a's pose table
inline void plain_bytes(const msfm_tri::HostTrack& a, int n, const msfm_point3d& r, const uint8_t* gained, uint8_t* mask) {
    for (int k = 0; k < n; ++k) {
        const msfm_tri::Pose* p = a.pose(k);
        mask[k] = plain_byte(r, p, p ? (int)(p - a.poses) : 0, gained);   // (without a pose the rank is not read)
    }
}

// tracks, rank_of_id, kxy as TriangulateTracks takes them; poses: the ENLARGED table by rank; gained: one byte per rank; prm: the
// thresholds of the triangulation that made the points; max_hypotheses: 0 = the plain route for created tracks, 1 .. 1024 = the robust
// one.  points / residuals / mask: read and rewritten in place; have_mask false: the bytes of the tracks of this call are created
// first.  `counts` (may be null) is added to; out_trace (may be null): one Trace per track at the track's own position.
inline void ExtendPoints(const int64_t* offsets, const int32_t* image_ids, const int32_t* point_idx, const uint8_t* consistent,
                         int64_t first_track, int64_t n_tracks, const int* rank_of_id, const float* const* kxy, const msfm_tri::Pose* poses,
                         const uint8_t* gained, const msfm_emat::Camera& cam, const msfm_tri::Params& prm, int max_hypotheses,
                         bool have_mask, msfm_point3d* points, double* residuals, uint8_t* mask, Counts* counts,
                         Trace* out_trace = nullptr) {
    const double f = (cam.fx + cam.fy) / 2.0;
    const msfm_ref::Verdict vd = {prm.max_error, prm.min_angle};
    const int ok = MSFM_TRI_POINT | MSFM_TRI_ERROR_OK | MSFM_TRI_ANGLE_OK;
    std::vector<msfm_ref::Obs> obs;
    for (int64_t t = first_track; t < first_track + n_tracks; ++t) {
        const int64_t b = offsets[t], e = offsets[t + 1];
        const int n = (int)(e - b);
        const msfm_tri::HostTrack a{image_ids + b, point_idx + b, rank_of_id, kxy, poses};
        if (!have_mask) plain_bytes(a, n, points[t], gained, mask + b);
        obs.resize((size_t)n);
        msfm_ref::host_obs(a, n, mask + b, cam, obs.data());
        const int fresh = consistent[t] ? new_observations(obs.data(), n, gained) : 0;
        Trace tr = {KIND_UNTOUCHED, fresh, 0, ROUTE_NONE};
        if (fresh > 0 && continues(points[t])) {
            Tally tl;
            extend_track(obs.data(), n, poses, gained, f, vd, points + t, residuals + b, mask + b, &tl);
            tr.kind = KIND_CONTINUE;
            tr.accepted = tl.accepted;
            if (counts) {
                counts->tracks_touched += 1;
                counts->continued += tl.accepted > 0 ? 1 : 0;
                counts->observations_added += tl.accepted;
                counts->observations_rejected += tl.rejected;
            }
        } else if (fresh > 0) {
            tr.kind = KIND_CREATE;
            tr.route = ROUTE_PLAIN;
            if (max_hypotheses > 0) {
                msfm_tri::RobustCounts rc = {0, 0, 0, 0};
                msfm_tri::robust_track(a, n, true, (long long)t, cam, msfm_tri::RobustParams{prm.max_error, prm.min_angle, prm.min_views, max_hypotheses},
                                       points + t, residuals + b, mask + b, &rc);
                if (rc.retried) tr.route = ROUTE_ROBUST;
                if (counts) counts->retried += rc.retried;
            } else {
                msfm_tri::triangulate_track(a, n, true, cam, prm, points + t, residuals + b);
                for (int k = 0; k < n; ++k) mask[b + k] = ((points[t].status & MSFM_TRI_ATTEMPTED) && a.pose(k)) ? 1 : 0;
            }
            points[t].status |= MSFM_TRI_EXTENDED;
            if (counts) {
                counts->tracks_touched += 1;
                counts->created_attempted += 1;
                counts->created += (points[t].status & ok) == ok ? 1 : 0;
            }
        }
        if (out_trace) out_trace[t] = tr;
    }
}
#endif

}  // namespace msfm_ext
