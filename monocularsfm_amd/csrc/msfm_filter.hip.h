// msfm_filter.hip.h -- map filtering on the device (include/msfm_match.h "map filtering"): the kernel and the host
// side of msfm_filter_points (defined in msfm_match.hip).  The arithmetic is msfm_filter.h, shared with the host twin FilterPoints: the
// same bits.  Included by msfm_match.hip behind msfm_extend.hip.h, whose ext_mask_kernel it launches unchanged, and behind
// msfm_refine.hip.h, whose ref_obs_kernel it launches unchanged.
//
// The call runs inside msfm_extend.hip.h's MapEditFrame ("the map-edit call frame"), with an all-zero `gained`:
// the frame prepares the inlier bytes and the per-observation array and holds the failure rule; the host waits once, at the end.
//   flt_track_kernel  one lane per kept track, a wave-uniform grid-stride loop, 256 threads, no LDS, the shape of ext_track_kernel.
//                      A lane of a track that is not eligible only counts its record; the others run msfm_flt::filter_track, which
//                      clears OBS_FIT of the observations it drops in the call's own Obs array.  Lanes diverge by their tracks'
//                      lengths and kinds: nothing is exchanged between them before the counters, which go through wave_add_counters.
// Plain vector loads and stores only; no floating-point atomics.
#pragma once
#include "msfm_filter.h"
#include "msfm_extend.hip.h"

namespace msfm {

struct FltCounters {
    unsigned long long eligible, dropped_by_depth, dropped_by_error, trimmed, regained, removed_by_views, removed_by_angle, succeeded,
        observations_used;
};
constexpr int kFltCounters = 9;

__global__ __launch_bounds__(256) void flt_track_kernel(const long long* __restrict__ offsets, const unsigned char* __restrict__ cons, int T,
                                                        msfm_ref::Obs* __restrict__ obs, const msfm_tri::Pose* __restrict__ poses,
                                                        const unsigned char* __restrict__ scope, double f, msfm_ref::Verdict flt,
                                                        msfm_ref::Verdict vd, msfm_point3d* __restrict__ points,
                                                        double* __restrict__ residuals, unsigned char* __restrict__ mask,
                                                        FltCounters* __restrict__ counters) {
    unsigned long long c[kFltCounters] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); t0 < T; t0 += stride) {   // (uniform over the wave)
        const long long t = t0 + lane;
        if (t >= T) continue;
        const long long b = offsets[t], e = offsets[t + 1];
        const int n = (int)(e - b);
        msfm_point3d r = points[t];
        if (cons[t] && msfm_ref::eligible(r) && msfm_flt::in_scope(obs + b, n, scope)) {
            msfm_flt::Tally tl;
            msfm_flt::filter_track(obs + b, n, poses, f, flt, vd, &r, residuals + b, mask + b, &tl);
            if (tl.trace.kind != msfm_flt::KIND_UNTOUCHED) points[t] = r;
            c[0] += 1;
            c[1] += (unsigned long long)tl.trace.dropped_by_depth;
            c[2] += (unsigned long long)tl.trace.dropped_by_error;
            c[3] += tl.trace.kind == msfm_flt::KIND_TRIMMED ? 1 : 0;
            c[4] += (unsigned long long)tl.regained;
            c[5] += tl.trace.kind == msfm_flt::KIND_REMOVED_BY_VIEWS ? 1 : 0;
            c[6] += tl.trace.kind == msfm_flt::KIND_REMOVED_BY_ANGLE ? 1 : 0;
        }
        c[7] += msfm_flt::succeeded(r.status) ? 1 : 0;
        c[8] += (unsigned long long)r.n_views;
    }
    wave_add_counters(c, reinterpret_cast<unsigned long long*>(counters));
}

}  // namespace msfm

namespace {

int filter_impl(msfm_ctx* ctx, const msfm_filter_params* params, const int32_t* image_ids, int n_images, msfm_filter_stats* stats) {
    TrackSession& ts = ctx->tracks;
    const std::string who = "msfm_filter_points";
    if (const int rc = tri_session_check(ctx, who, true)) return rc;
    msfm_ref::Verdict flt = {ts.tri_prm.max_error, ts.tri_prm.min_angle};
    if (params) flt = msfm_ref::Verdict{params->max_error, params->min_angle};
    if (!std::isfinite(flt.max_error) || !std::isfinite(flt.min_angle) || flt.max_error < 0.0 || flt.min_angle < 0.0)
        return fail(ctx, MSFM_E_INVALID, who + ": max_error and min_angle must be finite and not negative");
    if (n_images < 0 || (n_images > 0 && !image_ids)) return fail(ctx, MSFM_E_INVALID, who + ": bad list of images");
    std::vector<unsigned char> scope;
    if (const int rc = rank_bytes(ctx, image_ids, n_images, who + ": image not declared in the session: ", who + ": an image is given twice: ", &scope))
        return rc;
    const std::vector<unsigned char> gained(scope.size(), 0);   // no image gains a pose in this call
    MapEditFrame fr(ctx, who);
    if (const int rc = fr.begin(ts.tri_ids, ts.tri_poses, {&scope, &gained}, sizeof(FltCounters))) return rc;
    if (const int rc = fr.observe(fr.d_bytes(1))) return rc;
    if (fr.live()) {
        hipLaunchKernelGGL(flt_track_kernel, dim3(fr.grid), dim3(256), 0, fr.st, (const long long*)ts.r_offsets.as<long long>(),
                           (const unsigned char*)ts.r_cons.as<unsigned char>(), (int)fr.T, fr.obs.as<msfm_ref::Obs>(), fr.pt.d_poses(),
                           n_images > 0 ? fr.d_bytes(0) : (const unsigned char*)nullptr, (fr.pt.cam.fx + fr.pt.cam.fy) / 2.0, flt,
                           msfm_ref::Verdict{fr.prm.max_error, fr.prm.min_angle}, ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(),
                           ts.t_mask.as<unsigned char>(), fr.counters.as<FltCounters>());
        fr.wrote(hipGetLastError());
    }
    if (const int rc = fr.finish()) return rc;
    FltCounters hc = {};
    HIPCHK(ctx, hipMemcpy(&hc, fr.counters.p, sizeof(hc), hipMemcpyDeviceToHost));
    msfm_filter_stats s = {};
    HIPCHK(ctx, fr.elapsed(&s.prepare_ms, &s.filter_ms));
    s.eligible = (int64_t)hc.eligible;
    s.dropped_by_depth = (int64_t)hc.dropped_by_depth;
    s.dropped_by_error = (int64_t)hc.dropped_by_error;
    s.trimmed = (int64_t)hc.trimmed;
    s.regained = (int64_t)hc.regained;
    s.removed_by_views = (int64_t)hc.removed_by_views;
    s.removed_by_angle = (int64_t)hc.removed_by_angle;
    s.succeeded = (int64_t)hc.succeeded;
    s.observations_used = (int64_t)hc.observations_used;
    if (stats) *stats = s;
    return MSFM_OK;
}

}  // namespace

