// msfm_complete.hip.h -- map completion on the device (include/msfm_match.h "map completion"): the kernel and the
// host side of msfm_complete_points (defined in msfm_match.hip).  The arithmetic is msfm_complete.h, shared with the host twin
// CompletePoints: the same bits.  Included by msfm_match.hip behind msfm_filter.hip.h; like it, it launches msfm_extend.hip.h's
// ext_mask_kernel and msfm_refine.hip.h's ref_obs_kernel unchanged.
//
// The call runs inside msfm_extend.hip.h's MapEditFrame ("the map-edit call frame"), with an all-zero `gained`:
// the frame prepares the inlier bytes and the per-observation array and holds the failure rule; the host waits once, at the end.
//   cmp_track_kernel  one lane per kept track, a wave-uniform grid-stride loop, 256 threads, no LDS, the shape of flt_track_kernel.
//                      A lane of a track that is not eligible only counts its record; the others run msfm_cmp::complete_track, which
//                      sets OBS_FIT of the observations it admits in the call's own Obs array.  Lanes diverge by their tracks'
//                      lengths and kinds: nothing is exchanged between them before the counters, which go through wave_add_counters.
// Plain vector loads and stores only; no floating-point atomics.
#pragma once
#include "msfm_complete.h"
#include "msfm_filter.hip.h"

namespace msfm {

struct CmpCounters {
    unsigned long long eligible, candidates, admitted, rejected_by_depth, rejected_by_error, completed, succeeded, observations_used;
};
constexpr int kCmpCounters = 8;

__global__ __launch_bounds__(256) void cmp_track_kernel(const long long* __restrict__ offsets, const unsigned char* __restrict__ cons, int T,
                                                        msfm_ref::Obs* __restrict__ obs, const msfm_tri::Pose* __restrict__ poses,
                                                        const unsigned char* __restrict__ scope, double f, double max_error,
                                                        msfm_ref::Verdict vd, msfm_point3d* __restrict__ points,
                                                        double* __restrict__ residuals, unsigned char* __restrict__ mask,
                                                        CmpCounters* __restrict__ counters) {
    unsigned long long c[kCmpCounters] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); t0 < T; t0 += stride) {   // (uniform over the wave)
        const long long t = t0 + lane;
        if (t >= T) continue;
        const long long b = offsets[t], e = offsets[t + 1];
        const int n = (int)(e - b);
        msfm_point3d r = points[t];
        if (cons[t] && msfm_ext::continues(r)) {
            msfm_cmp::Trace tr;
            msfm_cmp::complete_track(obs + b, n, poses, scope, f, max_error, vd, &r, residuals + b, mask + b, &tr);
            if (tr.kind == msfm_cmp::KIND_COMPLETED) points[t] = r;
            c[0] += 1;
            c[1] += (unsigned long long)tr.candidates;
            c[2] += (unsigned long long)tr.admitted;
            c[3] += (unsigned long long)tr.rejected_by_depth;
            c[4] += (unsigned long long)(tr.candidates - tr.admitted - tr.rejected_by_depth);
            c[5] += tr.kind == msfm_cmp::KIND_COMPLETED ? 1 : 0;
        }
        c[6] += msfm_flt::succeeded(r.status) ? 1 : 0;
        c[7] += (unsigned long long)r.n_views;
    }
    wave_add_counters(c, reinterpret_cast<unsigned long long*>(counters));
}

}  // namespace msfm

namespace {

int complete_impl(msfm_ctx* ctx, const msfm_complete_params* params, const int32_t* image_ids, int n_images, msfm_complete_stats* stats) {
    TrackSession& ts = ctx->tracks;
    const std::string who = "msfm_complete_points";
    if (const int rc = tri_session_check(ctx, who, true)) return rc;
    const double max_error = params ? params->max_error : ts.tri_prm.max_error;
    if (!std::isfinite(max_error) || max_error < 0.0) return fail(ctx, MSFM_E_INVALID, who + ": max_error must be finite and not negative");
    if (max_error > ts.tri_prm.max_error)
        return fail(ctx, MSFM_E_INVALID, who + ": max_error must not exceed the session's: an admitted observation would clear ERROR_OK");
    if (n_images < 0 || (n_images > 0 && !image_ids)) return fail(ctx, MSFM_E_INVALID, who + ": bad list of images");
    std::vector<unsigned char> scope;
    if (const int rc = rank_bytes(ctx, image_ids, n_images, who + ": image not declared in the session: ", who + ": an image is given twice: ", &scope))
        return rc;
    const std::vector<unsigned char> gained(scope.size(), 0);   // no image gains a pose in this call
    MapEditFrame fr(ctx, who);
    if (const int rc = fr.begin(ts.tri_ids, ts.tri_poses, {&scope, &gained}, sizeof(CmpCounters))) return rc;
    if (const int rc = fr.observe(fr.d_bytes(1))) return rc;
    if (fr.live()) {
        hipLaunchKernelGGL(cmp_track_kernel, dim3(fr.grid), dim3(256), 0, fr.st, (const long long*)ts.r_offsets.as<long long>(),
                           (const unsigned char*)ts.r_cons.as<unsigned char>(), (int)fr.T, fr.obs.as<msfm_ref::Obs>(), fr.pt.d_poses(),
                           n_images > 0 ? fr.d_bytes(0) : (const unsigned char*)nullptr, (fr.pt.cam.fx + fr.pt.cam.fy) / 2.0, max_error,
                           msfm_ref::Verdict{fr.prm.max_error, fr.prm.min_angle}, ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(),
                           ts.t_mask.as<unsigned char>(), fr.counters.as<CmpCounters>());
        fr.wrote(hipGetLastError());
    }
    if (const int rc = fr.finish()) return rc;
    CmpCounters hc = {};
    HIPCHK(ctx, hipMemcpy(&hc, fr.counters.p, sizeof(hc), hipMemcpyDeviceToHost));
    msfm_complete_stats s = {};
    HIPCHK(ctx, fr.elapsed(&s.prepare_ms, &s.complete_ms));
    s.eligible = (int64_t)hc.eligible;
    s.candidates = (int64_t)hc.candidates;
    s.admitted = (int64_t)hc.admitted;
    s.rejected_by_depth = (int64_t)hc.rejected_by_depth;
    s.rejected_by_error = (int64_t)hc.rejected_by_error;
    s.completed = (int64_t)hc.completed;
    s.succeeded = (int64_t)hc.succeeded;
    s.observations_used = (int64_t)hc.observations_used;
    if (stats) *stats = s;
    return MSFM_OK;
}

}  // namespace

