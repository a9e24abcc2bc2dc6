// msfm_filter.hip.h -- map filtering on the device (include/msfm_match.h "map filtering"): the kernel and the host
// side of msfm_filter_points (defined in msfm_match.hip).  The arithmetic is msfm_filter.h, shared with the host twin FilterPoints: the
// same bits.  Included by msfm_match.hip behind msfm_extend.hip.h, whose ext_mask_kernel it launches unchanged, and behind
// msfm_refine.hip.h, whose ref_obs_kernel it launches unchanged.
//
// Everything runs on the library's stream between HIP events; the host waits once, at the end.
//   ext_mask_kernel    (msfm_extend.hip.h) with an all-zero `gained`; launched only on a session without inlier bytes.
//   ref_obs_kernel     (msfm_refine.hip.h) under the session's pose table and the current bytes.
//   flt_track_kernel   one lane per kept track, a wave-uniform grid-stride loop, 256 threads, no LDS, the shape of ext_track_kernel.
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
    const int n_img = (int)ts.nd.ids.size();
    std::vector<unsigned char> scope((size_t)std::max(n_img, 1), 0), gained((size_t)std::max(n_img, 1), 0);
    for (int k = 0; k < n_images; ++k) {
        const int id = image_ids[k];
        if (!ts.declares(id)) return fail(ctx, MSFM_E_INVALID, who + ": image not declared in the session: " + std::to_string(id));
        const int r = ts.rank_of[(size_t)id];
        if (scope[(size_t)r]) return fail(ctx, MSFM_E_INVALID, who + ": an image is given twice: " + std::to_string(id));
        scope[(size_t)r] = 1;
    }
    const msfm_tri::Params prm = {ts.tri_prm.max_error, ts.tri_prm.min_angle, ts.tri_prm.min_views, 0};
    std::vector<msfm_pose_rt> by_rank;
    std::vector<TriImage> table;
    if (const int rc = tri_tables(ctx, who, &ts.tri_camera, ts.tri_ids.data(), ts.tri_poses.data(), (int)ts.tri_ids.size(), prm, &by_rank, &table))
        return rc;   // (a posed image lost its keypoints: still nothing of the session is touched)
    // every check has passed: the registrations and the pose refinement's records are gone, they describe the map as it was
    ts.reg_valid = ts.rp_valid = false;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool had_mask = ts.mask_valid;
    const long long T = ts.stats.tracks_kept, O = ts.stats.observations_kept;
    PoseTables pt;   // (the temporaries are freed when the call returns, whatever it returns)
    struct {
        TmpBuf bytes, counters, obs;
    } t;
    TmpEvents<3> ev;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, ev.create());
    HIPCHK(ctx, t.bytes.ensure(2 * scope.size()));   // the scope | the all-zero `gained`
    HIPCHK(ctx, t.counters.ensure(sizeof(FltCounters)));
    HIPCHK(ctx, t.obs.ensure((size_t)std::max<long long>(1, O) * sizeof(msfm_ref::Obs)));
    HIPCHK(ctx, ts.t_mask.ensure((size_t)std::max<long long>(1, O)));
    HIPCHK(ctx, pt.upload(ts.tri_camera, by_rank, table, n_img));
    // (synchronous copies of the small tables: nothing queued reads host memory that an early return below would free)
    unsigned char* d_scope = t.bytes.as<unsigned char>();
    unsigned char* d_gained = d_scope + scope.size();
    HIPCHK(ctx, hipMemcpy(d_scope, scope.data(), scope.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(d_gained, gained.data(), gained.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemsetAsync(t.counters.p, 0, sizeof(FltCounters), st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    HIPCHK(ctx, pt.prepare(st));
    const msfm_emat::Camera cam = pt.cam;
    const unsigned grid = tk_grid(ctx, T);
    hipError_t queued = hipSuccess;   // from the first kernel that writes session memory on, an error drops the session's points
    auto wrote = [&](hipError_t e) {
        if (e != hipSuccess && queued == hipSuccess) queued = e;
        return e == hipSuccess;
    };
    if (T > 0 && O > 0) {
        if (!had_mask) {
            hipLaunchKernelGGL(ext_mask_kernel, dim3(grid), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(),
                               (const int*)ts.r_img.as<int>(), (int)T, pt.d_table(), pt.d_poses(), (const unsigned char*)d_gained,
                               (const msfm_point3d*)ts.t_points.as<msfm_point3d>(), ts.t_mask.as<unsigned char>());
            wrote(hipGetLastError());
        }
        if (queued == hipSuccess) {
            hipLaunchKernelGGL(ref_obs_kernel, dim3(tk_grid(ctx, O)), dim3(256), 0, st, (const int*)ts.r_img.as<int>(), (const int*)ts.r_idx.as<int>(), O,
                               pt.d_table(), pt.d_poses(), (const unsigned char*)ts.t_mask.as<unsigned char>(), cam,
                               t.obs.as<msfm_ref::Obs>());
            wrote(hipGetLastError());
        }
    }
    if (queued == hipSuccess) wrote(hipEventRecord(ev[1], st));
    if (T > 0 && O > 0 && queued == hipSuccess) {
        hipLaunchKernelGGL(flt_track_kernel, dim3(grid), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(),
                           (const unsigned char*)ts.r_cons.as<unsigned char>(), (int)T, t.obs.as<msfm_ref::Obs>(), pt.d_poses(),
                           n_images > 0 ? (const unsigned char*)d_scope : (const unsigned char*)nullptr, (cam.fx + cam.fy) / 2.0, flt,
                           msfm_ref::Verdict{prm.max_error, prm.min_angle}, ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(),
                           ts.t_mask.as<unsigned char>(), t.counters.as<FltCounters>());
        wrote(hipGetLastError());
    }
    if (queued == hipSuccess) wrote(hipEventRecord(ev[2], st));
    const hipError_t done = hipStreamSynchronize(st);   // (before anything returns: the temporaries die with this function)
    wrote(done);
    if (queued != hipSuccess) ts.tri_valid = ts.mask_valid = false;   // (the records and the bytes may be half rewritten)
    HIPCHK(ctx, queued);
    ts.mask_valid = true;
    FltCounters hc = {};
    HIPCHK(ctx, hipMemcpy(&hc, t.counters.p, sizeof(hc), hipMemcpyDeviceToHost));
    float prep_ms = 0.f, all_ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&prep_ms, ev[0], ev[1]));
    HIPCHK(ctx, hipEventElapsedTime(&all_ms, ev[0], ev[2]));
    msfm_filter_stats s = {};
    s.eligible = (int64_t)hc.eligible;
    s.dropped_by_depth = (int64_t)hc.dropped_by_depth;
    s.dropped_by_error = (int64_t)hc.dropped_by_error;
    s.trimmed = (int64_t)hc.trimmed;
    s.regained = (int64_t)hc.regained;
    s.removed_by_views = (int64_t)hc.removed_by_views;
    s.removed_by_angle = (int64_t)hc.removed_by_angle;
    s.succeeded = (int64_t)hc.succeeded;
    s.observations_used = (int64_t)hc.observations_used;
    s.filter_ms = all_ms;
    s.prepare_ms = prep_ms;
    if (stats) *stats = s;
    return MSFM_OK;
}

}  // namespace
