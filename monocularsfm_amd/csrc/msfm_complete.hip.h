// msfm_complete.hip.h -- map completion on the device (include/msfm_match.h "map completion"): the kernel and the
// host side of msfm_complete_points (defined in msfm_match.hip).  The arithmetic is msfm_complete.h, shared with the host twin
// CompletePoints: the same bits.  Included by msfm_match.hip behind msfm_filter.hip.h; like it, it launches msfm_extend.hip.h's
// ext_mask_kernel and msfm_refine.hip.h's ref_obs_kernel unchanged.
//
// Everything runs on the library's stream between HIP events; the host waits once, at the end.
//   ext_mask_kernel    (msfm_extend.hip.h) with an all-zero `gained`; launched only on a session without inlier bytes.
//   ref_obs_kernel     (msfm_refine.hip.h) under the session's pose table and the current bytes.
//   cmp_track_kernel   one lane per kept track, a wave-uniform grid-stride loop, 256 threads, no LDS, the shape of flt_track_kernel.
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
    HIPCHK(ctx, t.counters.ensure(sizeof(CmpCounters)));
    HIPCHK(ctx, t.obs.ensure((size_t)std::max<long long>(1, O) * sizeof(msfm_ref::Obs)));
    HIPCHK(ctx, ts.t_mask.ensure((size_t)std::max<long long>(1, O)));
    HIPCHK(ctx, pt.upload(ts.tri_camera, by_rank, table, n_img));
    // (synchronous copies of the small tables: nothing queued reads host memory that an early return below would free)
    unsigned char* d_scope = t.bytes.as<unsigned char>();
    unsigned char* d_gained = d_scope + scope.size();
    HIPCHK(ctx, hipMemcpy(d_scope, scope.data(), scope.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(d_gained, gained.data(), gained.size(), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemsetAsync(t.counters.p, 0, sizeof(CmpCounters), st));
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
        hipLaunchKernelGGL(cmp_track_kernel, dim3(grid), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(),
                           (const unsigned char*)ts.r_cons.as<unsigned char>(), (int)T, t.obs.as<msfm_ref::Obs>(), pt.d_poses(),
                           n_images > 0 ? (const unsigned char*)d_scope : (const unsigned char*)nullptr, (cam.fx + cam.fy) / 2.0, max_error,
                           msfm_ref::Verdict{prm.max_error, prm.min_angle}, ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(),
                           ts.t_mask.as<unsigned char>(), t.counters.as<CmpCounters>());
        wrote(hipGetLastError());
    }
    if (queued == hipSuccess) wrote(hipEventRecord(ev[2], st));
    const hipError_t done = hipStreamSynchronize(st);   // (before anything returns: the temporaries die with this function)
    wrote(done);
    if (queued != hipSuccess) ts.tri_valid = ts.mask_valid = false;   // (the records and the bytes may be half rewritten)
    HIPCHK(ctx, queued);
    ts.mask_valid = true;
    CmpCounters hc = {};
    HIPCHK(ctx, hipMemcpy(&hc, t.counters.p, sizeof(hc), hipMemcpyDeviceToHost));
    float prep_ms = 0.f, all_ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&prep_ms, ev[0], ev[1]));
    HIPCHK(ctx, hipEventElapsedTime(&all_ms, ev[0], ev[2]));
    msfm_complete_stats s = {};
    s.eligible = (int64_t)hc.eligible;
    s.candidates = (int64_t)hc.candidates;
    s.admitted = (int64_t)hc.admitted;
    s.rejected_by_depth = (int64_t)hc.rejected_by_depth;
    s.rejected_by_error = (int64_t)hc.rejected_by_error;
    s.completed = (int64_t)hc.completed;
    s.succeeded = (int64_t)hc.succeeded;
    s.observations_used = (int64_t)hc.observations_used;
    s.complete_ms = all_ms;
    s.prepare_ms = prep_ms;
    if (stats) *stats = s;
    return MSFM_OK;
}

}  // namespace
