// msfm_refine.hip.h -- point refinement on the device (include/msfm_match.h "point refinement"): the two kernels
// and the host side of msfm_refine_points (defined in msfm_match.hip).  The arithmetic is msfm_refine.h, shared with the host twin
// RefinePoints: the same bits.  Included by msfm_match.hip behind msfm_triangulate_robust.hip.h, whose PoseTables, tri_tables and
// wave_add_counters it reuses.
//
// Everything runs on the library's stream between HIP events; the host waits once, at the end.
//   ref_obs_kernel     one lane per kept OBSERVATION, grid-stride: the dependent gather of tri_track_kernel (CSR element -> image table
//                      -> keypoint + the pose's valid flag) is walked ONCE per observation, fully parallel, and leaves a 24-byte
//                      msfm_ref::Obs aligned with the track CSR: undistorted (u, v), the pose rank, USED / FIT.  It does not look at
//                      the records: observations of tracks that are not eligible are resolved too and never read.
//   ref_track_kernel   one lane per kept track, grid-stride, 256 threads, no LDS; lanes of tracks that are not eligible fall through.
//                      A lane reads only its track's Obs and the prepared poses; H, g, the Cholesky factor and X live in registers
//                      (every index is a compile-time constant), lanes leave the LM loop individually.  The five counters go through
//                      wave_add_counters; the two cost sums are reduced per
//                      wave by the same fixed shuffle tree and STORED per wave (no floating-point atomics: the host adds the waves'
//                      sums in wave order).
// Plain vector loads and stores only.
#pragma once
#include "msfm_refine.h"
#include "msfm_triangulate_robust.hip.h"

namespace msfm {

struct RefCounters {
    unsigned long long eligible, refined, gained_error_ok, rejected_by_verdict, iterations;
};
constexpr int kRefCounters = 5;

__global__ __launch_bounds__(256) void ref_obs_kernel(const int* __restrict__ img, const int* __restrict__ idx, long long O,
                                                      const TriImage* __restrict__ table, const msfm_tri::Pose* __restrict__ poses,
                                                      const unsigned char* __restrict__ mask, msfm_emat::Camera cam,
                                                      msfm_ref::Obs* __restrict__ obs) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < O; o += stride) {
        const TriImage im = table[img[o]];   // (a track's images are declared: rank >= 0)
        const msfm_tri::Pose* p = poses[im.rank].valid ? poses + im.rank : nullptr;
        double x = 0.0, y = 0.0;
        if (p) {
            const float2 q = im.kxy[idx[o]];
            x = (double)q.x;
            y = (double)q.y;
        }
        msfm_ref::prepare_obs(p, im.rank, x, y, mask ? mask[o] != 0 : true, cam, obs + o);
    }
}

__global__ __launch_bounds__(256) void ref_track_kernel(const long long* __restrict__ offsets, int T, const msfm_ref::Obs* __restrict__ obs,
                                                        const msfm_tri::Pose* __restrict__ poses, double f, msfm_ref::Verdict vd,
                                                        msfm_ref::Params prm, msfm_point3d* __restrict__ points,
                                                        double* __restrict__ residuals, RefCounters* __restrict__ counters,
                                                        double* __restrict__ wave_costs) {
    unsigned long long c[kRefCounters] = {0, 0, 0, 0, 0};
    double before = 0.0, after = 0.0;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        msfm_point3d r = points[t];
        if (!msfm_ref::eligible(r)) continue;
        const long long b = offsets[t], e = offsets[t + 1];
        msfm_ref::Tally tl;
        msfm_ref::refine_track(obs + b, (int)(e - b), poses, f, vd, prm, &r, residuals + b, &tl, nullptr);
        if (tl.refined) points[t] = r;
        c[0] += 1;
        c[1] += (unsigned long long)tl.refined;
        c[2] += (unsigned long long)tl.gained_error_ok;
        c[3] += (unsigned long long)tl.rejected_by_verdict;
        c[4] += (unsigned long long)tl.iterations;
        before = before + tl.cost_before;
        after = after + tl.cost_after;
    }
    wave_add_counters(c, reinterpret_cast<unsigned long long*>(counters));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {   // (the cost sums: a fixed tree and a store per wave, no floating-point atomics)
        before = before + __shfl_down(before, d, 64);
        after = after + __shfl_down(after, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
        wave_costs[2 * wave] = before;
        wave_costs[2 * wave + 1] = after;
    }
}

}  // namespace msfm

namespace {

// ref_obs_kernel over the session's kept observations (there are some) under the pose tables of a call; mask: the inlier bytes, or
// nullptr on a plain session
hipError_t launch_ref_obs(msfm_ctx* ctx, const PoseTables& pt, const unsigned char* mask, msfm_ref::Obs* obs, hipStream_t st) {
    const TrackSession& ts = ctx->tracks;
    const long long O = ts.stats.observations_kept;
    hipLaunchKernelGGL(ref_obs_kernel, dim3(tk_grid(ctx, O)), dim3(256), 0, st, (const int*)ts.r_img.as<int>(), (const int*)ts.r_idx.as<int>(), O,
                       pt.d_table(), pt.d_poses(), mask, pt.cam, obs);
    return hipGetLastError();
}

int refine_impl(msfm_ctx* ctx, const msfm_refine_params* params, msfm_refine_stats* stats) {
    TrackSession& ts = ctx->tracks;
    const std::string who = "msfm_refine_points";
    if (const int rc = tri_session_check(ctx, who, true)) return rc;
    msfm_ref::Params prm = {1e-10, 10, 0};
    if (params) prm = msfm_ref::Params{params->step_tol, params->max_iters, 0};
    if (prm.max_iters < 0 || prm.max_iters > 100) return fail(ctx, MSFM_E_INVALID, who + ": max_iters must lie in 0 .. 100");
    if (!std::isfinite(prm.step_tol) || prm.step_tol < 0.0) return fail(ctx, MSFM_E_INVALID, who + ": step_tol must be finite and not negative");
    // from here on the registrations and the pose refinement's records are gone: they describe the points as they were (DESIGN.md,
    // the flag table of section 15)
    ts.reg_valid = ts.rp_valid = false;
    const bool had_mask = ts.mask_valid;
    std::vector<msfm_pose_rt> by_rank;
    std::vector<TriImage> table;
    if (const int rc = tri_tables(ctx, who, &ts.tri_camera, ts.tri_ids.data(), ts.tri_poses.data(), (int)ts.tri_ids.size(),
                                  msfm_tri::Params{ts.tri_prm.max_error, ts.tri_prm.min_angle, ts.tri_prm.min_views, 0}, &by_rank, &table))
        return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long T = ts.stats.tracks_kept, O = ts.stats.observations_kept;
    PoseTables pt;   // (the temporaries are freed when the call returns, whatever it returns)
    TmpBuf counters, obs, wave_costs;
    TmpEvents<3> ev;
    hipStream_t st = store_stream(ctx);
    const unsigned grid = tk_grid(ctx, T);
    const size_t waves = (size_t)grid * 4;
    HIPCHK(ctx, ev.create());
    HIPCHK(ctx, counters.ensure(sizeof(RefCounters)));
    HIPCHK(ctx, obs.ensure((size_t)std::max<long long>(1, O) * sizeof(msfm_ref::Obs)));
    HIPCHK(ctx, wave_costs.ensure(2 * waves * sizeof(double)));
    HIPCHK(ctx, pt.upload(ts.tri_camera, by_rank, table, (int)ts.nd.ids.size()));
    HIPCHK(ctx, hipMemsetAsync(counters.p, 0, sizeof(RefCounters), st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    HIPCHK(ctx, pt.prepare(st));
    const msfm_emat::Camera cam = pt.cam;
    if (T > 0 && O > 0)
        HIPCHK(ctx, launch_ref_obs(ctx, pt, had_mask ? ts.t_mask.as<unsigned char>() : nullptr, obs.as<msfm_ref::Obs>(), st));
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    if (T > 0) {
        hipLaunchKernelGGL(ref_track_kernel, dim3(grid), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(), (int)T,
                           (const msfm_ref::Obs*)obs.as<msfm_ref::Obs>(), pt.d_poses(),
                           (cam.fx + cam.fy) / 2.0, msfm_ref::Verdict{ts.tri_prm.max_error, ts.tri_prm.min_angle}, prm,
                           ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(), counters.as<RefCounters>(), wave_costs.as<double>());
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ev[2], st));
    const hipError_t done = hipStreamSynchronize(st);   // (before anything returns: the temporaries die with this function)
    if (done != hipSuccess) ts.tri_valid = ts.mask_valid = false;   // (the records may be half rewritten)
    HIPCHK(ctx, done);
    RefCounters hc = {};
    HIPCHK(ctx, hipMemcpy(&hc, counters.p, sizeof(hc), hipMemcpyDeviceToHost));
    std::vector<double> costs(2 * waves, 0.0);
    if (T > 0) HIPCHK(ctx, hipMemcpy(costs.data(), wave_costs.p, costs.size() * sizeof(double), hipMemcpyDeviceToHost));
    float prep_ms = 0.f, all_ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&prep_ms, ev[0], ev[1]));
    HIPCHK(ctx, hipEventElapsedTime(&all_ms, ev[0], ev[2]));
    msfm_refine_stats s = {};
    s.eligible = (int64_t)hc.eligible;
    s.refined = (int64_t)hc.refined;
    s.gained_error_ok = (int64_t)hc.gained_error_ok;
    s.rejected_by_verdict = (int64_t)hc.rejected_by_verdict;
    s.iterations = (int64_t)hc.iterations;
    for (size_t w = 0; w < waves; ++w) {
        s.cost_before = s.cost_before + costs[2 * w];
        s.cost_after = s.cost_after + costs[2 * w + 1];
    }
    s.refine_ms = all_ms;
    s.prepare_ms = prep_ms;
    if (stats) *stats = s;
    return MSFM_OK;
}

}  // namespace
