// msfm_align.hip.h -- map alignment on the device (include/msfm_match.h "map alignment"): the two kernels and the
// host side of msfm_estimate_alignment / msfm_transform_map (defined in msfm_match.hip).  The arithmetic is msfm_align.h, shared with the
// host twins EstimateAlignment / TransformMap: the same bits.  Included by msfm_match.hip behind msfm_visibility.hip.h; it reuses
// ref_obs_kernel beside PoseTables, tri_tables and wave_add_counters.
//
//   aln_estimate_kernel  ONE workgroup of 256 threads: it is one problem, and a second workgroup would only add a reduction.  The priors
//                        (camera centre and position, 48 bytes each; the centres computed on the host by msfm_tri::centre -- the same
//                        header, the same bits) are uploaded with the call.  Rounds of 256 hypotheses, one per lane: the sample's fit
//                        stays in registers (every Jacobi index is a compile-time constant), the priors pass through LDS in tiles of
//                        kAlnTile = 256 (12 KiB) and every lane counts from broadcast reads; the round's counts go to an LDS array and
//                        every thread replays the stopping rule over the counts so far.  Winner, refits and the final errors: EVERY
//                        thread runs msfm_aln::estimate on the same bits, so the control flow is uniform over the workgroup (the
//                        arrangement of tv_refine_kernel); the sums are workgroup reductions through LDS in the stated order, the
//                        counts integer adds.  Every loop bound is a data-independent cap: max_hypotheses <= 4096, kRefits, sample3
//                        with m >= 3.
//   aln_track_kernel     one lane per kept track, wave-uniform grid-stride loop, 256 threads, no LDS (the shape of flt_track_kernel):
//                        msfm_aln::align_track for every record with ATTEMPTED | POINT, behind PoseTables::upload / prepare of the NEW
//                        poses and ref_obs_kernel.  Its counters go through wave_add_counters.
// Plain vector loads and stores only; no floating-point atomics; no inline assembly; no graph capture; one host wait per call.
#pragma once
#include "msfm_align.h"
#include "msfm_refine_camera.hip.h"

namespace msfm {

constexpr int kAlnThreads = msfm_aln::kAlnRound;
constexpr int kAlnSumsMax = 10;   // the widest reduced pass (M and va)

struct AlnCounters {
    unsigned long long transformed, lost, gained, succeeded;
};

// the reduced passes of msfm_aln::estimate on the device; every thread of the workgroup calls every member
struct AlnDevicePriors {
    const msfm_aln::Prior* priors;   // global
    int n, tid;
    msfm_aln::Prior* s_tile;         // kAlnTile priors of LDS
    double* s_red;                   // kAlnSumsMax * kAlnThreads doubles of LDS
    int* s_counts;                   // kMaxHypotheses ints of LDS
    int* s_int;                      // 2 * kAlnThreads ints of LDS
    msfm_alignment_residual* records;

    __device__ __forceinline__ int m() const { return n; }
    __device__ __forceinline__ msfm_aln::Prior prior(int k) const { return priors[k]; }

    template <int K, class F>
    __device__ __forceinline__ void sum(F term, double out[K]) const {
        static_assert(K <= kAlnSumsMax, "s_red holds kAlnSumsMax arrays of partials");
        double part[K];
#pragma unroll
        for (int j = 0; j < K; ++j) part[j] = 0.0;
        for (int k = tid; k < n; k += kAlnThreads) {
            double v[K];
            if (!term(k, v)) continue;
#pragma unroll
            for (int j = 0; j < K; ++j) part[j] = part[j] + v[j];
        }
#pragma unroll
        for (int j = 0; j < K; ++j) s_red[j * kAlnThreads + tid] = part[j];
        __syncthreads();
        for (int s = kAlnThreads / 2; s >= 1; s >>= 1) {
            if (tid < s)
#pragma unroll
                for (int j = 0; j < K; ++j) s_red[j * kAlnThreads + tid] = s_red[j * kAlnThreads + tid] + s_red[j * kAlnThreads + tid + s];
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < K; ++j) out[j] = s_red[j * kAlnThreads];
        __syncthreads();   // (s_red is rewritten by the next pass)
    }

    template <class F>
    __device__ __forceinline__ void count(F term, int* out) const {
        int c[2] = {0, 0};
        for (int k = tid; k < n; k += kAlnThreads) term(k, c);
        s_int[tid] = c[0];
        s_int[kAlnThreads + tid] = c[1];
        __syncthreads();
        for (int s = kAlnThreads / 2; s >= 1; s >>= 1) {
            if (tid < s) {
                s_int[tid] += s_int[tid + s];
                s_int[kAlnThreads + tid] += s_int[kAlnThreads + tid + s];
            }
            __syncthreads();
        }
        out[0] = s_int[0];
        out[1] = s_int[kAlnThreads];
        __syncthreads();
    }

    __device__ __forceinline__ void score(int round, unsigned long long seed, const msfm_aln::Params& prm) const {
        const int it = round * kAlnThreads + tid;
        const bool active = it < prm.max_hypotheses;
        msfm_similarity g;
        bool valid = false;
        if (active) valid = msfm_aln::hypothesis([&](int k) { return priors[k]; }, n, seed, it, &g);
        int c = 0;
        for (int base = 0; base < n; base += msfm_aln::kAlnTile) {   // (uniform over the workgroup)
            __syncthreads();   // (every lane has finished the tile before)
            if (tid < msfm_aln::kAlnTile && base + tid < n) s_tile[tid] = priors[base + tid];
            __syncthreads();
            const int nt = n - base < msfm_aln::kAlnTile ? n - base : msfm_aln::kAlnTile;
            if (valid)
                for (int j = 0; j < nt; ++j) c += msfm_aln::prior_error(g, s_tile[j]) <= prm.max_error ? 1 : 0;
        }
        if (active) s_counts[it] = valid ? c : 0;
        __syncthreads();
    }
    __device__ __forceinline__ int count_at(int it) const { return s_counts[it]; }
    __device__ __forceinline__ void store(int k, int flags, double error) const { records[k] = msfm_alignment_residual{flags, 0, error}; }
};

__global__ __launch_bounds__(kAlnThreads) void aln_estimate_kernel(const msfm_aln::Prior* __restrict__ priors, int m, msfm_aln::Params prm,
                                                                   msfm_alignment* __restrict__ out,
                                                                   msfm_alignment_residual* __restrict__ records) {
    __shared__ msfm_aln::Prior s_tile[msfm_aln::kAlnTile];
    __shared__ double s_red[kAlnSumsMax * kAlnThreads];
    __shared__ int s_counts[msfm_aln::kMaxHypotheses];
    __shared__ int s_int[2 * kAlnThreads];
    const AlnDevicePriors pv{priors, m, (int)threadIdx.x, s_tile, s_red, s_counts, s_int, records};
    msfm_alignment a;
    msfm_aln::estimate(pv, prm, &a);
    if (threadIdx.x == 0) *out = a;
}

__global__ __launch_bounds__(256) void aln_track_kernel(const long long* __restrict__ offsets, int T, const msfm_ref::Obs* __restrict__ obs,
                                                        const msfm_tri::Pose* __restrict__ poses, double f, msfm_ref::Verdict vd,
                                                        msfm_similarity g, msfm_point3d* __restrict__ points, double* __restrict__ residuals,
                                                        AlnCounters* __restrict__ counters) {
    unsigned long long c[4] = {0, 0, 0, 0};
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); t0 < T; t0 += stride) {   // (uniform over the wave)
        const long long t = t0 + lane;
        if (t >= T) continue;
        msfm_point3d r = points[t];
        if (msfm_ref::eligible(r)) {
            const long long b = offsets[t], e = offsets[t + 1];
            msfm_aln::Tally tl;
            msfm_aln::align_track(obs + b, (int)(e - b), poses, f, vd, g, &r, residuals + b, &tl);
            points[t] = r;
            c[0] += (unsigned long long)tl.transformed;
            c[1] += (unsigned long long)tl.lost;
            c[2] += (unsigned long long)tl.gained;
        }
        c[3] += msfm_rp::succeeded(r) ? 1 : 0;
    }
    wave_add_counters(c, &counters->transformed);
}

}  // namespace msfm

namespace {

int estimate_alignment_impl(msfm_ctx* ctx, const int32_t* image_ids, const double* positions, int n, const msfm_alignment_params* params,
                            msfm_alignment* out, msfm_alignment_residual* out_per_prior) {
    const TrackSession& ts = ctx->tracks;   // (read-only: nothing of the session is written)
    const std::string who = "msfm_estimate_alignment";
    if (const int rc = tri_session_check(ctx, who, true)) return rc;
    msfm_aln::Params prm = {0.0, 0.9999, 0, 3};   // NULL: least squares
    if (params) prm = msfm_aln::Params{params->max_error, params->confidence, params->max_hypotheses, params->min_inliers};
    if (!out) return fail(ctx, MSFM_E_INVALID, who + ": NULL out");
    if (n < 0 || (n > 0 && (!image_ids || !positions))) return fail(ctx, MSFM_E_INVALID, who + ": bad list of priors");
    if (prm.max_hypotheses < 0 || prm.max_hypotheses > msfm_aln::kMaxHypotheses)
        return fail(ctx, MSFM_E_INVALID, who + ": max_hypotheses must lie in 0 .. 4096");
    if (prm.max_hypotheses > 0 && !(std::isfinite(prm.max_error) && prm.max_error > 0.0))
        return fail(ctx, MSFM_E_INVALID, who + ": max_error must be finite and positive");
    if (!(prm.confidence > 0.0 && prm.confidence < 1.0)) return fail(ctx, MSFM_E_INVALID, who + ": confidence must lie in (0, 1)");
    std::vector<unsigned char> listed;
    if (const int rc = rank_bytes(ctx, image_ids, n, who + ": image not declared in the session: ", who + ": an image is given twice: ", &listed))
        return rc;
    for (long long k = 0; k < 3LL * n; ++k)
        if (!std::isfinite(positions[k])) return fail(ctx, MSFM_E_INVALID, who + ": non-finite position of image " + std::to_string(image_ids[k / 3]));
    // the centre of every rank with a valid pose
    const int n_img = (int)ts.nd.ids.size();
    std::vector<msfm_tri::Pose> by_rank((size_t)std::max(n_img, 1));
    for (auto& p : by_rank) p.valid = 0;
    for (size_t k = 0; k < ts.tri_ids.size(); ++k) msfm_tri::prepare_pose(ts.tri_poses[k], &by_rank[(size_t)ts.rank_of[(size_t)ts.tri_ids[k]]]);
    std::vector<msfm_aln::Prior> priors;
    std::vector<int> at;   // the list position of each usable prior
    for (int k = 0; k < n; ++k) {
        const msfm_tri::Pose& p = by_rank[(size_t)ts.rank_of[(size_t)image_ids[k]]];
        if (!p.valid) continue;
        priors.push_back(msfm_aln::Prior{{p.O[0], p.O[1], p.O[2]}, {positions[3 * k], positions[3 * k + 1], positions[3 * k + 2]}});
        at.push_back(k);
    }
    const int m = (int)priors.size();
    msfm_alignment a;
    msfm_aln::clear_alignment(&a, m);
    std::vector<msfm_alignment_residual> used((size_t)std::max(m, 1), msfm_alignment_residual{MSFM_ALN_USED, 0, -1.0});
    float ms = 0.f;
    if (m >= 3) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        TmpBuf d_priors, d_out, d_records;   // (the temporaries are freed when the call returns, whatever it returns)
        TmpEvents<2> ev;
        hipStream_t st = store_stream(ctx);
        HIPCHK(ctx, ev.create());
        HIPCHK(ctx, d_priors.ensure((size_t)m * sizeof(msfm_aln::Prior)));
        HIPCHK(ctx, d_out.ensure(sizeof(msfm_alignment)));
        HIPCHK(ctx, d_records.ensure((size_t)m * sizeof(msfm_alignment_residual)));
        HIPCHK(ctx, hipMemcpy(d_priors.p, priors.data(), (size_t)m * sizeof(msfm_aln::Prior), hipMemcpyHostToDevice));   // (synchronous)
        HIPCHK(ctx, hipEventRecord(ev[0], st));
        hipLaunchKernelGGL(msfm::aln_estimate_kernel, dim3(1), dim3(msfm::kAlnThreads), 0, st, (const msfm_aln::Prior*)d_priors.as<msfm_aln::Prior>(),
                           m, prm, d_out.as<msfm_alignment>(), d_records.as<msfm_alignment_residual>());
        hipError_t queued = hipGetLastError();
        if (queued == hipSuccess) queued = hipEventRecord(ev[1], st);
        const hipError_t done = hipStreamSynchronize(st);   // (before anything returns: the temporaries die with this function)
        HIPCHK(ctx, queued);
        HIPCHK(ctx, done);
        HIPCHK(ctx, hipMemcpy(&a, d_out.p, sizeof(a), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(used.data(), d_records.p, (size_t)m * sizeof(msfm_alignment_residual), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
    }
    a.n_listed = n;
    a.estimate_ms = ms;
    *out = a;
    if (out_per_prior) {
        for (int k = 0; k < n; ++k) out_per_prior[k] = msfm_alignment_residual{0, 0, -1.0};
        for (int j = 0; j < m; ++j) out_per_prior[at[(size_t)j]] = used[(size_t)j];
    }
    return MSFM_OK;
}

int transform_map_impl(msfm_ctx* ctx, const msfm_similarity* similarity, msfm_transform_stats* stats) {
    TrackSession& ts = ctx->tracks;
    const std::string who = "msfm_transform_map";
    if (const int rc = tri_session_check(ctx, who, true)) return rc;
    if (!similarity) return fail(ctx, MSFM_E_INVALID, who + ": NULL similarity");
    const msfm_similarity g = *similarity;
    if (!msfm_aln::similarity_ok(g))
        return fail(ctx, MSFM_E_INVALID, who + ": s must be finite and positive, d finite, Q a proper rotation (max |Q Q^T - I| <= 1e-9)");
    const int n_list = (int)ts.tri_ids.size();
    std::vector<msfm_pose_rt> moved = ts.tri_poses;   // (TransformPoses of the twin)
    long long n_moved = 0;
    for (int k = 0; k < n_list; ++k) {
        msfm_tri::Pose p;
        msfm_tri::prepare_pose(ts.tri_poses[(size_t)k], &p);
        if (!p.valid) continue;
        if (!msfm_aln::transform_pose(g, ts.tri_poses[(size_t)k].R, ts.tri_poses[(size_t)k].t, moved[(size_t)k].R, moved[(size_t)k].t))
            return fail(ctx, MSFM_E_INVALID, who + ": a transformed pose would not be finite");
        n_moved += 1;
    }
    std::vector<msfm_pose_rt> by_rank;
    std::vector<TriImage> table;
    if (const int rc = tri_tables(ctx, who, &ts.tri_camera, ts.tri_ids.data(), moved.data(), n_list,
                                  msfm_tri::Params{ts.tri_prm.max_error, ts.tri_prm.min_angle, ts.tri_prm.min_views, 0}, &by_rank, &table))
        return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long T = ts.stats.tracks_kept, O = ts.stats.observations_kept;
    PoseTables pt;   // (the temporaries are freed when the call returns, whatever it returns)
    TmpBuf counters, obs;
    TmpEvents<2> ev;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, ev.create());
    HIPCHK(ctx, counters.ensure(sizeof(msfm::AlnCounters)));
    HIPCHK(ctx, obs.ensure((size_t)std::max<long long>(1, O) * sizeof(msfm_ref::Obs)));
    HIPCHK(ctx, pt.upload(ts.tri_camera, by_rank, table, (int)ts.nd.ids.size()));
    HIPCHK(ctx, hipMemsetAsync(counters.p, 0, sizeof(msfm::AlnCounters), st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    HIPCHK(ctx, pt.prepare(st));
    // (up to here a failure returns with the session exactly as it was: only temporaries have been touched)
    // from here on the registrations and the pose refinement's records are gone: they hold poses of the old frame
    ts.reg_valid = ts.rp_valid = false;
    hipError_t queued = hipSuccess;   // from the first launch that writes the session on, the call waits before it fails
    const bool work = T > 0 && O > 0;
    if (work) {
        queued = launch_ref_obs(ctx, pt, ts.mask_valid ? ts.t_mask.as<unsigned char>() : nullptr, obs.as<msfm_ref::Obs>(), st);
        if (queued == hipSuccess) {
            hipLaunchKernelGGL(msfm::aln_track_kernel, dim3(tk_grid(ctx, T)), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(), (int)T,
                               (const msfm_ref::Obs*)obs.as<msfm_ref::Obs>(), pt.d_poses(), (pt.cam.fx + pt.cam.fy) / 2.0,
                               msfm_ref::Verdict{ts.tri_prm.max_error, ts.tri_prm.min_angle}, g, ts.t_points.as<msfm_point3d>(),
                               ts.t_resid.as<double>(), counters.as<msfm::AlnCounters>());
            queued = hipGetLastError();
        }
    }
    if (queued == hipSuccess) queued = hipEventRecord(ev[1], st);
    const hipError_t done = hipStreamSynchronize(st);   // (before anything returns: the temporaries die with this function)
    msfm::AlnCounters hc = {};
    hipError_t back = (queued == hipSuccess && done == hipSuccess) ? hipMemcpy(&hc, counters.p, sizeof(hc), hipMemcpyDeviceToHost) : hipSuccess;
    if ((queued != hipSuccess || done != hipSuccess || back != hipSuccess) && work)
        ts.tri_valid = ts.mask_valid = false;   // (the records may be half rewritten, under poses the session does not have)
    HIPCHK(ctx, queued);
    HIPCHK(ctx, done);
    HIPCHK(ctx, back);
    ts.tri_poses.swap(moved);   // the new poses replace the session's
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
    msfm_transform_stats s = {};
    s.poses_transformed = n_moved;
    s.points_transformed = (int64_t)hc.transformed;
    s.points_lost = (int64_t)hc.lost;
    s.points_gained = (int64_t)hc.gained;
    s.succeeded = (int64_t)hc.succeeded;
    s.transform_ms = ms;
    if (stats) *stats = s;
    return MSFM_OK;
}

}  // namespace
