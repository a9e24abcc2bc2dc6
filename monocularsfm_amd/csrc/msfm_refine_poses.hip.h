// msfm_refine_poses.hip.h -- pose refinement on the device (include/msfm_match.h "pose refinement"): the kernels and
// the host side of msfm_refine_poses / msfm_fetch_poses / msfm_fetch_pose_refinements (defined in msfm_match.hip).  The arithmetic is
// msfm_refine_poses.h, shared with the host twin RefinePoses: the same bits.  Included by msfm_match.hip behind msfm_refine.hip.h, whose
// ref_obs_kernel it reuses beside PoseTables, tri_tables and wave_add_counters.
//
// Everything runs on the library's stream between HIP events; the host waits once for the size of the image-major list and once at the
// end.
//   rp_key_kernel      one lane per kept OBSERVATION, grid-stride: a FIT observation in a candidate image (valid pose, not fixed) of a
//                      succeeded track gives the 64-bit key (pose rank << 32 | track number), every other one the key of a rank one past
//                      the last; the value is the observation's index.  The track number by bisection of the CSR offsets.
//   rocprim radix sort by key: the fitting set of every candidate image, images by rank, by ascending track number, compact at the front.
//   rp_offsets_kernel  one lane per rank: the lower bound of its first key.
//   rp_fill_kernel     one lane per list entry: (u, w) of the Obs and X of the record as a structure of arrays in list order.
//   rp_image_kernel    one wave per listed image, four waves per workgroup walking the pose list by grid stride.  Lane j holds partial
//                      j of the cost and of the 27 sums, the butterfly runs by cross-lane shuffles, after it every lane holds the same
//                      bits: the LM loop's control flow is wave-uniform.  The 6 x 6 system, R, t and delta are indexed by compile-time
//                      constants only.  Lane 0 writes the pose that stands into the pose table (its own entry: images are independent),
//                      the record and the rank's `changed` byte.  The four counters are wave-uniform: lane 0 adds each with one vector
//                      atomic per wave.  The costs are stored in the records; the host adds them in list order.
//   rp_verdict_kernel  one lane per kept track, grid-stride: a lane scans its track's Obs for a changed rank and falls through if
//                      there is none; otherwise the re-verdict under the new pose table.  Its three counters go through
//                      wave_add_counters.
// Plain vector loads and stores only; no LDS; no floating-point atomics.
#pragma once
#include "msfm_refine_poses.h"
#include "msfm_refine.hip.h"

namespace msfm {

enum { kRpCandidate = 1, kRpFixed = 2 };

struct RpImage {   // one listed image, in the pose list's order
    int rank, flags, image_id, pad;
};

struct RpCounters {
    unsigned long long eligible, refined, rejected_by_inliers, iterations, points_reposed, points_lost, points_gained;
};

__global__ __launch_bounds__(256) void rp_key_kernel(const long long* __restrict__ offsets, int T, long long O,
                                                     const msfm_ref::Obs* __restrict__ obs, const msfm_point3d* __restrict__ points,
                                                     const unsigned char* __restrict__ candidate, int n_ranks,
                                                     unsigned long long* __restrict__ keys, int* __restrict__ vals) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < O; o += stride) {
        const msfm_ref::Obs ob = obs[o];
        bool use = (ob.flags & msfm_ref::OBS_FIT) != 0 && candidate[ob.rank] != 0;   // (a FIT observation has a rank in [0, n_ranks))
        int tid = 0;
        if (use) {
            int lo = 0, hi = T - 1;   // the last track whose first observation is <= o
            while (lo < hi) {
                const int mid = (int)(((long long)lo + hi + 1) >> 1);
                if (offsets[mid] <= o) lo = mid;
                else hi = mid - 1;
            }
            tid = lo;
            use = msfm_rp::succeeded(points[tid]);
        }
        keys[o] = use ? (((unsigned long long)(unsigned)ob.rank << 32) | (unsigned long long)(unsigned)tid) : ((unsigned long long)n_ranks << 32);
        vals[o] = (int)o;
    }
}

__global__ __launch_bounds__(256) void rp_offsets_kernel(const unsigned long long* __restrict__ keys, long long O, int n_ranks,
                                                         long long* __restrict__ offsets) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_ranks) return;
    const unsigned long long key = (unsigned long long)j << 32;
    long long lo = 0, hi = O;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    offsets[j] = lo;
}

__global__ __launch_bounds__(256) void rp_fill_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ vals, long long M,
                                                      const msfm_ref::Obs* __restrict__ obs, const msfm_point3d* __restrict__ points,
                                                      double* __restrict__ cu, double* __restrict__ cw, double* __restrict__ cX,
                                                      double* __restrict__ cY, double* __restrict__ cZ) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        const int tid = (int)(unsigned)(keys[i] & 0xffffffffull);
        const msfm_ref::Obs ob = obs[vals[i]];
        cu[i] = ob.u;
        cw[i] = ob.w;
        cX[i] = points[tid].X[0];
        cY[i] = points[tid].X[1];
        cZ[i] = points[tid].X[2];
    }
}

// the three reduced passes of msfm_rp::refine_image over one image's list, by the wave that owns it (all 64 lanes active)
struct RpWaveEval {
    const double *cu, *cw, *cX, *cY, *cZ;
    int n, lane;
    double f, max_error;
    __device__ __forceinline__ double cost(const double R[9], const double t[3], bool* depth) const {
        bool d;
        double c = msfm_rp::lane_cost(R, t, cu, cw, cX, cY, cZ, n, lane, f, &d);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) c = c + __shfl_xor(c, s, 64);
        *depth = __ballot(!d) == 0ull;
        return c;
    }
    __device__ __forceinline__ void sums(const double R[9], const double t[3], double acc[msfm_reg::kRegSums]) const {
        msfm_rp::lane_sums(R, t, cu, cw, cX, cY, cZ, n, lane, acc);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
            for (int k = 0; k < msfm_reg::kRegSums; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], s, 64);
    }
    __device__ __forceinline__ int inliers(const double R[9], const double t[3]) const {
        int c = msfm_rp::lane_inliers(R, t, cu, cw, cX, cY, cZ, n, lane, f, max_error);
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s, 64);
        return c;
    }
};

__global__ __launch_bounds__(256) void rp_image_kernel(const RpImage* __restrict__ list, int n_list, const long long* __restrict__ offsets,
                                                       const double* __restrict__ cu, const double* __restrict__ cw,
                                                       const double* __restrict__ cX, const double* __restrict__ cY,
                                                       const double* __restrict__ cZ, double f, double max_error, msfm_rp::Params prm,
                                                       msfm_tri::Pose* __restrict__ poses, msfm_pose_refinement* __restrict__ records,
                                                       unsigned char* __restrict__ changed, RpCounters* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), waves = (int)((gridDim.x * blockDim.x) >> 6);
    unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int k = wave; k < n_list; k += waves) {   // (uniform over the wave)
        const RpImage im = list[k];
        msfm_pose_refinement rec;
        msfm_rp::clear_record(&rec, im.image_id);
        if (im.flags & kRpFixed) rec.status = MSFM_POSE_FIXED;
        if (im.flags & kRpCandidate) {
            const long long base = offsets[im.rank];
            const int n = (int)(offsets[im.rank + 1] - base);
            rec.n_observations = n;
            if (n >= prm.min_observations) {
                msfm_tri::Pose* p = poses + im.rank;
                double R[9], t[3];
#pragma unroll
                for (int q = 0; q < 9; ++q) R[q] = p->R[q];
#pragma unroll
                for (int q = 0; q < 3; ++q) t[q] = p->t[q];
                const RpWaveEval ev{cu + base, cw + base, cX + base, cY + base, cZ + base, n, lane, f, max_error};
                msfm_rp::Result res;
                msfm_rp::refine_image(ev, prm, R, t, &res, nullptr);
                msfm_rp::fill_record(&rec, res);
                if (res.stands && lane == 0) {
                    double O[3];
                    msfm_tri::centre(R, t, O);
#pragma unroll
                    for (int q = 0; q < 9; ++q) p->R[q] = R[q];
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        p->t[q] = t[q];
                        p->O[q] = O[q];
                    }
                    changed[im.rank] = 1;
                }
                c0 += 1;
                c1 += (unsigned long long)res.stands;
                c2 += (res.accepted > 0 && !res.stands) ? 1 : 0;
                c3 += (unsigned long long)res.iterations;
            }
        }
        if (lane == 0) records[k] = rec;
    }
    if (lane == 0) {
        if (c0) atomicAdd(&counters->eligible, c0);
        if (c1) atomicAdd(&counters->refined, c1);
        if (c2) atomicAdd(&counters->rejected_by_inliers, c2);
        if (c3) atomicAdd(&counters->iterations, c3);
    }
}

__global__ __launch_bounds__(256) void rp_verdict_kernel(const long long* __restrict__ offsets, int T, const msfm_ref::Obs* __restrict__ obs,
                                                         const msfm_tri::Pose* __restrict__ poses, const unsigned char* __restrict__ changed,
                                                         double f, msfm_ref::Verdict vd, msfm_point3d* __restrict__ points,
                                                         double* __restrict__ residuals, RpCounters* __restrict__ counters) {
    unsigned long long c[3] = {0, 0, 0};
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        msfm_point3d r = points[t];
        if (!msfm_ref::eligible(r)) continue;
        const long long b = offsets[t], e = offsets[t + 1];
        if (!msfm_rp::touches_changed(obs + b, (int)(e - b), changed)) continue;
        msfm_rp::Tally tl;
        msfm_rp::reverdict_track(obs + b, (int)(e - b), poses, f, vd, &r, residuals + b, &tl);
        points[t] = r;
        c[0] += (unsigned long long)tl.reposed;
        c[1] += (unsigned long long)tl.lost;
        c[2] += (unsigned long long)tl.gained;
    }
    wave_add_counters(c, &counters->points_reposed);
}

}  // namespace msfm

namespace {

int refine_poses_impl(msfm_ctx* ctx, const msfm_pose_refine_params* params, const int32_t* fixed_ids, int n_fixed,
                      msfm_pose_refine_stats* stats) {
    TrackSession& ts = ctx->tracks;
    const std::string who = "msfm_refine_poses";
    if (const int rc = tri_session_check(ctx, who, true)) return rc;
    msfm_rp::Params prm = {1e-6, 10, 15};
    if (params) prm = msfm_rp::Params{params->step_tol, params->max_iters, params->min_observations};
    if (prm.max_iters < 0 || prm.max_iters > 100) return fail(ctx, MSFM_E_INVALID, who + ": max_iters must lie in 0 .. 100");
    if (!std::isfinite(prm.step_tol) || prm.step_tol < 0.0) return fail(ctx, MSFM_E_INVALID, who + ": step_tol must be finite and not negative");
    if (prm.min_observations < 3) return fail(ctx, MSFM_E_INVALID, who + ": min_observations must be at least 3");
    if (n_fixed < 0 || (n_fixed > 0 && !fixed_ids)) return fail(ctx, MSFM_E_INVALID, who + ": bad list of fixed images");
    const int n_img = (int)ts.nd.ids.size();
    std::vector<unsigned char> fixed;
    if (const int rc = rank_bytes(ctx, fixed_ids, n_fixed, who + ": fixed image not declared in the session: ",
                                  who + ": a fixed image is given twice: ", &fixed))
        return rc;
    // from here on the registrations and the previous records are gone, as after msfm_refine_points
    ts.reg_valid = ts.rp_valid = false;
    const bool had_mask = ts.mask_valid;
    std::vector<msfm_pose_rt> by_rank;
    std::vector<TriImage> table;
    if (const int rc = tri_tables(ctx, who, &ts.tri_camera, ts.tri_ids.data(), ts.tri_poses.data(), (int)ts.tri_ids.size(),
                                  msfm_tri::Params{ts.tri_prm.max_error, ts.tri_prm.min_angle, ts.tri_prm.min_views, 0}, &by_rank, &table))
        return rc;
    const int n_list = (int)ts.tri_ids.size();
    std::vector<RpImage> list((size_t)std::max(n_list, 1), RpImage{0, 0, 0, 0});
    std::vector<unsigned char> candidate((size_t)std::max(n_img, 1), 0);
    for (int k = 0; k < n_list; ++k) {
        const int r = ts.rank_of[(size_t)ts.tri_ids[(size_t)k]];
        const bool cand = by_rank[(size_t)r].valid && !fixed[(size_t)r];
        candidate[(size_t)r] = cand ? 1 : 0;
        list[(size_t)k] = RpImage{r, (cand ? kRpCandidate : 0) | (fixed[(size_t)r] ? kRpFixed : 0), ts.tri_ids[(size_t)k], 0};
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long T = ts.stats.tracks_kept, O = ts.stats.observations_kept;
    if (O > 0x7fffffffLL) return fail(ctx, MSFM_E_CAPACITY, who + ": more than 2^31 - 1 kept observations");
    PoseTables pt;   // (the temporaries are freed when the call returns, whatever it returns)
    struct {
        TmpBuf counters, obs, list, candidate, changed, records, keys, keys2, vals, vals2, sort_tmp, offsets, cu, cw, cX, cY, cZ;
    } t;
    TmpEvents<3> ev;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, ev.create());
    const size_t N = (size_t)std::max(n_img, 1), L = (size_t)std::max(n_list, 1), Oz = (size_t)std::max<long long>(1, O);
    HIPCHK(ctx, t.counters.ensure(sizeof(RpCounters)));
    HIPCHK(ctx, t.obs.ensure(Oz * sizeof(msfm_ref::Obs)));
    HIPCHK(ctx, t.list.ensure(L * sizeof(RpImage)));
    HIPCHK(ctx, t.candidate.ensure(N));
    HIPCHK(ctx, t.changed.ensure(N));
    HIPCHK(ctx, t.records.ensure(L * sizeof(msfm_pose_refinement)));
    HIPCHK(ctx, t.keys.ensure(Oz * 8));
    HIPCHK(ctx, t.keys2.ensure(Oz * 8));
    HIPCHK(ctx, t.vals.ensure(Oz * 4));
    HIPCHK(ctx, t.vals2.ensure(Oz * 4));
    HIPCHK(ctx, t.offsets.ensure((N + 1) * 8));
    HIPCHK(ctx, pt.upload(ts.tri_camera, by_rank, table, n_img));
    // (synchronous copies of the small tables: nothing queued reads host memory that an early return below would free)
    HIPCHK(ctx, hipMemcpy(t.list.p, list.data(), L * sizeof(RpImage), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(t.candidate.p, candidate.data(), N, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemsetAsync(t.counters.p, 0, sizeof(RpCounters), st));
    HIPCHK(ctx, hipMemsetAsync(t.changed.p, 0, N, st));
    HIPCHK(ctx, hipMemsetAsync(t.offsets.p, 0, (N + 1) * 8, st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    HIPCHK(ctx, pt.prepare(st));
    const msfm_emat::Camera cam = pt.cam;
    const double f = (cam.fx + cam.fy) / 2.0;
    const msfm_ref::Obs* d_obs = t.obs.as<msfm_ref::Obs>();
    const msfm_point3d* d_points = ts.t_points.as<msfm_point3d>();
    const unsigned long long* keys2 = t.keys2.as<unsigned long long>();
    long long M = 0;
    if (T > 0 && O > 0) {
        HIPCHK(ctx, launch_ref_obs(ctx, pt, had_mask ? ts.t_mask.as<unsigned char>() : nullptr, t.obs.as<msfm_ref::Obs>(), st));
        hipLaunchKernelGGL(rp_key_kernel, dim3(tk_grid(ctx, O)), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(), (int)T, O, d_obs,
                           d_points, (const unsigned char*)t.candidate.as<unsigned char>(), n_img, t.keys.as<unsigned long long>(), t.vals.as<int>());
        HIPCHK(ctx, hipGetLastError());
        unsigned bits = 1;
        while (bits < 31 && (1ll << bits) <= (long long)n_img) ++bits;   // the rank one past the last sorts too
        size_t tmp_bytes = 0;
        HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, t.keys.as<unsigned long long>(), t.keys2.as<unsigned long long>(), t.vals.as<int>(),
                                              t.vals2.as<int>(), (size_t)O, 0u, 32u + bits, st));
        HIPCHK(ctx, t.sort_tmp.ensure(std::max<size_t>(tmp_bytes, 256)));
        HIPCHK(ctx, rocprim::radix_sort_pairs(t.sort_tmp.p, tmp_bytes, t.keys.as<unsigned long long>(), t.keys2.as<unsigned long long>(),
                                              t.vals.as<int>(), t.vals2.as<int>(), (size_t)O, 0u, 32u + bits, st));
        hipLaunchKernelGGL(rp_offsets_kernel, dim3((unsigned)((n_img + 256) / 256)), dim3(256), 0, st, keys2, O, n_img, t.offsets.as<long long>());
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&M, t.offsets.as<long long>() + n_img, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));   // the first wait: the size of the image-major list
    }
    const size_t Mz = (size_t)std::max<long long>(1, M);
    for (TmpBuf* b : {&t.cu, &t.cw, &t.cX, &t.cY, &t.cZ}) HIPCHK(ctx, b->ensure(Mz * 8));
    if (M > 0) {
        hipLaunchKernelGGL(rp_fill_kernel, dim3(tk_grid(ctx, M)), dim3(256), 0, st, keys2, (const int*)t.vals2.as<int>(), M, d_obs, d_points,
                           t.cu.as<double>(), t.cw.as<double>(), t.cX.as<double>(), t.cY.as<double>(), t.cZ.as<double>());
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    if (n_list > 0) {
        const unsigned groups = (unsigned)((n_list + 3) / 4);
        const unsigned grid = std::min<unsigned>(groups, 8u * (unsigned)std::max(1, ctx->cu_count));
        hipLaunchKernelGGL(rp_image_kernel, dim3(grid), dim3(256), 0, st, (const RpImage*)t.list.as<RpImage>(), n_list,
                           (const long long*)t.offsets.as<long long>(), (const double*)t.cu.as<double>(), (const double*)t.cw.as<double>(),
                           (const double*)t.cX.as<double>(), (const double*)t.cY.as<double>(), (const double*)t.cZ.as<double>(), f,
                           ts.tri_prm.max_error, prm, pt.poses.as<msfm_tri::Pose>(), t.records.as<msfm_pose_refinement>(),
                           t.changed.as<unsigned char>(), t.counters.as<RpCounters>());
        HIPCHK(ctx, hipGetLastError());
    }
    if (T > 0 && O > 0 && n_list > 0) {
        hipLaunchKernelGGL(rp_verdict_kernel, dim3(tk_grid(ctx, T)), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(), (int)T, d_obs,
                           pt.d_poses(), (const unsigned char*)t.changed.as<unsigned char>(), f,
                           msfm_ref::Verdict{ts.tri_prm.max_error, ts.tri_prm.min_angle}, ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(),
                           t.counters.as<RpCounters>());
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ev[2], st));
    const hipError_t done = hipStreamSynchronize(st);   // the second wait (before anything returns: the temporaries die with this function)
    if (done != hipSuccess) ts.tri_valid = ts.mask_valid = false;   // (the records may be half rewritten)
    HIPCHK(ctx, done);
    RpCounters hc = {};
    std::vector<msfm_pose_refinement> records(L);
    std::vector<msfm_tri::Pose> poses(N);
    std::vector<unsigned char> changed(N, 0);
    hipError_t back = hipMemcpy(&hc, t.counters.p, sizeof(hc), hipMemcpyDeviceToHost);
    if (back == hipSuccess && n_list > 0) back = hipMemcpy(records.data(), t.records.p, L * sizeof(msfm_pose_refinement), hipMemcpyDeviceToHost);
    if (back == hipSuccess && n_img > 0) back = hipMemcpy(poses.data(), pt.poses.p, N * sizeof(msfm_tri::Pose), hipMemcpyDeviceToHost);
    if (back == hipSuccess) back = hipMemcpy(changed.data(), t.changed.p, N, hipMemcpyDeviceToHost);
    if (back != hipSuccess) ts.tri_valid = ts.mask_valid = false;   // (the points may describe poses the session does not have)
    HIPCHK(ctx, back);
    float prep_ms = 0.f, all_ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&prep_ms, ev[0], ev[1]));
    HIPCHK(ctx, hipEventElapsedTime(&all_ms, ev[0], ev[2]));
    msfm_pose_refine_stats s = {};
    s.images = n_list;
    s.eligible = (int64_t)hc.eligible;
    s.refined = (int64_t)hc.refined;
    s.rejected_by_inliers = (int64_t)hc.rejected_by_inliers;
    s.iterations = (int64_t)hc.iterations;
    s.observations = M;
    s.points_reposed = (int64_t)hc.points_reposed;
    s.points_lost = (int64_t)hc.points_lost;
    s.points_gained = (int64_t)hc.points_gained;
    for (int k = 0; k < n_list; ++k) {
        s.cost_before = s.cost_before + records[(size_t)k].cost_before;
        s.cost_after = s.cost_after + records[(size_t)k].cost_after;
        const size_t r = (size_t)list[(size_t)k].rank;
        if (!changed[r]) continue;
        msfm_pose_rt& p = ts.tri_poses[(size_t)k];   // the pose that stands replaces the session's
        for (int q = 0; q < 9; ++q) p.R[q] = poses[r].R[q];
        for (int q = 0; q < 3; ++q) p.t[q] = poses[r].t[q];
    }
    s.refine_ms = all_ms;
    s.prepare_ms = prep_ms;
    records.resize((size_t)n_list);
    ts.rp_records.swap(records);
    ts.rp_valid = true;
    if (stats) *stats = s;
    return MSFM_OK;
}

int fetch_poses_impl(msfm_ctx* ctx, int32_t* out_ids, msfm_pose_rt* out_poses, int* n) {
    TrackSession& ts = ctx->tracks;
    if (!ts.open) return fail(ctx, MSFM_E_STATE, "msfm_fetch_poses without a track session (msfm_tracks_begin)");
    if (!ts.finished || !ts.tri_valid)
        return fail(ctx, MSFM_E_STATE, "msfm_fetch_poses without poses: msfm_triangulate_tracks has not run since the last msfm_tracks_finish");
    if (!n) return fail(ctx, MSFM_E_INVALID, "msfm_fetch_poses: NULL n");
    *n = (int)ts.tri_ids.size();
    if (out_ids) std::copy(ts.tri_ids.begin(), ts.tri_ids.end(), out_ids);
    if (out_poses) std::copy(ts.tri_poses.begin(), ts.tri_poses.end(), out_poses);
    return MSFM_OK;
}

int fetch_pose_refinements_impl(msfm_ctx* ctx, msfm_pose_refinement* out) {
    TrackSession& ts = ctx->tracks;
    if (!ts.open) return fail(ctx, MSFM_E_STATE, "msfm_fetch_pose_refinements without a track session (msfm_tracks_begin)");
    if (!ts.finished || !ts.tri_valid || !ts.rp_valid)
        return fail(ctx, MSFM_E_STATE, "msfm_fetch_pose_refinements without records: msfm_refine_poses was not the last call that rebuilt the session's pose tables");
    if (out) std::copy(ts.rp_records.begin(), ts.rp_records.end(), out);
    return MSFM_OK;
}

}  // namespace
