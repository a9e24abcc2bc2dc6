// msfm_refine_camera.hip.h -- camera refinement on the device (include/msfm_match.h "camera refinement"): the
// kernels and the host side of msfm_refine_camera / msfm_fetch_camera (defined in msfm_match.hip).  The arithmetic is
// msfm_refine_camera.h, shared with the host twin RefineCamera: the same bits.  Included by msfm_match.hip behind
// msfm_refine_poses.hip.h; it reuses ref_obs_kernel beside PoseTables, tri_tables and wave_add_counters.
//
// ONE problem whose 28 sums run over every contributing observation of the map.  The sums are reduced on the device in the order of
// msfm_refine_camera.h's summation paragraph, which the data fixes; the 6 x 6 solve and the LM control flow run on the HOST over
// msfm_rc::CameraProblem (literally the twin's code), with the launches behind RcDevEval::sums / ::cost and a copy of 30 words back:
// at most 2 max_iters + 2 small synchronisations per call (the first cost, per evaluated step at most one pass of sums and one of
// cost, the standing rule's count under the final camera), and one at the end.
//   rc_slot_kernel     one lane per kept track, grid-stride: msfm_rc::prepare_slot for every observation of the track -- the
//                      camera-independent half (raw pixel, reprojection, contributes / behind), once per call.
//   rc_sums_kernel     one lane per slot, one workgroup of 256 per chunk at a time, grid-stride over chunks: undistort, Jacobian, the
//                      28 contributions, the level-1 tree (the butterfly by cross-lane shuffles, the four waves through 896 bytes of
//                      LDS); writes [n_chunks][28].
//   rc_cost_kernel     the same with the cost alone, and the chunk's two integer counts (contributing, inliers).
//   rc_reduce_kernel   level 2, one workgroup per column (28 or 1), the two counts beside the first.
//   rc_verdict_kernel  one lane per kept track, grid-stride: the re-verdict of every eligible track under the new camera.
// The grid of rc_sums_kernel / rc_cost_kernel is capped at kRcGridPerCu workgroups per CU; a chunk's sum is stored at the chunk's own
// place, so which workgroup computed it -- hence the cap and the CU count -- reaches no bit.
// Plain vector loads and stores only; no floating-point atomics; the integer counters by one vector atomic per wave.
#pragma once
#include "msfm_refine_camera.h"
#include "msfm_refine_poses.hip.h"

namespace msfm {

constexpr unsigned kRcGridPerCu = 8;   // the grid cap of the two chunk kernels: 8 workgroups per CU

struct RcCounters {
    unsigned long long contributing, behind, recalibrated, lost, gained;
};

struct RcReduced {   // what one reduced pass leaves: 30 words
    double sums[msfm_rc::kSums];
    long long contributing, inliers;
};

__global__ __launch_bounds__(256) void rc_slot_kernel(const long long* __restrict__ offsets, const int* __restrict__ img,
                                                      const int* __restrict__ idx, int T, const TriImage* __restrict__ table,
                                                      const msfm_ref::Obs* __restrict__ obs, const msfm_tri::Pose* __restrict__ poses,
                                                      const msfm_point3d* __restrict__ points, msfm_rc::Slot* __restrict__ slots,
                                                      RcCounters* __restrict__ counters) {
    unsigned long long c[2] = {0, 0};
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        const msfm_point3d r = points[t];
        const bool standing = msfm_rp::succeeded(r);
        const long long b = offsets[t], e = offsets[t + 1];
        for (long long o = b; o < e; ++o) {
            const msfm_ref::Obs ob = obs[o];
            double px = 0.0, py = 0.0;
            if ((ob.flags & msfm_ref::OBS_FIT) && standing) {
                const float2 q = table[img[o]].kxy[idx[o]];
                px = (double)q.x;
                py = (double)q.y;
            }
            msfm_rc::Slot s;
            msfm_rc::prepare_slot(ob, standing, poses, r.X, px, py, &s);
            slots[o] = s;
            c[0] += (s.flags & msfm_rc::SLOT_IN) ? 1 : 0;
            c[1] += (s.flags & msfm_rc::SLOT_BEHIND) ? 1 : 0;
        }
    }
    wave_add_counters(c, &counters->contributing);
}

// the level-1 tree's first half: the butterfly over the 64 lanes of a wave (every lane ends with the same bits)
__device__ __forceinline__ double rc_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(256) void rc_sums_kernel(const msfm_rc::Slot* __restrict__ slots, long long O, int n_chunks,
                                                      msfm_emat::Camera cam, int mask, double* __restrict__ chunk_sums) {
    __shared__ double w[4][msfm_rc::kSums];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {   // (uniform over the workgroup)
        const long long s = (long long)c * msfm_rc::kChunk + threadIdx.x;
        msfm_rc::Slot sl = {0.0, 0.0, 0.0, 0.0, 0, 0};
        if (s < O) sl = slots[s];
        double acc[msfm_rc::kSums];
        msfm_rc::slot_sums(sl, cam, mask, acc);
#pragma unroll
        for (int k = 0; k < msfm_rc::kSums; ++k) {
            const double v = rc_wave_sum(acc[k]);
            if (lane == 0) w[wave][k] = v;
        }
        __syncthreads();
        if (threadIdx.x < msfm_rc::kSums) {
            const int k = threadIdx.x;
            chunk_sums[(long long)c * msfm_rc::kSums + k] = ((w[0][k] + w[1][k]) + w[2][k]) + w[3][k];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void rc_cost_kernel(const msfm_rc::Slot* __restrict__ slots, long long O, int n_chunks,
                                                      msfm_emat::Camera cam, double max_error, double* __restrict__ chunk_cost,
                                                      int* __restrict__ chunk_counts) {
    __shared__ double w[4];
    __shared__ int n[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {   // (uniform over the workgroup)
        const long long s = (long long)c * msfm_rc::kChunk + threadIdx.x;
        msfm_rc::Slot sl = {0.0, 0.0, 0.0, 0.0, 0, 0};
        if (s < O) sl = slots[s];
        int inlier;
        const double v = rc_wave_sum(msfm_rc::slot_cost(sl, cam, max_error, &inlier));
        const int in = __popcll(__ballot((sl.flags & msfm_rc::SLOT_IN) != 0)), good = __popcll(__ballot(inlier != 0));
        if (lane == 0) {
            w[wave] = v;
            n[wave][0] = in;
            n[wave][1] = good;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            chunk_cost[c] = ((w[0] + w[1]) + w[2]) + w[3];
            chunk_counts[2 * c] = n[0][0] + n[1][0] + n[2][0] + n[3][0];
            chunk_counts[2 * c + 1] = n[0][1] + n[1][1] + n[2][1] + n[3][1];
        }
        __syncthreads();
    }
}

// level 2: one workgroup of 256 per column (workgroup k reduces column k of in: [n_chunks][K] on its own, so the grid reaches no bit);
// counts (may be null): [n_chunks][2], added by workgroup 0
__global__ __launch_bounds__(256) void rc_reduce_kernel(const double* __restrict__ in, const int* __restrict__ counts, int n_chunks, int K,
                                                        int at, RcReduced* __restrict__ out) {
    __shared__ double w[4];
    __shared__ long long n[4][2];
    const int j = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = blockIdx.x;   // (< K: the grid is K workgroups)
    double p = 0.0;
    for (int c = j; c < n_chunks; c += msfm_rc::kChunk) p = p + in[(long long)c * K + k];
    const double v = rc_wave_sum(p);
    if (lane == 0) w[wave] = v;
    __syncthreads();
    if (j == 0) out->sums[at + k] = ((w[0] + w[1]) + w[2]) + w[3];
    if (counts && k == 0) {   // (uniform over the workgroup)
        long long a = 0, b = 0;
        for (int c = j; c < n_chunks; c += msfm_rc::kChunk) {
            a += counts[2 * c];
            b += counts[2 * c + 1];
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            a += __shfl_xor(a, m, 64);
            b += __shfl_xor(b, m, 64);
        }
        if (lane == 0) {
            n[wave][0] = a;
            n[wave][1] = b;
        }
        __syncthreads();
        if (j == 0) {
            out->contributing = n[0][0] + n[1][0] + n[2][0] + n[3][0];
            out->inliers = n[0][1] + n[1][1] + n[2][1] + n[3][1];
        }
    }
}

__global__ __launch_bounds__(256) void rc_verdict_kernel(const long long* __restrict__ offsets, int T, const msfm_ref::Obs* __restrict__ obs,
                                                         const msfm_tri::Pose* __restrict__ poses, double f, msfm_ref::Verdict vd,
                                                         msfm_point3d* __restrict__ points, double* __restrict__ residuals,
                                                         RcCounters* __restrict__ counters) {
    unsigned long long c[3] = {0, 0, 0};
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        msfm_point3d r = points[t];
        if (!msfm_ref::eligible(r)) continue;
        const long long b = offsets[t], e = offsets[t + 1];
        msfm_rc::Tally tl;
        msfm_rc::recalibrate_track(obs + b, (int)(e - b), poses, f, vd, &r, residuals + b, &tl);
        points[t] = r;
        c[0] += (unsigned long long)tl.recalibrated;
        c[1] += (unsigned long long)tl.lost;
        c[2] += (unsigned long long)tl.gained;
    }
    wave_add_counters(c, &counters->recalibrated);
}

}  // namespace msfm

namespace {

// The reduced passes of msfm_rc::refine_camera on the device.  A HIP error is kept in `err` and turns the pass into a NaN cost / zero
// sums (a rejected step): the caller looks at `err` after the loop.  The first evaluation is remembered: refine_camera asks for the
// contributing count, the starting cost and the old camera's inliers, which are one pass.
struct RcDevEval {
    hipStream_t st;
    const msfm_rc::Slot* slots;
    long long O;
    int n_chunks;
    unsigned grid;   // min(n_chunks, kRcGridPerCu * CUs)
    double max_error;
    int mask;
    double* chunk_sums;   // [n_chunks][28]
    double* chunk_cost;   // [n_chunks]
    int* chunk_counts;    // [n_chunks][2]
    RcReduced* reduced;   // device
    msfm_emat::Camera start;
    mutable hipError_t err = hipSuccess;
    mutable int passes = 0;
    mutable bool have_first = false;
    mutable RcReduced first = {};

    bool fetch(RcReduced* out) const {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out, reduced, sizeof(RcReduced), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        passes += 1;
        if (e != hipSuccess && err == hipSuccess) err = e;
        return e == hipSuccess;
    }
    bool run_cost(const msfm_emat::Camera& c, RcReduced* out) const {
        *out = RcReduced{};
        if (err != hipSuccess) return false;
        if (n_chunks == 0) return true;   // (nothing contributes: the cost of an empty set)
        hipLaunchKernelGGL(rc_cost_kernel, dim3(grid), dim3(256), 0, st, slots, O, n_chunks, c, max_error, chunk_cost, chunk_counts);
        hipLaunchKernelGGL(rc_reduce_kernel, dim3(1), dim3(256), 0, st, (const double*)chunk_cost, (const int*)chunk_counts, n_chunks, 1,
                           msfm_rc::kCost, reduced);
        return fetch(out);
    }
    const RcReduced& first_pass() const {
        if (!have_first) {
            (void)run_cost(start, &first);
            have_first = true;
        }
        return first;
    }
    static bool same(const msfm_emat::Camera& a, const msfm_emat::Camera& b) { return std::memcmp(&a, &b, sizeof a) == 0; }
    long long contributing() const { return first_pass().contributing; }
    double cost(const msfm_emat::Camera& c, long long* inliers) const {
        RcReduced r;
        if (same(c, start)) r = first_pass();
        else (void)run_cost(c, &r);
        *inliers = r.inliers;
        if (err != hipSuccess) return std::numeric_limits<double>::quiet_NaN();
        return r.sums[msfm_rc::kCost];
    }
    void sums(const msfm_emat::Camera& c, double acc[msfm_rc::kSums]) const {
        RcReduced r = {};
        if (err == hipSuccess && n_chunks > 0) {
            hipLaunchKernelGGL(rc_sums_kernel, dim3(grid), dim3(256), 0, st, slots, O, n_chunks, c, mask, chunk_sums);
            hipLaunchKernelGGL(rc_reduce_kernel, dim3(msfm_rc::kSums), dim3(256), 0, st, (const double*)chunk_sums, (const int*)nullptr, n_chunks,
                               msfm_rc::kSums, 0, reduced);
            (void)fetch(&r);
        }
        for (int k = 0; k < msfm_rc::kSums; ++k) acc[k] = r.sums[k];
    }
};

int refine_camera_impl(msfm_ctx* ctx, const msfm_camera_refine_params* params, msfm_camera_refine_stats* stats) {
    TrackSession& ts = ctx->tracks;
    const std::string who = "msfm_refine_camera";
    if (const int rc = tri_session_check(ctx, who, true)) return rc;
    msfm_rc::Params prm = {1e-6, MSFM_CAM_FX_FY, 10, 100, 0};
    if (params) prm = msfm_rc::Params{params->step_tol, params->mask, params->max_iters, params->min_observations, 0};
    if (!msfm_rc::mask_ok(prm.mask))
        return fail(ctx, MSFM_E_INVALID, who + ": mask must be a non-empty set of MSFM_CAM_* bits, FX_FY and F not together");
    if (prm.max_iters < 0 || prm.max_iters > 100) return fail(ctx, MSFM_E_INVALID, who + ": max_iters must lie in 0 .. 100");
    if (!std::isfinite(prm.step_tol) || prm.step_tol < 0.0) return fail(ctx, MSFM_E_INVALID, who + ": step_tol must be finite and not negative");
    if (prm.min_observations < 6) return fail(ctx, MSFM_E_INVALID, who + ": min_observations must be at least 6");
    // from here on the registrations and the pose refinement's records are gone, as after msfm_refine_points
    ts.reg_valid = ts.rp_valid = false;
    const bool had_mask = ts.mask_valid;
    std::vector<msfm_pose_rt> by_rank;
    std::vector<TriImage> table;
    if (const int rc = tri_tables(ctx, who, &ts.tri_camera, ts.tri_ids.data(), ts.tri_poses.data(), (int)ts.tri_ids.size(),
                                  msfm_tri::Params{ts.tri_prm.max_error, ts.tri_prm.min_angle, ts.tri_prm.min_views, 0}, &by_rank, &table))
        return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long T = ts.stats.tracks_kept, O = ts.stats.observations_kept;
    if (O > 0x7fffffffLL) return fail(ctx, MSFM_E_CAPACITY, who + ": more than 2^31 - 1 kept observations");
    const int n_chunks = (T > 0 && O > 0) ? (int)((O + msfm_rc::kChunk - 1) / msfm_rc::kChunk) : 0;
    const size_t Cz = (size_t)std::max(n_chunks, 1), Oz = (size_t)std::max<long long>(1, O);
    PoseTables pt;   // (the temporaries are freed when the call returns, whatever it returns)
    struct {
        TmpBuf counters, obs, slots, chunk_sums, chunk_cost, chunk_counts, reduced;
    } t;
    TmpEvents<2> ev;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, ev.create());
    HIPCHK(ctx, t.counters.ensure(sizeof(RcCounters)));
    HIPCHK(ctx, t.obs.ensure(Oz * sizeof(msfm_ref::Obs)));
    HIPCHK(ctx, t.slots.ensure(Oz * sizeof(msfm_rc::Slot)));
    HIPCHK(ctx, t.chunk_sums.ensure(Cz * msfm_rc::kSums * sizeof(double)));
    HIPCHK(ctx, t.chunk_cost.ensure(Cz * sizeof(double)));
    HIPCHK(ctx, t.chunk_counts.ensure(Cz * 2 * sizeof(int)));
    HIPCHK(ctx, t.reduced.ensure(sizeof(RcReduced)));
    HIPCHK(ctx, pt.upload(ts.tri_camera, by_rank, table, (int)ts.nd.ids.size()));
    HIPCHK(ctx, hipMemsetAsync(t.counters.p, 0, sizeof(RcCounters), st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    HIPCHK(ctx, pt.prepare(st));
    const unsigned char* d_mask = had_mask ? ts.t_mask.as<unsigned char>() : nullptr;
    if (n_chunks > 0) {
        HIPCHK(ctx, launch_ref_obs(ctx, pt, d_mask, t.obs.as<msfm_ref::Obs>(), st));
        hipLaunchKernelGGL(rc_slot_kernel, dim3(tk_grid(ctx, T)), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(),
                           (const int*)ts.r_img.as<int>(), (const int*)ts.r_idx.as<int>(), (int)T, pt.d_table(),
                           (const msfm_ref::Obs*)t.obs.as<msfm_ref::Obs>(), pt.d_poses(), (const msfm_point3d*)ts.t_points.as<msfm_point3d>(),
                           t.slots.as<msfm_rc::Slot>(), t.counters.as<RcCounters>());
        HIPCHK(ctx, hipGetLastError());
    }
    const unsigned grid = std::max(1u, std::min<unsigned>((unsigned)n_chunks, kRcGridPerCu * (unsigned)std::max(1, ctx->cu_count)));
    RcDevEval dev{st, t.slots.as<msfm_rc::Slot>(), O, n_chunks, grid, ts.tri_prm.max_error, prm.mask, t.chunk_sums.as<double>(),
                  t.chunk_cost.as<double>(), t.chunk_counts.as<int>(), t.reduced.as<RcReduced>(), pt.cam};
    const msfm_emat::Camera before = pt.cam;
    msfm_emat::Camera cam = before;
    msfm_rc::Result res;
    msfm_rc::refine_camera(dev, prm, &cam, &res, nullptr);
    HIPCHK(ctx, dev.err);   // (nothing of the session has been written yet)
    if (res.stands && n_chunks > 0) {
        pt.cam = cam;
        HIPCHK(ctx, launch_ref_obs(ctx, pt, d_mask, t.obs.as<msfm_ref::Obs>(), st));
        hipLaunchKernelGGL(rc_verdict_kernel, dim3(tk_grid(ctx, T)), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(), (int)T,
                           (const msfm_ref::Obs*)t.obs.as<msfm_ref::Obs>(), pt.d_poses(), (cam.fx + cam.fy) / 2.0,
                           msfm_ref::Verdict{ts.tri_prm.max_error, ts.tri_prm.min_angle}, ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(),
                           t.counters.as<RcCounters>());
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    const hipError_t done = hipStreamSynchronize(st);   // (before anything returns: the temporaries die with this function)
    if (done != hipSuccess && res.stands) ts.tri_valid = ts.mask_valid = false;   // (the records may be half rewritten)
    HIPCHK(ctx, done);
    RcCounters hc = {};
    const hipError_t back = hipMemcpy(&hc, t.counters.p, sizeof(hc), hipMemcpyDeviceToHost);
    if (back != hipSuccess && res.stands) ts.tri_valid = ts.mask_valid = false;   // (the points describe a camera the session does not have)
    HIPCHK(ctx, back);
    float all_ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&all_ms, ev[0], ev[1]));
    const auto as_c = [](const msfm_emat::Camera& c) { return msfm_camera{c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2}; };
    if (res.stands) ts.tri_camera = as_c(cam);   // the camera that stands replaces the session's
    msfm_camera_refine_stats s = {};
    s.observations = (int64_t)hc.contributing;
    s.behind = (int64_t)hc.behind;
    s.iterations = res.iterations;
    s.accepted_steps = res.accepted;
    s.stop = res.stop;
    s.refined = res.stands;
    s.rejected_by_inliers = (res.accepted > 0 && !res.stands) ? 1 : 0;
    s.inliers_before = res.inliers_before;
    s.inliers_after = res.inliers_after;
    s.points_recalibrated = (int64_t)hc.recalibrated;
    s.points_lost = (int64_t)hc.lost;
    s.points_gained = (int64_t)hc.gained;
    s.cost_before = res.cost_before;
    s.cost_after = res.cost_after;
    s.camera_before = as_c(before);
    s.camera_after = as_c(cam);
    s.refine_ms = all_ms;
    if (stats) *stats = s;
    return MSFM_OK;
}

int fetch_camera_impl(msfm_ctx* ctx, msfm_camera* out) {
    TrackSession& ts = ctx->tracks;
    if (!ts.open) return fail(ctx, MSFM_E_STATE, "msfm_fetch_camera without a track session (msfm_tracks_begin)");
    if (!ts.finished || !ts.tri_valid)
        return fail(ctx, MSFM_E_STATE, "msfm_fetch_camera without a camera: msfm_triangulate_tracks has not run since the last msfm_tracks_finish");
    if (!out) return fail(ctx, MSFM_E_INVALID, "msfm_fetch_camera: NULL out");
    *out = ts.tri_camera;
    return MSFM_OK;
}

}  // namespace
