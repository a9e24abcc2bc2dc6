// msfm_triangulate_robust.hip.h -- robust track triangulation on the device (include/msfm_match.h "robust track triangulation",
// DESIGN.md section 17): the two kernels and the host side of msfm_triangulate_tracks_robust / msfm_fetch_point_inliers (defined in
// msfm_match.hip).  The arithmetic is msfm_triangulate.h's robust part, shared with the host twin TriangulateTracksRobust: the same
// bits.  Included by msfm_match.hip behind msfm_triangulate.hip.h, whose TriDevTrack, PoseTables, tri_tables and wave helpers it reuses.
//
// Everything runs on the library's stream between HIP events; the host waits once, for the length of the retry list.
//   trr_first_kernel   one lane per kept track, grid-stride, the shape of tri_track_kernel: the plain record (triangulate_track), the
//                      residuals, the inlier byte of every element (1 on the used observations of an attempted track).  The tracks to
//                      retry (msfm_tri::retry) are appended to a list: a ballot per wave, one atomic per wave for the list position.
//                      The list's order differs from run to run; no output depends on it.  Tracks that are not retried are counted.
//   trr_retry_kernel   one wave per listed track, kTrrWaves waves per workgroup, grid-stride over the list; not launched for an empty
//                      list.  The wave first writes the track's used observations by position (the elements of posed images, compacted
//                      by ballots).  Lanes are hypotheses, in rounds of 64: a lane adds its two observations to a 4 x 4 normal matrix
//                      in registers (every index a compile-time constant) and solves it.  The used observations pass through the wave's
//                      LDS in tiles of kTrrTile -- (u, v), R, t, O: 17 doubles each, 8.5 KiB per wave, 34 KiB + 1 KiB of element
//                      numbers per workgroup; four workgroups would fit a CU's 160 KiB, the 214 VGPRs of a lane's Jacobi state allow
//                      two (two waves per SIMD) -- and every lane scores its point from broadcast reads.  The round's winner by __shfl_xor (largest count, lowest hypothesis).  mask1 and
//                      mask2: lane k tests observation k of a tile, a ballot gives the count, the lane stores its byte.  The refit
//                      (dlt_point on Masked) runs on every lane redundantly -- uniform addresses, no sum re-ordered -- and
//                      evaluate_point on lane 0.
// Plain vector loads and stores; the stats' counters are kept per wave and added with one vector atomic each.
#pragma once
#include "msfm_triangulate.hip.h"

namespace msfm {

constexpr int kTrrTile = 64;          // used observations staged in LDS at a time = lanes of a wave
constexpr int kTrrWaves = 4;          // waves (tracks in flight) per trr_retry_kernel workgroup
constexpr int kTrrGroupsPerCU = 2;    // trr_retry_kernel workgroups resident per CU (register-bound: 214 VGPRs, two waves per SIMD)
constexpr int kTrrObsDoubles = 17;    // u, v | R[9] | t[3] | O[3]

struct TrrCounters {
    unsigned long long tri[kTriCounters];   // TriCounters' order
    unsigned long long retried, rescued, observations_rejected, hypotheses;
};
constexpr int kTrrCounters = kTriCounters + 4;

// what one wave wrote (LDS, or memory its own lanes read back) is visible to all of its lanes
__device__ __forceinline__ void trr_wave_sync() {
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void trr_first_kernel(const long long* __restrict__ offsets, const int* __restrict__ img,
                                                        const int* __restrict__ idx, const unsigned char* __restrict__ cons, int T,
                                                        const TriImage* __restrict__ table, const msfm_tri::Pose* __restrict__ poses,
                                                        msfm_emat::Camera cam, msfm_tri::Params prm, msfm_point3d* __restrict__ points,
                                                        double* __restrict__ residuals, unsigned char* __restrict__ mask,
                                                        int* __restrict__ list, int* __restrict__ list_count,
                                                        TrrCounters* __restrict__ counters) {
    unsigned long long c[kTriCounters] = {0, 0, 0, 0, 0, 0, 0};
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); t0 < T; t0 += stride) {   // (uniform over the wave)
        const long long t = t0 + lane;
        bool again = false;
        if (t < T) {
            const long long b = offsets[t], e = offsets[t + 1];
            const int n = (int)(e - b);
            const TriDevTrack a{img + b, idx + b, table, poses};
            msfm_point3d r;
            msfm_tri::triangulate_track(a, n, cons[t] != 0, cam, prm, &r, residuals + b);
            points[t] = r;
            const bool attempted = (r.status & MSFM_TRI_ATTEMPTED) != 0;
            for (int k = 0; k < n; ++k) mask[b + k] = (attempted && a.pose(k)) ? 1 : 0;
            again = msfm_tri::retry(r, r.n_views);
            if (!again) tri_count(c, r);
        }
        wave_list_append(again, (int)t, list, list_count);
    }
    wave_add_counters(c, counters->tri);
}

// the staged observation at slot q of the wave's tile
__device__ __forceinline__ void trr_load_obs(const double (*so)[kTrrTile], int q, double R[9], double t[3], double* u, double* w) {
    *u = so[0][q];
    *w = so[1][q];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = so[2 + k][q];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = so[11 + k][q];
}

__global__ __launch_bounds__(64 * kTrrWaves) void trr_retry_kernel(const long long* __restrict__ offsets, const int* __restrict__ img,
                                                                  const int* __restrict__ idx, const TriImage* __restrict__ table,
                                                                  const msfm_tri::Pose* __restrict__ poses, msfm_emat::Camera cam,
                                                                  msfm_tri::RobustParams prm, const int* __restrict__ list, int listed,
                                                                  int* positions, msfm_point3d* __restrict__ points,
                                                                  double* __restrict__ residuals, unsigned char* mask,
                                                                  TrrCounters* __restrict__ counters) {
    using namespace msfm_tri;
    __shared__ double s_obs[kTrrWaves][kTrrObsDoubles][kTrrTile];
    __shared__ int s_elem[kTrrWaves][kTrrTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double (*so)[kTrrTile] = s_obs[wave];
    int* se = s_elem[wave];
    const unsigned long long below = (1ull << lane) - 1ull;
    const int need = prm.min_views > 2 ? prm.min_views : 2;
    const double f = (cam.fx + cam.fy) / 2.0;
    unsigned long long c[kTrrCounters] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // (lane 0's are the wave's)
    for (int at = blockIdx.x * kTrrWaves + wave; at < listed; at += gridDim.x * kTrrWaves) {   // (uniform over the wave)
        const int t = list[at];
        const long long b = offsets[t];
        const int n = (int)(offsets[t + 1] - b);
        const TriDevTrack a{img + b, idx + b, table, poses};
        int* pos_elem = positions + b;
        unsigned char* tmask = mask + b;
        // the used observations by position
        int m = 0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            const bool posed = k < n && a.pose(k);
            const unsigned long long bal = __ballot(posed);
            if (posed) pos_elem[m + __popcll(bal & below)] = k;
            m += __popcll(bal);
        }
        trr_wave_sync();
        // tile c0 .. of the used observations into the wave's LDS
        auto stage = [&](int c0) {
            trr_wave_sync();
            if (c0 + lane < m) {
                const int k = pos_elem[c0 + lane];
                const Pose* p = poses + table[a.img[k]].rank;
                double x, y, u, w;
                a.pixel(k, &x, &y);
                msfm_emat::undistort(cam, x, y, &u, &w);
                so[0][lane] = u;
                so[1][lane] = w;
#pragma unroll
                for (int q = 0; q < 9; ++q) so[2 + q][lane] = p->R[q];
#pragma unroll
                for (int q = 0; q < 3; ++q) so[11 + q][lane] = p->t[q];
#pragma unroll
                for (int q = 0; q < 3; ++q) so[14 + q][lane] = p->O[q];
                se[lane] = k;
            }
            trr_wave_sync();
        };
        const bool one_tile = m <= kTrrTile;
        if (one_tile) stage(0);   // (it stays for the whole track)
        // the inliers of X over all used observations: the count; store: each observation's byte as well
        auto inliers = [&](const double X[3], bool store) {
            int count = 0;
            for (int c0 = 0; c0 < m; c0 += kTrrTile) {
                if (!one_tile) stage(c0);
                bool in = false;
                if (c0 + lane < m) {
                    double R[9], tt[3], u, w;
                    trr_load_obs(so, lane, R, tt, &u, &w);
                    in = obs_inlier(R, tt, u, w, X, f, prm.max_error);
                    if (store) tmask[se[lane]] = in ? 1 : 0;
                }
                count += __popcll(__ballot(in));
            }
            return count;
        };
        const int H = (int)hypotheses_of(m, prm.max_hypotheses);
        const unsigned long long seed = tri_seed(t);
        int best = -1;
        double Xb[3] = {0.0, 0.0, 0.0};
        for (int h0 = 0; h0 < H; h0 += 64) {
            const int h = h0 + lane;
            const bool live = h < H;
            int pi = 1, pj = 0;
            if (live) hypothesis_pair(seed, h, m, prm.max_hypotheses, &pi, &pj);
            double A4[4][4], Oi[3] = {0.0, 0.0, 0.0}, Oj[3] = {0.0, 0.0, 0.0};
            dlt_clear(A4);
            for (int c0 = 0; c0 < m; c0 += kTrrTile) {   // (tiles ascend: observation j is added before observation i)
                if (!one_tile) stage(c0);
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    const int q = (side == 0 ? pj : pi) - c0;
                    if (live && q >= 0 && q < kTrrTile) {
                        double R[9], tt[3], u, w;
                        trr_load_obs(so, q, R, tt, &u, &w);
                        dlt_add(A4, R, tt, u, w);
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            if (side == 0) Oj[k] = so[14 + k][q];
                            else Oi[k] = so[14 + k][q];
                        }
                    }
                }
            }
            double X[3];
            bool valid = dlt_solve(A4, X) && live;
            int count = 0;
            for (int c0 = 0; c0 < m; c0 += kTrrTile) {
                if (!one_tile) stage(c0);
                const int mt = min(kTrrTile, m - c0);
                for (int q = 0; q < mt; ++q) {   // every lane reads the same address: LDS broadcast
                    double R[9], tt[3], u, w;
                    trr_load_obs(so, q, R, tt, &u, &w);
                    bool depth;
                    const double err = obs_error(R, tt, u, w, X, f, &depth);
                    count += (depth && err <= prm.max_error) ? 1 : 0;
                    if (c0 + q == pi || c0 + q == pj) valid = valid && depth;
                }
            }
            valid = valid && parallax(X, Oi, Oj) >= prm.min_angle;
            // the round's winner: the largest count, the lowest hypothesis
            int wc = valid ? count : -1, wh = h;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const int oc = __shfl_xor(wc, d, 64), oh = __shfl_xor(wh, d, 64);
                if (oc > wc || (oc == wc && oh < wh)) {
                    wc = oc;
                    wh = oh;
                }
            }
            if (wc > best) {   // (a later round wins only with a larger count: its hypotheses are higher)
                best = wc;
#pragma unroll
                for (int k = 0; k < 3; ++k) Xb[k] = __shfl(X[k], wh - h0, 64);
            }
        }
        msfm_point3d r;
        int kept = 0;
        if (best < need) {
            for (int k = lane; k < n; k += 64) {
                residuals[b + k] = -1.0;
                tmask[k] = 0;
            }
            clear_point(&r);
            r.status = MSFM_TRI_ATTEMPTED | MSFM_TRI_ROBUST;
        } else {
            kept = inliers(Xb, true);   // mask1
            trr_wave_sync();
            double X1[3];
            const Masked<TriDevTrack> masked{a, tmask};
            if (dlt_point(masked, n, cam, X1)) {   // (every lane, the same addresses)
                const int n2 = inliers(X1, false);
                if (n2 >= max(kept, need)) {
                    kept = inliers(X1, true);   // mask2
#pragma unroll
                    for (int k = 0; k < 3; ++k) Xb[k] = X1[k];
                }
            }
            trr_wave_sync();
            if (lane == 0) evaluate_point(a, n, Xb, tmask, cam, prm.min_angle, &r, residuals + b);
        }
        if (lane == 0) {
            points[t] = r;
            tri_count(c, r);
            c[kTriCounters] += 1;
            c[kTriCounters + 1] += ((r.status & (MSFM_TRI_POINT | MSFM_TRI_ANGLE_OK)) == (MSFM_TRI_POINT | MSFM_TRI_ANGLE_OK)) ? 1 : 0;
            c[kTriCounters + 2] += (r.status & MSFM_TRI_POINT) ? (unsigned long long)(m - kept) : 0;
            c[kTriCounters + 3] += (unsigned long long)H;
        }
        trr_wave_sync();   // (the next track's staging overwrites the tile)
    }
    if (lane == 0) {
        unsigned long long* out = counters->tri;
#pragma unroll
        for (int k = 0; k < kTrrCounters; ++k)
            if (c[k]) atomicAdd(out + k, c[k]);
    }
}

}  // namespace msfm

namespace {

int triangulate_robust_impl(msfm_ctx* ctx, const msfm_camera* camera, const int32_t* image_ids, const msfm_pose_rt* poses, int n_poses,
                            const msfm_robust_triangulation_params* params, msfm_triangulation_stats* stats,
                            msfm_robust_stats* robust_stats) {
    TrackSession& ts = ctx->tracks;
    msfm_tri::RobustParams rp = {2.0, 1.5, 2, 64};
    if (params) rp = msfm_tri::RobustParams{params->max_error, params->min_angle, params->min_views, params->max_hypotheses};
    const msfm_tri::Params prm = {rp.max_error, rp.min_angle, rp.min_views, 0};
    // whatever happens below, the previous points are gone, and with them the inlier bytes of a robust call, the registrations made
    // from them and the pose refinement's records
    ts.tri_valid = ts.mask_valid = ts.reg_valid = ts.rp_valid = false;
    const std::string who = "msfm_triangulate_tracks_robust";
    if (const int rc = tri_session_check(ctx, who, false)) return rc;
    std::vector<msfm_pose_rt> by_rank;
    std::vector<TriImage> table;
    if (const int rc = tri_tables(ctx, who, camera, image_ids, poses, n_poses, prm, &by_rank, &table)) return rc;
    if (rp.max_hypotheses < 1 || rp.max_hypotheses > 1024) return fail(ctx, MSFM_E_INVALID, who + ": max_hypotheses must lie in 1 .. 1024");
    const msfm_camera c = *camera;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long T = ts.stats.tracks_kept, O = ts.stats.observations_kept;
    PoseTables pt;   // (the temporaries are freed when the call returns, whatever it returns)
    TmpBuf counters, list, positions;
    TmpEvents<3> ev;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, ev.create());
    HIPCHK(ctx, counters.ensure(sizeof(TrrCounters)));
    HIPCHK(ctx, list.ensure((size_t)(std::max<long long>(1, T) + 1) * sizeof(int)));   // the list | its length
    HIPCHK(ctx, ts.t_points.ensure((size_t)std::max<long long>(1, T) * sizeof(msfm_point3d)));
    HIPCHK(ctx, ts.t_resid.ensure((size_t)std::max<long long>(1, O) * sizeof(double)));
    HIPCHK(ctx, ts.t_mask.ensure((size_t)std::max<long long>(1, O)));
    HIPCHK(ctx, pt.upload(c, by_rank, table, (int)ts.nd.ids.size()));
    HIPCHK(ctx, hipMemsetAsync(counters.p, 0, sizeof(TrrCounters), st));
    int* d_list = list.as<int>();
    int* d_listed = d_list + std::max<long long>(1, T);
    HIPCHK(ctx, hipMemsetAsync(d_listed, 0, sizeof(int), st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    HIPCHK(ctx, pt.prepare(st));
    const msfm_emat::Camera cam = pt.cam;
    int listed = 0;
    if (T > 0) {
        hipLaunchKernelGGL(trr_first_kernel, dim3(tk_grid(ctx, T)), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(),
                           (const int*)ts.r_img.as<int>(), (const int*)ts.r_idx.as<int>(), (const unsigned char*)ts.r_cons.as<unsigned char>(), (int)T,
                           pt.d_table(), pt.d_poses(), cam, prm,
                           ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(), ts.t_mask.as<unsigned char>(), d_list, d_listed,
                           counters.as<TrrCounters>());
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(ev[1], st));
        HIPCHK(ctx, hipMemcpyAsync(&listed, d_listed, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));   // the one wait: the length of the retry list
    } else {
        HIPCHK(ctx, hipEventRecord(ev[1], st));
    }
    if (listed > 0) {
        HIPCHK(ctx, positions.ensure((size_t)O * sizeof(int)));
        const unsigned groups = (unsigned)((listed + kTrrWaves - 1) / kTrrWaves);
        const unsigned grid = std::min<unsigned>(groups, (unsigned)(kTrrGroupsPerCU * std::max(1, ctx->cu_count)));
        hipLaunchKernelGGL(trr_retry_kernel, dim3(grid), dim3(64 * kTrrWaves), 0, st, (const long long*)ts.r_offsets.as<long long>(),
                           (const int*)ts.r_img.as<int>(), (const int*)ts.r_idx.as<int>(), pt.d_table(),
                           pt.d_poses(), cam, rp, (const int*)d_list, listed, positions.as<int>(),
                           ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(), ts.t_mask.as<unsigned char>(), counters.as<TrrCounters>());
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ev[2], st));
    const hipError_t done = hipStreamSynchronize(st);   // (before anything returns: the temporaries die with this function)
    HIPCHK(ctx, done);
    TrrCounters hc = {};
    HIPCHK(ctx, hipMemcpy(&hc, counters.p, sizeof(hc), hipMemcpyDeviceToHost));
    float first_ms = 0.f, all_ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&first_ms, ev[0], ev[1]));
    HIPCHK(ctx, hipEventElapsedTime(&all_ms, ev[0], ev[2]));
    msfm_triangulation_stats s = {};
    s.tracks = T;
    s.attempted = (int64_t)hc.tri[0];
    s.with_point = (int64_t)hc.tri[1];
    s.error_ok = (int64_t)hc.tri[2];
    s.angle_ok = (int64_t)hc.tri[3];
    s.depth_ok = (int64_t)hc.tri[4];
    s.succeeded = (int64_t)hc.tri[5];
    s.observations_used = (int64_t)hc.tri[6];
    s.device_bytes = (int64_t)(ts.t_points.cap + ts.t_resid.cap + ts.t_mask.cap);
    s.triangulate_ms = first_ms;   // tri_pose_kernel + trr_first_kernel: what msfm_triangulate_tracks times
    msfm_robust_stats rs = {};
    rs.retried = (int64_t)hc.retried;
    rs.rescued = (int64_t)hc.rescued;
    rs.observations_rejected = (int64_t)hc.observations_rejected;
    rs.hypotheses = (int64_t)hc.hypotheses;
    rs.robust_ms = all_ms;
    tri_keep_inputs(ts, c, image_ids, poses, n_poses, prm);
    ts.tri_valid = true;
    ts.mask_valid = true;
    if (stats) *stats = s;
    if (robust_stats) *robust_stats = rs;
    return MSFM_OK;
}

int fetch_point_inliers_impl(msfm_ctx* ctx, uint8_t* out) {
    TrackSession& ts = ctx->tracks;
    if (!ts.open) return fail(ctx, MSFM_E_STATE, "msfm_fetch_point_inliers without a track session (msfm_tracks_begin)");
    if (!ts.finished || !ts.tri_valid || !ts.mask_valid)
        return fail(ctx, MSFM_E_STATE, "msfm_fetch_point_inliers without inlier bytes: the session's last successful triangulation was not msfm_triangulate_tracks_robust");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t O = (size_t)ts.stats.observations_kept;
    if (out && O) HIPCHK(ctx, hipMemcpy(out, ts.t_mask.p, O, hipMemcpyDeviceToHost));
    return MSFM_OK;
}

}  // namespace
