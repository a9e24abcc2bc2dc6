// msfm_visibility.hip.h -- map visibility on the device (include/msfm_match.h "map visibility"): the two kernels
// and the host side of msfm_map_visibility (defined in msfm_match.hip).  The counting is msfm_visibility.h, shared with the host twin
// MapVisibility: the same integers.  Included by msfm_match.hip behind msfm_complete.hip.h.
//
// The call is READ-ONLY: it runs outside msfm_extend.hip.h's MapEditFrame, which prepares inlier bytes and drops validity flags.  It
// reads the track CSR, the records' status words and -- only where the session has them -- the inlier bytes; it needs no keypoint, no
// camera and no pose beyond its validity, so it uploads one small table (per image id: rank | query row | posed) instead of
// tri_tables' two.  Its temporaries die with the call.
//   vis_lane_kernel   one lane per kept track, a wave-uniform grid-stride loop, 256 threads, the shape of cmp_track_kernel.  A lane
//                     runs msfm_vis::walk_track over a track of at most kLaneMax elements; a longer consistent track goes to a list
//                     (a ballot per wave, one atomic per wave for the position; no output depends on its order).  <false>
//                     (ROUTE_GLOBAL): every add is an agent-scope uint32 add in global memory.  <true> (ROUTE_LDS): the 3 n per-image
//                     words, and the matrix rows where the route function admits them, are uint32 adds in the workgroup's LDS, zeroed
//                     at the start and flushed once at the end: thread i takes words i, i + 256, ..., skips zeros, and adds the rest
//                     to global memory, so one wave instruction covers 64 contiguous words.
//   vis_wave_kernel   one WAVE per listed track, grid-stride over the list, whose length it reads from device memory (the kernel
//                     boundary orders it): the lanes share the track's elements (walk_track with first = lane, step = 64), global
//                     adds on both routes.  A track of 256 elements under 256 query rows costs each lane 1024 adds, not 65 536.
// Counters are zeroed by hipMemsetAsync on the call's stream and copied out behind the last kernel: no fence inside a kernel, no plain
// read of another workgroup's counters.
#pragma once
#include "msfm_visibility.h"
#include "msfm_complete.hip.h"

namespace msfm {

struct VisCounters {
    unsigned long long tracks, elements, increments;
};
constexpr int kVisCounters = 3;

// the elements of one track as msfm_vis::walk_track reads them; tab: per image id {rank, ((row + 1) << 1) | posed}
struct VisDevTrack {
    const int* __restrict__ img;
    const unsigned char* __restrict__ mask;   // nullptr: the session has no inlier bytes
    const int2* __restrict__ tab;
    __device__ __forceinline__ msfm_vis::Elem operator()(int k) const {
        const int2 v = tab[img[k]];   // (a track's images are declared: rank >= 0)
        return msfm_vis::Elem{v.x, (v.y >> 1) - 1, (v.y & 1) != 0, mask ? mask[k] : (unsigned char)1};
    }
};

// image_words = 3 n; g_counts: the per-image words, then the matrix rows.  lds_words (kLds): how many of them the workgroup
// privatises -- image_words, or image_words + n_query n.
template <bool kLds>
__global__ __launch_bounds__(256) void vis_lane_kernel(const long long* __restrict__ offsets, const int* __restrict__ img,
                                                       const unsigned char* __restrict__ cons, const msfm_point3d* __restrict__ points,
                                                       const unsigned char* __restrict__ mask, const int2* __restrict__ tab, int T, int n,
                                                       int n_query, int basis, int lds_words, unsigned* __restrict__ g_counts,
                                                       int* __restrict__ list, int* __restrict__ list_count,
                                                       VisCounters* __restrict__ counters) {
    extern __shared__ unsigned vis_lds[];
    const int image_words = msfm_vis::kImageCounters * n;
    const bool lds_matrix = kLds && lds_words > image_words;
    if (kLds) {
        for (int i = threadIdx.x; i < lds_words; i += 256) vis_lds[i] = 0u;
        __syncthreads();
    }
    msfm_vis::Tally tl = {0, 0, 0};
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); t0 < T; t0 += stride) {   // (uniform over the wave)
        const long long t = t0 + lane;
        bool wide = false;
        if (t < T) {
            const long long b = offsets[t], e = offsets[t + 1];
            const int len = (int)(e - b);
            const bool consistent = cons[t] != 0;
            wide = consistent && list != nullptr && len > msfm_vis::kLaneMax;
            if (consistent && !wide) {
                const VisDevTrack a{img + b, mask ? mask + b : nullptr, tab};
                msfm_vis::walk_track(
                    a, len, 0, 1, basis, true, points ? points[t].status : 0, n_query > 0,
                    [&](int k, int rank) {
                        if (kLds) atomicAdd(&vis_lds[k * n + rank], 1u);
                        else atomicAdd(&g_counts[k * n + rank], 1u);
                    },
                    [&](int row, int rank) {
                        if (lds_matrix) atomicAdd(&vis_lds[image_words + row * n + rank], 1u);
                        else atomicAdd(&g_counts[(size_t)image_words + (size_t)row * (size_t)n + (size_t)rank], 1u);
                    },
                    &tl);
            }
        }
        wave_list_append(wide, (int)t, list, list_count);
    }
    if (kLds) {
        __syncthreads();
        for (int i = threadIdx.x; i < lds_words; i += 256) {
            const unsigned v = vis_lds[i];
            if (v) atomicAdd(&g_counts[i], v);
        }
    }
    const unsigned long long c[kVisCounters] = {(unsigned long long)tl.tracks, (unsigned long long)tl.elements, (unsigned long long)tl.increments};
    wave_add_counters(c, reinterpret_cast<unsigned long long*>(counters));
}

__global__ __launch_bounds__(256) void vis_wave_kernel(const long long* __restrict__ offsets, const int* __restrict__ img,
                                                       const msfm_point3d* __restrict__ points, const unsigned char* __restrict__ mask,
                                                       const int2* __restrict__ tab, int n, int n_query, int basis,
                                                       unsigned* __restrict__ g_counts, const int* __restrict__ list,
                                                       const int* __restrict__ list_count, VisCounters* __restrict__ counters) {
    const int image_words = msfm_vis::kImageCounters * n;
    msfm_vis::Tally tl = {0, 0, 0};
    const int lane = threadIdx.x & 63;
    const int waves = (int)((gridDim.x * blockDim.x) >> 6);
    const int listed = *list_count;
    for (int i = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); i < listed; i += waves) {   // (uniform over the wave)
        const long long t = list[i];
        const long long b = offsets[t];
        const VisDevTrack a{img + b, mask ? mask + b : nullptr, tab};
        msfm_vis::walk_track(
            a, (int)(offsets[t + 1] - b), lane, 64, basis, true, points ? points[t].status : 0, n_query > 0,
            [&](int k, int rank) { atomicAdd(&g_counts[k * n + rank], 1u); },
            [&](int row, int rank) { atomicAdd(&g_counts[(size_t)image_words + (size_t)row * (size_t)n + (size_t)rank], 1u); }, &tl);
    }
    const unsigned long long c[kVisCounters] = {(unsigned long long)tl.tracks, (unsigned long long)tl.elements, (unsigned long long)tl.increments};
    wave_add_counters(c, reinterpret_cast<unsigned long long*>(counters));
}

}  // namespace msfm

namespace {

int visibility_impl(msfm_ctx* ctx, const msfm_visibility_params* params, const int32_t* query_ids, int n_query,
                    msfm_image_visibility* out_images, uint32_t* out_covisible, msfm_visibility_stats* stats) {
    const TrackSession& ts = ctx->tracks;   // (const: not one byte of the session changes)
    const std::string who = "msfm_map_visibility";
    const int basis = params ? params->basis : (int)MSFM_VIS_MAP;
    const int want = params ? params->route : (int)MSFM_VIS_ROUTE_AUTO;
    if (basis != MSFM_VIS_TRACKS && basis != MSFM_VIS_MAP) return fail(ctx, MSFM_E_INVALID, who + ": unknown basis");
    if (want != MSFM_VIS_ROUTE_AUTO && want != MSFM_VIS_ROUTE_GLOBAL && want != MSFM_VIS_ROUTE_LDS)
        return fail(ctx, MSFM_E_INVALID, who + ": unknown route");
    if (const int rc = tri_session_check(ctx, who, basis == MSFM_VIS_MAP)) return rc;
    if (n_query < 0 || (n_query > 0 && !query_ids)) return fail(ctx, MSFM_E_INVALID, who + ": bad list of images");
    std::vector<unsigned char> queried;
    if (const int rc = rank_bytes(ctx, query_ids, n_query, who + ": image not declared in the session: ", who + ": an image is given twice: ", &queried))
        return rc;
    const int n = (int)ts.nd.ids.size();
    const long long T = ts.stats.tracks_kept, O = ts.stats.observations_kept;
    const msfm_vis::Route rt = msfm_vis::vis_route(want, n, n_query, T, O);
    if (rt.route == 0) return fail(ctx, MSFM_E_INVALID, who + ": MSFM_VIS_ROUTE_LDS does not fit this many images (msfm_vis::vis_route)");
    // the one table of the call: per image id its rank, its row in the query list and whether it is posed (basis MAP: what
    // tri_pose_kernel makes of the session's pose list)
    std::vector<unsigned char> posed((size_t)std::max(n, 1), 0);
    int n_posed = 0;
    if (basis == MSFM_VIS_MAP) {
        for (size_t k = 0; k < ts.tri_ids.size(); ++k) {
            msfm_tri::Pose p;
            msfm_tri::prepare_pose(ts.tri_poses[k], &p);
            if (!p.valid) continue;
            posed[(size_t)ts.rank_of[(size_t)ts.tri_ids[k]]] = 1;
            n_posed += 1;
        }
    }
    std::vector<int2> tab((size_t)MSFM_MAX_IMAGES, int2{-1, 0});
    for (int r = 0; r < n; ++r) tab[(size_t)ts.nd.ids[(size_t)r]] = int2{r, (int)posed[(size_t)r]};
    for (int k = 0; k < n_query; ++k) tab[(size_t)query_ids[k]].y |= (k + 1) << 1;
    const size_t image_words = (size_t)msfm_vis::kImageCounters * (size_t)std::max(n, 1);
    const size_t words = image_words + (size_t)n_query * (size_t)std::max(n, 1);
    const size_t count_bytes = sizeof(msfm::VisCounters) + words * sizeof(unsigned);
    const bool long_tracks = ts.stats.longest_track > msfm_vis::kLaneMax;   // (a list only where a kept track can need it)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TmpBuf d_tab, d_counts, d_list;   // (the temporaries are freed when the call returns, whatever it returns)
    TmpEvents<2> ev;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, ev.create());
    HIPCHK(ctx, d_tab.ensure(tab.size() * sizeof(int2)));
    HIPCHK(ctx, d_counts.ensure(count_bytes));
    if (long_tracks) HIPCHK(ctx, d_list.ensure((size_t)(T + 1) * sizeof(int)));
    HIPCHK(ctx, hipMemcpy(d_tab.p, tab.data(), tab.size() * sizeof(int2), hipMemcpyHostToDevice));   // (synchronous, like PoseTables::upload)
    msfm::VisCounters* d_stats = d_counts.as<msfm::VisCounters>();
    unsigned* d_words = reinterpret_cast<unsigned*>(d_stats + 1);
    int* d_listed = long_tracks ? d_list.as<int>() + T : nullptr;
    HIPCHK(ctx, hipMemsetAsync(d_counts.p, 0, count_bytes, st));
    if (long_tracks) HIPCHK(ctx, hipMemsetAsync(d_listed, 0, sizeof(int), st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    hipError_t queued = hipSuccess;   // from the first launch on the call waits before it fails: the temporaries die with it
    if (T > 0 && O > 0) {
        const long long* offsets = ts.r_offsets.as<long long>();
        const int* img = ts.r_img.as<int>();
        const unsigned char* cons = ts.r_cons.as<unsigned char>();
        const msfm_point3d* points = basis == MSFM_VIS_MAP ? ts.t_points.as<msfm_point3d>() : nullptr;
        const unsigned char* mask = (basis == MSFM_VIS_MAP && ts.mask_valid) ? ts.t_mask.as<unsigned char>() : nullptr;
        const int cus = std::max(1, ctx->cu_count);
        if (rt.route == MSFM_VIS_ROUTE_LDS) {
            // few workgroups, so that few flushes follow: two a CU
            const unsigned grid = (unsigned)std::min<long long>((T + 255) / 256, 2LL * cus);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(msfm::vis_lane_kernel<true>), dim3(grid), dim3(256), (size_t)rt.lds_bytes, st, offsets, img, cons,
                               points, mask, (const int2*)d_tab.as<int2>(), (int)T, n, n_query, basis, rt.lds_bytes / 4, d_words,
                               long_tracks ? d_list.as<int>() : (int*)nullptr, d_listed, d_stats);
        } else {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(msfm::vis_lane_kernel<false>), dim3(tk_grid(ctx, T)), dim3(256), 0, st, offsets, img, cons, points,
                               mask, (const int2*)d_tab.as<int2>(), (int)T, n, n_query, basis, 0, d_words,
                               long_tracks ? d_list.as<int>() : (int*)nullptr, d_listed, d_stats);
        }
        queued = hipGetLastError();
        if (long_tracks && queued == hipSuccess) {
            hipLaunchKernelGGL(msfm::vis_wave_kernel, dim3((unsigned)std::min<long long>((T + 3) / 4, 4LL * cus)), dim3(256), 0, st, offsets, img,
                               points, mask, (const int2*)d_tab.as<int2>(), n, n_query, basis, d_words, (const int*)d_list.as<int>(),
                               (const int*)d_listed, d_stats);
            queued = hipGetLastError();
        }
    }
    if (queued == hipSuccess) queued = hipEventRecord(ev[1], st);
    const hipError_t done = hipStreamSynchronize(st);
    HIPCHK(ctx, queued);
    HIPCHK(ctx, done);
    msfm::VisCounters hc = {};
    std::vector<uint32_t> h_words(words, 0);
    HIPCHK(ctx, hipMemcpy(&hc, d_stats, sizeof(hc), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(h_words.data(), d_words, words * sizeof(unsigned), hipMemcpyDeviceToHost));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (out_images) {
        for (int r = 0; r < n; ++r) {
            msfm_image_visibility v = {};
            v.image_id = ts.nd.ids[(size_t)r];
            v.flags = (posed[(size_t)r] ? MSFM_VIS_POSED : 0) | (queried[(size_t)r] ? MSFM_VIS_QUERIED : 0);
            v.n_elements = (int32_t)h_words[(size_t)msfm_vis::IMG_ELEMENTS * (size_t)n + (size_t)r];
            v.n_visible = (int32_t)h_words[(size_t)msfm_vis::IMG_VISIBLE * (size_t)n + (size_t)r];
            v.n_points = (int32_t)h_words[(size_t)msfm_vis::IMG_POINTS * (size_t)n + (size_t)r];
            out_images[r] = v;
        }
    }
    if (out_covisible && n_query > 0 && n > 0) std::memcpy(out_covisible, h_words.data() + image_words, (size_t)n_query * (size_t)n * sizeof(uint32_t));
    msfm_visibility_stats s = {};
    s.tracks_counted = (int64_t)hc.tracks;
    s.elements_counted = (int64_t)hc.elements;
    s.pair_increments = (int64_t)hc.increments;
    s.device_bytes = (int64_t)(d_tab.cap + d_counts.cap + d_list.cap);
    s.images = n;
    s.posed = n_posed;
    s.query = n_query;
    s.route = rt.route;
    s.visibility_ms = ms;
    if (stats) *stats = s;
    return MSFM_OK;
}

}  // namespace
