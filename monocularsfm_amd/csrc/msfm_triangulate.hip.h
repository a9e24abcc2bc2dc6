// msfm_triangulate.hip.h -- track triangulation on the device (include/msfm_match.h "track triangulation"): the
// two kernels and the host side of msfm_triangulate_tracks / msfm_fetch_points3d (defined in msfm_match.hip).  The arithmetic is
// msfm_triangulate.h, shared with the host twin TriangulateTracks: the same bits.  Included by msfm_match.hip behind msfm_tracks.hip.h.
//
//   tri_pose_kernel   one lane per declared image: the caller's pose -> msfm_tri::Pose (valid iff flagged valid and finite; the centre).
//   tri_track_kernel  one lane per kept track, grid-stride, 256 threads, no LDS, on the library's stream.  Per used observation a
//                     dependent gather: the element's (image id, keypoint index) from the track CSR, the image's table entry, the 8-byte
//                     keypoint, the 128-byte pose.  The 4 x 4 normal matrix and the Jacobi state stay in registers (every index is a
//                     compile-time constant); the track's elements are re-read in the error pass and the parallax scan instead of
//                     being kept, so the register need does not depend on the track's length.  Plain vector loads and stores; the
//                     counters of the stats go through wave_add_counters (they only COUNT: no order reaches the output).
#pragma once
#include "msfm_triangulate.h"

namespace msfm {

struct TriImage {
    const float2* kxy;   // the image's keypoints (not read unless the image is posed)
    int rank;            // declared-image rank = index into the pose table; -1: not declared
    int pad;
};

struct TriCounters {
    unsigned long long attempted, with_point, error_ok, angle_ok, depth_ok, succeeded, observations_used;
};
constexpr int kTriCounters = 7;

// Integer counters of a kernel, one set per lane: reduced over the wave by a shuffle tree, then one vector atomic per wave and non-zero
// counter (they only COUNT: no order reaches the output).  Every lane of the wave must call it.
template <int N>
__device__ __forceinline__ void wave_add_counters(const unsigned long long (&c)[N], unsigned long long* out) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        unsigned long long v = c[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(out + k, v);
    }
}

// The lanes of a wave with `add` set append `value` to a list: a ballot, one atomic per wave for the position.  The list's order
// differs from run to run.  Every lane of the wave must call it.
__device__ __forceinline__ void wave_list_append(bool add, int value, int* __restrict__ list, int* __restrict__ list_count) {
    const int lane = threadIdx.x & 63;
    const unsigned long long bal = __ballot(add);
    if (bal) {
        const int leader = __ffsll((long long)bal) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(list_count, __popcll(bal));
        base = __shfl(base, leader, 64);
        if (add) list[base + __popcll(bal & ((1ull << lane) - 1ull))] = value;
    }
}

// one record added to the seven counters of TriCounters, in its order
__device__ __forceinline__ void tri_count(unsigned long long* c, const msfm_point3d& r) {
    const int s = r.status, ok = MSFM_TRI_POINT | MSFM_TRI_ERROR_OK | MSFM_TRI_ANGLE_OK;
    c[0] += (s & MSFM_TRI_ATTEMPTED) ? 1 : 0;
    c[1] += (s & MSFM_TRI_POINT) ? 1 : 0;
    c[2] += (s & MSFM_TRI_ERROR_OK) ? 1 : 0;
    c[3] += (s & MSFM_TRI_ANGLE_OK) ? 1 : 0;
    c[4] += (s & MSFM_TRI_DEPTH_OK) ? 1 : 0;
    c[5] += ((s & ok) == ok) ? 1 : 0;
    c[6] += (unsigned long long)r.n_views;
}

__global__ __launch_bounds__(256) void tri_pose_kernel(const msfm_pose_rt* __restrict__ in, int n, msfm_tri::Pose* __restrict__ out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) msfm_tri::prepare_pose(in[p], out + p);
}

// the elements of one track as msfm_tri::triangulate_track reads them
struct TriDevTrack {
    const int* __restrict__ img;
    const int* __restrict__ idx;
    const TriImage* __restrict__ table;
    const msfm_tri::Pose* __restrict__ poses;
    __device__ __forceinline__ const msfm_tri::Pose* pose(int k) const {
        const msfm_tri::Pose* p = poses + table[img[k]].rank;   // (a track's images are declared: rank >= 0)
        return p->valid ? p : nullptr;
    }
    __device__ __forceinline__ void pixel(int k, double* x, double* y) const {
        const float2 q = table[img[k]].kxy[idx[k]];
        *x = (double)q.x;
        *y = (double)q.y;
    }
};

__global__ __launch_bounds__(256) void tri_track_kernel(const long long* __restrict__ offsets, const int* __restrict__ img,
                                                        const int* __restrict__ idx, const unsigned char* __restrict__ cons, int T,
                                                        const TriImage* __restrict__ table, const msfm_tri::Pose* __restrict__ poses,
                                                        msfm_emat::Camera cam, msfm_tri::Params prm, msfm_point3d* __restrict__ points,
                                                        double* __restrict__ residuals, TriCounters* __restrict__ counters) {
    unsigned long long c[kTriCounters] = {0, 0, 0, 0, 0, 0, 0};
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        const long long b = offsets[t], e = offsets[t + 1];
        const TriDevTrack a{img + b, idx + b, table, poses};
        msfm_point3d r;
        msfm_tri::triangulate_track(a, (int)(e - b), cons[t] != 0, cam, prm, &r, residuals + b);
        points[t] = r;
        tri_count(c, r);
    }
    wave_add_counters(c, reinterpret_cast<unsigned long long*>(counters));
}

}  // namespace msfm

namespace {

// A device buffer that lives as long as the call that declares it: DevBuf (which never frees by itself: the session's long-lived
// buffers rely on that) plus the release when it goes out of scope, whatever the call returns.
struct TmpBuf : DevBuf {
    TmpBuf() = default;
    TmpBuf(const TmpBuf&) = delete;
    TmpBuf& operator=(const TmpBuf&) = delete;
    ~TmpBuf() { release(); }
};

// the N events a call times itself with, destroyed with it
template <int N>
struct TmpEvents {
    hipEvent_t ev[N] = {};
    TmpEvents() = default;
    TmpEvents(const TmpEvents&) = delete;
    TmpEvents& operator=(const TmpEvents&) = delete;
    ~TmpEvents() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t create() {
        for (hipEvent_t& e : ev)
            if (const hipError_t rc = hipEventCreate(&e)) return rc;
        return hipSuccess;
    }
    hipEvent_t operator[](int k) const { return ev[k]; }
};

// The session state every call of the reconstruction stage (`who`) needs: an open, finished track session and no open series; the
// calls that work on points (needs_points) need the points of a triangulation as well.
int tri_session_check(msfm_ctx* ctx, const std::string& who, bool needs_points) {
    const TrackSession& ts = ctx->tracks;
    if (!ts.open) return fail(ctx, MSFM_E_STATE, who + " without a track session (msfm_tracks_begin)");
    if (needs_points && (!ts.finished || !ts.tri_valid))
        return fail(ctx, MSFM_E_STATE, who + " without points: msfm_triangulate_tracks has not run since the last msfm_tracks_finish");
    if (!ts.finished) return fail(ctx, MSFM_E_STATE, who + " before a successful msfm_tracks_finish");
    if (ctx->series_open) return fail(ctx, MSFM_E_STATE, who + " while a streaming series (msfm_match_pairs_begin .. _next) is open");
    return MSFM_OK;
}

// A caller's list of image ids as one byte per declared-image rank.  Per id, in this order: it is declared in the session (else
// `undeclared`), it is not in the list already (else `twice`); both texts are the caller's own and the id is appended to them.
int rank_bytes(msfm_ctx* ctx, const int32_t* ids, int n, const std::string& undeclared, const std::string& twice,
               std::vector<unsigned char>* bytes) {
    const TrackSession& ts = ctx->tracks;
    bytes->assign(std::max<size_t>(ts.nd.ids.size(), 1), 0);
    for (int k = 0; k < n; ++k) {
        if (!ts.declares(ids[k])) return fail(ctx, MSFM_E_INVALID, undeclared + std::to_string(ids[k]));
        unsigned char& b = (*bytes)[(size_t)ts.rank_of[(size_t)ids[k]]];
        if (b) return fail(ctx, MSFM_E_INVALID, twice + std::to_string(ids[k]));
        b = 1;
    }
    return MSFM_OK;
}

// What a call (`who`) checks of a camera, thresholds and a pose list before any device work, and the two tables it uploads: the
// caller's poses by declared-image rank, the per-image-id entry of the kernels.  It reads the session and changes nothing of it.
int tri_tables(msfm_ctx* ctx, const std::string& who, const msfm_camera* camera, const int32_t* image_ids, const msfm_pose_rt* poses,
               int n_poses, const msfm_tri::Params& prm, std::vector<msfm_pose_rt>* by_rank_out, std::vector<TriImage>* table_out) {
    const TrackSession& ts = ctx->tracks;
    if (!camera) return fail(ctx, MSFM_E_INVALID, who + ": NULL camera");
    const msfm_camera c = *camera;
    for (double v : {c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2})
        if (!std::isfinite(v)) return fail(ctx, MSFM_E_INVALID, who + ": camera parameters must be finite");
    if (!(c.fx > 0.0) || !(c.fy > 0.0)) return fail(ctx, MSFM_E_INVALID, who + ": fx and fy must be positive");
    if (!std::isfinite(prm.max_error) || !std::isfinite(prm.min_angle)) return fail(ctx, MSFM_E_INVALID, who + ": parameters must be finite");
    if (prm.max_error < 0.0 || prm.min_angle < 0.0) return fail(ctx, MSFM_E_INVALID, who + ": max_error and min_angle must not be negative");
    if (n_poses < 0 || (n_poses > 0 && (!image_ids || !poses))) return fail(ctx, MSFM_E_INVALID, who + ": bad pose list");
    const int n_img = (int)ts.nd.ids.size();
    std::vector<msfm_pose_rt>& by_rank = *by_rank_out;
    by_rank.assign((size_t)std::max(n_img, 1), msfm_pose_rt{});
    std::vector<char> given((size_t)std::max(n_img, 1), 0);
    for (int k = 0; k < n_poses; ++k) {
        const int id = image_ids[k];
        if (!ts.declares(id)) return fail(ctx, MSFM_E_INVALID, who + ": image not declared in the session: " + std::to_string(id));
        const int r = ts.rank_of[(size_t)id];
        if (given[(size_t)r]) return fail(ctx, MSFM_E_INVALID, who + ": an image is given twice: " + std::to_string(id));
        given[(size_t)r] = 1;
        if (poses[k].valid) {
            for (double v : poses[k].R)
                if (!std::isfinite(v)) return fail(ctx, MSFM_E_INVALID, who + ": non-finite R of image " + std::to_string(id));
            for (double v : poses[k].t)
                if (!std::isfinite(v)) return fail(ctx, MSFM_E_INVALID, who + ": non-finite t of image " + std::to_string(id));
        }
        by_rank[(size_t)r] = poses[k];
        by_rank[(size_t)r].valid = poses[k].valid ? 1 : 0;
        by_rank[(size_t)r].reserved = 0;
    }
    std::vector<TriImage>& table = *table_out;
    table.assign((size_t)MSFM_MAX_IMAGES, TriImage{nullptr, -1, 0});
    for (int r = 0; r < n_img; ++r) {
        const int id = ts.nd.ids[(size_t)r];
        const Image& im = ctx->images[(size_t)id];
        if (by_rank[(size_t)r].valid && im.nk < ts.nd.rows[(size_t)r])
            return fail(ctx, MSFM_E_NOIMAGE, who + ": posed image without keypoints (msfm_upload_keypoints): " + std::to_string(id));
        table[(size_t)id] = TriImage{im.kxy, r, 0};
    }
    return MSFM_OK;
}

// The pose tables of one call on the device: tri_tables' two tables, the prepared poses the kernels read, and the camera in the
// kernels' form.
struct PoseTables {
    TmpBuf in, poses, table;
    msfm_emat::Camera cam;
    int n_ranks = 0;
    const msfm_tri::Pose* d_poses() const { return poses.as<msfm_tri::Pose>(); }
    const TriImage* d_table() const { return table.as<TriImage>(); }
    // (synchronous copies of the two small tables: nothing queued reads host memory that an early return of the caller would free)
    hipError_t upload(const msfm_camera& c, const std::vector<msfm_pose_rt>& by_rank, const std::vector<TriImage>& tab, int n_img) {
        cam = msfm_emat::Camera{c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2};
        n_ranks = n_img;
        hipError_t e = in.ensure(by_rank.size() * sizeof(msfm_pose_rt));
        if (e == hipSuccess) e = poses.ensure(by_rank.size() * sizeof(msfm_tri::Pose));
        if (e == hipSuccess) e = table.ensure(tab.size() * sizeof(TriImage));
        if (e == hipSuccess) e = hipMemcpy(in.p, by_rank.data(), by_rank.size() * sizeof(msfm_pose_rt), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(table.p, tab.data(), tab.size() * sizeof(TriImage), hipMemcpyHostToDevice);
        return e;
    }
    // tri_pose_kernel over the declared images
    hipError_t prepare(hipStream_t st) {
        if (n_ranks <= 0) return hipSuccess;
        hipLaunchKernelGGL(tri_pose_kernel, dim3((unsigned)((n_ranks + 255) / 256)), dim3(256), 0, st, (const msfm_pose_rt*)in.as<msfm_pose_rt>(),
                           n_ranks, poses.as<msfm_tri::Pose>());
        return hipGetLastError();
    }
};

// what a successful msfm_triangulate_tracks / _robust leaves behind for msfm_refine_points (msfm_refine.hip.h): a host copy of its inputs
void tri_keep_inputs(TrackSession& ts, const msfm_camera& camera, const int32_t* image_ids, const msfm_pose_rt* poses, int n_poses,
                     const msfm_tri::Params& prm) {
    ts.tri_camera = camera;
    ts.tri_prm = msfm_triangulation_params{prm.max_error, prm.min_angle, prm.min_views, 0};
    ts.tri_ids.assign(image_ids, image_ids + (n_poses > 0 ? n_poses : 0));
    ts.tri_poses.assign(poses, poses + (n_poses > 0 ? n_poses : 0));
}

int triangulate_impl(msfm_ctx* ctx, const msfm_camera* camera, const int32_t* image_ids, const msfm_pose_rt* poses, int n_poses,
                     const msfm_triangulation_params* params, msfm_triangulation_stats* stats) {
    TrackSession& ts = ctx->tracks;
    msfm_tri::Params prm = {2.0, 1.5, 2, 0};   // Triangulator::Parameters
    if (params) prm = msfm_tri::Params{params->max_error, params->min_angle, params->min_views, 0};
    // whatever happens below, the previous points are gone, and with them the inlier bytes of a robust call, the registrations made
    // from them and the pose refinement's records
    ts.tri_valid = ts.mask_valid = ts.reg_valid = ts.rp_valid = false;
    const std::string who = "msfm_triangulate_tracks";
    if (const int rc = tri_session_check(ctx, who, false)) return rc;
    std::vector<msfm_pose_rt> by_rank;
    std::vector<TriImage> table;
    if (const int rc = tri_tables(ctx, who, camera, image_ids, poses, n_poses, prm, &by_rank, &table)) return rc;
    const msfm_camera c = *camera;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long long T = ts.stats.tracks_kept, O = ts.stats.observations_kept;
    PoseTables pt;   // (the temporaries are freed when the call returns, whatever it returns)
    TmpBuf counters;
    TmpEvents<2> ev;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, ev.create());
    HIPCHK(ctx, counters.ensure(sizeof(TriCounters)));
    HIPCHK(ctx, ts.t_points.ensure((size_t)std::max<long long>(1, T) * sizeof(msfm_point3d)));
    HIPCHK(ctx, ts.t_resid.ensure((size_t)std::max<long long>(1, O) * sizeof(double)));
    HIPCHK(ctx, pt.upload(c, by_rank, table, (int)ts.nd.ids.size()));
    HIPCHK(ctx, hipMemsetAsync(counters.p, 0, sizeof(TriCounters), st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    HIPCHK(ctx, pt.prepare(st));
    if (T > 0) {
        hipLaunchKernelGGL(tri_track_kernel, dim3(tk_grid(ctx, T)), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(),
                           (const int*)ts.r_img.as<int>(), (const int*)ts.r_idx.as<int>(), (const unsigned char*)ts.r_cons.as<unsigned char>(), (int)T,
                           pt.d_table(), pt.d_poses(), pt.cam, prm, ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(),
                           counters.as<TriCounters>());
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    const hipError_t done = hipStreamSynchronize(st);   // (before anything returns: the temporaries die with this function)
    HIPCHK(ctx, done);
    TriCounters hc = {};
    HIPCHK(ctx, hipMemcpy(&hc, counters.p, sizeof(hc), hipMemcpyDeviceToHost));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
    msfm_triangulation_stats s = {};
    s.tracks = T;
    s.attempted = (int64_t)hc.attempted;
    s.with_point = (int64_t)hc.with_point;
    s.error_ok = (int64_t)hc.error_ok;
    s.angle_ok = (int64_t)hc.angle_ok;
    s.depth_ok = (int64_t)hc.depth_ok;
    s.succeeded = (int64_t)hc.succeeded;
    s.observations_used = (int64_t)hc.observations_used;
    s.device_bytes = (int64_t)(ts.t_points.cap + ts.t_resid.cap);
    s.triangulate_ms = ms;
    tri_keep_inputs(ts, c, image_ids, poses, n_poses, prm);
    ts.tri_valid = true;
    if (stats) *stats = s;
    return MSFM_OK;
}

int fetch_points3d_impl(msfm_ctx* ctx, msfm_point3d* out_points, double* out_residuals) {
    TrackSession& ts = ctx->tracks;
    if (!ts.open) return fail(ctx, MSFM_E_STATE, "msfm_fetch_points3d without a track session (msfm_tracks_begin)");
    if (!ts.finished || !ts.tri_valid) return fail(ctx, MSFM_E_STATE, "msfm_fetch_points3d without points: msfm_triangulate_tracks has not run since the last msfm_tracks_finish");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t T = (size_t)ts.stats.tracks_kept, O = (size_t)ts.stats.observations_kept;
    if (out_points && T) HIPCHK(ctx, hipMemcpy(out_points, ts.t_points.p, T * sizeof(msfm_point3d), hipMemcpyDeviceToHost));
    if (out_residuals && O) HIPCHK(ctx, hipMemcpy(out_residuals, ts.t_resid.p, O * sizeof(double), hipMemcpyDeviceToHost));
    return MSFM_OK;
}

}  // namespace
