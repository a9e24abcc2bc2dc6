// msfm_extend.hip.h -- map extension on the device (include/msfm_match.h "map extension"): the three kernels and
// the host side of msfm_extend_points (defined in msfm_match.hip).  The arithmetic is msfm_extend.h, shared with the host twin
// ExtendPoints: the same bits.  Included by msfm_match.hip behind msfm_refine.hip.h, whose ref_obs_kernel it launches unchanged, and
// behind msfm_triangulate_robust.hip.h, whose trr_retry_kernel it launches unchanged.
//
// Everything runs on the library's stream between HIP events; the host waits once for the length of the retry list (robust route
// only) and once at the end.
//   ext_mask_kernel    one lane per kept track, grid-stride; launched only on a session without inlier bytes: the byte of every
//                      element (msfm_ext::plain_byte).  Per track, not per observation: the byte needs the record's ATTEMPTED bit
//                      and the session keeps no observation -> track map.
//   ref_obs_kernel     (msfm_refine.hip.h) under the enlarged pose table and the current bytes.
//   ext_track_kernel   one lane per kept track, grid-stride, 256 threads, no LDS, the shape of trr_first_kernel.  A lane scans its
//                      track's Obs for new observations; untouched lanes only count.  Continue lanes run msfm_ext::extend_track,
//                      create lanes msfm_tri::triangulate_track through TriDevTrack and write the track's bytes.  On the robust route
//                      the tracks that msfm_tri::retry selects are appended to a list: a ballot per wave, one atomic per wave for the
//                      list position; no output depends on its order.  The counters go through wave_add_counters.
//   trr_retry_kernel   (msfm_triangulate_robust.hip.h) over that list with its own `positions` scratch; not launched for an empty list.
//   ext_mark_kernel    one lane per listed track: the record the retry left | MSFM_TRI_EXTENDED.
// Plain vector loads and stores only; no floating-point atomics.
#pragma once
#include "msfm_extend.h"
#include "msfm_refine.hip.h"

namespace msfm {

struct ExtCounters {
    unsigned long long tracks_touched, continued, observations_added, observations_rejected, created_attempted, created, succeeded,
        observations_used;
};
constexpr int kExtCounters = 8;

__global__ __launch_bounds__(256) void ext_mask_kernel(const long long* __restrict__ offsets, const int* __restrict__ img, int T,
                                                       const TriImage* __restrict__ table, const msfm_tri::Pose* __restrict__ poses,
                                                       const unsigned char* __restrict__ gained, const msfm_point3d* __restrict__ points,
                                                       unsigned char* __restrict__ mask) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < T; t += stride) {
        const long long b = offsets[t], e = offsets[t + 1];
        const msfm_point3d r = points[t];
        for (long long o = b; o < e; ++o) {
            const int rank = table[img[o]].rank;   // (a track's images are declared: rank >= 0)
            mask[o] = msfm_ext::plain_byte(r, poses[rank].valid ? poses + rank : nullptr, rank, gained);
        }
    }
}

__global__ __launch_bounds__(256) void ext_track_kernel(const long long* __restrict__ offsets, const int* __restrict__ img,
                                                        const int* __restrict__ idx, const unsigned char* __restrict__ cons, int T,
                                                        const msfm_ref::Obs* __restrict__ obs, const TriImage* __restrict__ table,
                                                        const msfm_tri::Pose* __restrict__ poses, const unsigned char* __restrict__ gained,
                                                        msfm_emat::Camera cam, msfm_tri::Params prm, int robust, msfm_point3d* points,
                                                        double* residuals, unsigned char* mask, int* __restrict__ list,
                                                        int* __restrict__ list_count, ExtCounters* __restrict__ counters) {
    unsigned long long c[kExtCounters] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int lane = threadIdx.x & 63;
    const int ok = MSFM_TRI_POINT | MSFM_TRI_ERROR_OK | MSFM_TRI_ANGLE_OK;
    const double f = (cam.fx + cam.fy) / 2.0;
    const msfm_ref::Verdict vd = {prm.max_error, prm.min_angle};
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long t0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane); t0 < T; t0 += stride) {   // (uniform over the wave)
        const long long t = t0 + lane;
        bool again = false;
        if (t < T) {
            const long long b = offsets[t], e = offsets[t + 1];
            const int n = (int)(e - b);
            msfm_point3d r = points[t];
            const int fresh = cons[t] ? msfm_ext::new_observations(obs + b, n, gained) : 0;
            if (fresh > 0) {
                c[0] += 1;
                if (msfm_ext::continues(r)) {
                    msfm_ext::Tally tl;
                    msfm_ext::extend_track(obs + b, n, poses, gained, f, vd, &r, residuals + b, mask + b, &tl);
                    if (tl.accepted > 0) points[t] = r;
                    c[1] += tl.accepted > 0 ? 1 : 0;
                    c[2] += (unsigned long long)tl.accepted;
                    c[3] += (unsigned long long)tl.rejected;
                } else {
                    const TriDevTrack a{img + b, idx + b, table, poses};
                    msfm_tri::triangulate_track(a, n, true, cam, prm, &r, residuals + b);
                    const bool attempted = (r.status & MSFM_TRI_ATTEMPTED) != 0;
                    for (int k = 0; k < n; ++k) mask[b + k] = (attempted && a.pose(k)) ? 1 : 0;
                    again = robust && msfm_tri::retry(r, r.n_views);
                    if (!again) r.status |= MSFM_TRI_EXTENDED;   // (a retried track gets the bit from ext_mark_kernel)
                    points[t] = r;
                    c[4] += 1;
                    c[5] += (!again && (r.status & ok) == ok) ? 1 : 0;
                }
            }
            if (!again) {   // (trr_retry_kernel counts the tracks it rewrites)
                c[6] += ((r.status & ok) == ok) ? 1 : 0;
                c[7] += (unsigned long long)r.n_views;
            }
        }
        wave_list_append(again, (int)t, list, list_count);
    }
    wave_add_counters(c, reinterpret_cast<unsigned long long*>(counters));
}

__global__ __launch_bounds__(256) void ext_mark_kernel(const int* __restrict__ list, int listed, msfm_point3d* __restrict__ points) {
    const int at = blockIdx.x * blockDim.x + threadIdx.x;
    if (at < listed) points[list[at]].status |= MSFM_TRI_EXTENDED;
}

}  // namespace msfm

namespace {

// The frame of one map-edit call (msfm_extend_points, msfm_filter_points, msfm_complete_points): what the
// three own for the length of the call, the order of their work on the library's stream, and their failure rule.  A call checks its
// own parameters, then runs begin, observe, its track kernel(s) through `wrote`, and finish, and maps its counters to its stats.
// Until the first kernel that writes session memory is queued an error returns at once; from then on `queued` latches the first
// error, nothing more is launched, and finish still waits before it fails (the temporaries die with the frame).
struct MapEditFrame {
    msfm_ctx* const ctx;
    TrackSession& ts;
    const std::string who;
    const hipStream_t st;
    const long long T, O;          // the session's kept tracks and observations
    const unsigned grid;           // of a kernel with one lane per kept track
    const msfm_tri::Params prm;    // the thresholds of the triangulation that made the points
    bool had_mask = false;
    PoseTables pt;
    TmpBuf bytes, counters, obs;   // the caller's byte tables one behind the other | its counters | ref_obs_kernel's array
    TmpEvents<3> ev;
    hipError_t queued = hipSuccess;

    MapEditFrame(msfm_ctx* c, const std::string& name)
        : ctx(c), ts(c->tracks), who(name), st(store_stream(c)), T(ts.stats.tracks_kept), O(ts.stats.observations_kept), grid(tk_grid(c, T)),
          prm{ts.tri_prm.max_error, ts.tri_prm.min_angle, ts.tri_prm.min_views, 0} {}

    bool wrote(hipError_t e) {
        if (e != hipSuccess && queued == hipSuccess) queued = e;
        return e == hipSuccess;
    }
    // whether a kernel over the tracks is still to be launched
    bool live() const { return T > 0 && O > 0 && queued == hipSuccess; }
    // table k of begin's `tables` on the device
    const unsigned char* d_bytes(size_t k) const { return bytes.as<unsigned char>() + k * std::max<size_t>(ts.nd.ids.size(), 1); }

    // The pose list the call runs under (the session's, or extend's enlarged one) passes tri_tables' checks, which still leave the
    // session untouched.  Then the registrations and the pose refinement's records are gone, the temporaries exist, the small tables
    // (`tables`: one byte per rank each) are on the device and the counters are zeroed on the stream.  `more`: a buffer of the caller's
    // own that is allocated among the frame's.
    int begin(const std::vector<int32_t>& ids, const std::vector<msfm_pose_rt>& list, std::initializer_list<const std::vector<unsigned char>*> tables,
              size_t counter_bytes, TmpBuf* more = nullptr, size_t more_bytes = 0) {
        std::vector<msfm_pose_rt> by_rank;
        std::vector<TriImage> table;
        if (const int rc = tri_tables(ctx, who, &ts.tri_camera, ids.data(), list.data(), (int)ids.size(), prm, &by_rank, &table))
            return rc;   // (a posed image of the session lost its keypoints)
        // every check has passed: the registrations and the pose refinement's records describe the map as it was
        ts.reg_valid = ts.rp_valid = false;
        HIPCHK(ctx, hipSetDevice(ctx->device));
        had_mask = ts.mask_valid;
        HIPCHK(ctx, ev.create());
        HIPCHK(ctx, bytes.ensure(tables.size() * by_rank.size()));
        HIPCHK(ctx, counters.ensure(counter_bytes));
        HIPCHK(ctx, obs.ensure((size_t)std::max<long long>(1, O) * sizeof(msfm_ref::Obs)));
        if (more) HIPCHK(ctx, more->ensure(more_bytes));
        HIPCHK(ctx, ts.t_mask.ensure((size_t)std::max<long long>(1, O)));
        HIPCHK(ctx, pt.upload(ts.tri_camera, by_rank, table, (int)ts.nd.ids.size()));
        // (synchronous copies, like upload's: nothing queued reads host memory that an early return would free)
        size_t k = 0;
        for (const std::vector<unsigned char>* b : tables)
            HIPCHK(ctx, hipMemcpy(bytes.as<unsigned char>() + k++ * b->size(), b->data(), b->size(), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemsetAsync(counters.p, 0, counter_bytes, st));
        return MSFM_OK;
    }

    // ev[0], the prepared poses, the inlier bytes where the session had none (ext_mask_kernel under `d_gained`, one byte per rank),
    // the per-observation array under them, ev[1]
    int observe(const unsigned char* d_gained) {
        HIPCHK(ctx, hipEventRecord(ev[0], st));
        HIPCHK(ctx, pt.prepare(st));
        if (T > 0 && O > 0) {
            if (!had_mask) {
                hipLaunchKernelGGL(ext_mask_kernel, dim3(grid), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(),
                                   (const int*)ts.r_img.as<int>(), (int)T, pt.d_table(), pt.d_poses(), d_gained,
                                   (const msfm_point3d*)ts.t_points.as<msfm_point3d>(), ts.t_mask.as<unsigned char>());
                wrote(hipGetLastError());
            }
            if (queued == hipSuccess) wrote(launch_ref_obs(ctx, pt, ts.t_mask.as<unsigned char>(), obs.as<msfm_ref::Obs>(), st));
        }
        if (queued == hipSuccess) wrote(hipEventRecord(ev[1], st));
        return MSFM_OK;
    }

    // ev[2] and the call's last wait.  An error latched since the first write drops the points and the bytes: they may be half
    // rewritten.  Otherwise the session has inlier bytes from here on.
    int finish() {
        if (queued == hipSuccess) wrote(hipEventRecord(ev[2], st));
        wrote(hipStreamSynchronize(st));
        if (queued != hipSuccess) ts.tri_valid = ts.mask_valid = false;
        HIPCHK(ctx, queued);
        ts.mask_valid = true;
        return MSFM_OK;
    }

    // after finish: ev[0] .. ev[1] and ev[0] .. ev[2]
    hipError_t elapsed(double* prepare_ms, double* all_ms) const {
        float prep = 0.f, all = 0.f;
        hipError_t e = hipEventElapsedTime(&prep, ev[0], ev[1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&all, ev[0], ev[2]);
        *prepare_ms = prep;
        *all_ms = all;
        return e;
    }
};

int extend_impl(msfm_ctx* ctx, const int32_t* image_ids, const msfm_pose_rt* poses, int n_poses, const msfm_extend_params* params,
                msfm_extend_stats* stats) {
    TrackSession& ts = ctx->tracks;
    const std::string who = "msfm_extend_points";
    if (const int rc = tri_session_check(ctx, who, true)) return rc;
    const int max_hyp = params ? params->max_hypotheses : 0;
    if (max_hyp < 0 || max_hyp > 1024) return fail(ctx, MSFM_E_INVALID, who + ": max_hypotheses must lie in 0 .. 1024");
    if (n_poses < 0 || (n_poses > 0 && (!image_ids || !poses))) return fail(ctx, MSFM_E_INVALID, who + ": bad pose list");
    // the enlarged pose list: nothing of the session is touched before every check has passed
    const int n_img = (int)ts.nd.ids.size();
    std::vector<int> at_of((size_t)std::max(n_img, 1), -1);   // rank -> position in the session's pose list
    for (size_t k = 0; k < ts.tri_ids.size(); ++k) at_of[(size_t)ts.rank_of[(size_t)ts.tri_ids[k]]] = (int)k;
    std::vector<int32_t> ids = ts.tri_ids;
    std::vector<msfm_pose_rt> list = ts.tri_poses;
    std::vector<unsigned char> gained((size_t)std::max(n_img, 1), 0), given((size_t)std::max(n_img, 1), 0);
    long long added = 0;
    for (int k = 0; k < n_poses; ++k) {   // (not rank_bytes: each id's own checks come before the next id's)
        const int id = image_ids[k];
        if (!ts.declares(id)) return fail(ctx, MSFM_E_INVALID, who + ": image not declared in the session: " + std::to_string(id));
        const int r = ts.rank_of[(size_t)id];
        if (given[(size_t)r]) return fail(ctx, MSFM_E_INVALID, who + ": an image is given twice: " + std::to_string(id));
        given[(size_t)r] = 1;
        const int at = at_of[(size_t)r];
        if (at >= 0 && ts.tri_poses[(size_t)at].valid)
            return fail(ctx, MSFM_E_INVALID, who + ": the image already has a pose in the session (msfm_refine_poses or a full triangulation changes one): " + std::to_string(id));
        if (!poses[k].valid) continue;
        for (double v : poses[k].R)
            if (!std::isfinite(v)) return fail(ctx, MSFM_E_INVALID, who + ": non-finite R of image " + std::to_string(id));
        for (double v : poses[k].t)
            if (!std::isfinite(v)) return fail(ctx, MSFM_E_INVALID, who + ": non-finite t of image " + std::to_string(id));
        if (ctx->images[(size_t)id].nk < ts.nd.rows[(size_t)r])
            return fail(ctx, MSFM_E_NOIMAGE, who + ": posed image without keypoints (msfm_upload_keypoints): " + std::to_string(id));
        msfm_pose_rt p = poses[k];
        p.valid = 1;
        p.reserved = 0;
        if (at >= 0) {
            list[(size_t)at] = p;
        } else {
            ids.push_back(id);
            list.push_back(p);
        }
        gained[(size_t)r] = 1;
        added += 1;
    }
    TmpBuf t_list, t_positions;   // the retry list | its length, and trr_retry_kernel's scratch (released behind the frame's events)
    MapEditFrame fr(ctx, who);
    const long long T = fr.T, O = fr.O;
    hipStream_t st = fr.st;
    if (const int rc = fr.begin(ids, list, {&gained}, sizeof(ExtCounters) + sizeof(TrrCounters),   // this file's counters | the retry kernel's
                                &t_list, (size_t)(std::max<long long>(1, T) + 1) * sizeof(int)))   // the list | its length
        return rc;
    ExtCounters* d_ext = fr.counters.as<ExtCounters>();
    TrrCounters* d_trr = reinterpret_cast<TrrCounters*>(d_ext + 1);
    int* d_list = t_list.as<int>();
    int* d_listed = d_list + std::max<long long>(1, T);
    HIPCHK(ctx, hipMemsetAsync(d_listed, 0, sizeof(int), st));
    if (const int rc = fr.observe(fr.d_bytes(0))) return rc;
    const PoseTables& pt = fr.pt;
    int listed = 0;
    if (fr.live()) {
        hipLaunchKernelGGL(ext_track_kernel, dim3(fr.grid), dim3(256), 0, st, (const long long*)ts.r_offsets.as<long long>(),
                           (const int*)ts.r_img.as<int>(), (const int*)ts.r_idx.as<int>(), (const unsigned char*)ts.r_cons.as<unsigned char>(), (int)T,
                           (const msfm_ref::Obs*)fr.obs.as<msfm_ref::Obs>(), pt.d_table(), pt.d_poses(), fr.d_bytes(0), pt.cam, fr.prm,
                           max_hyp > 0 ? 1 : 0, ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(), ts.t_mask.as<unsigned char>(), d_list,
                           d_listed, d_ext);
        fr.wrote(hipGetLastError());
        if (max_hyp > 0 && fr.queued == hipSuccess) {
            if (fr.wrote(hipMemcpyAsync(&listed, d_listed, sizeof(int), hipMemcpyDeviceToHost, st)))
                fr.wrote(hipStreamSynchronize(st));   // the first wait: the length of the retry list
            if (fr.queued != hipSuccess) listed = 0;
        }
    }
    if (listed > 0 && fr.wrote(t_positions.ensure((size_t)O * sizeof(int)))) {
        const msfm_tri::RobustParams rp = {fr.prm.max_error, fr.prm.min_angle, fr.prm.min_views, max_hyp};
        const unsigned groups = (unsigned)((listed + kTrrWaves - 1) / kTrrWaves);
        const unsigned rgrid = std::min<unsigned>(groups, (unsigned)(kTrrGroupsPerCU * std::max(1, ctx->cu_count)));
        hipLaunchKernelGGL(trr_retry_kernel, dim3(rgrid), dim3(64 * kTrrWaves), 0, st, (const long long*)ts.r_offsets.as<long long>(),
                           (const int*)ts.r_img.as<int>(), (const int*)ts.r_idx.as<int>(), pt.d_table(),
                           pt.d_poses(), pt.cam, rp, (const int*)d_list, listed, t_positions.as<int>(),
                           ts.t_points.as<msfm_point3d>(), ts.t_resid.as<double>(), ts.t_mask.as<unsigned char>(), d_trr);
        if (fr.wrote(hipGetLastError())) {
            hipLaunchKernelGGL(ext_mark_kernel, dim3((unsigned)((listed + 255) / 256)), dim3(256), 0, st, (const int*)d_list, listed,
                               ts.t_points.as<msfm_point3d>());
            fr.wrote(hipGetLastError());
        }
    }
    if (const int rc = fr.finish()) return rc;
    ts.tri_ids.swap(ids);   // (the records describe the enlarged list from here on, whatever the copies below return)
    ts.tri_poses.swap(list);
    ExtCounters hc = {};
    TrrCounters hr = {};
    HIPCHK(ctx, hipMemcpy(&hc, d_ext, sizeof(hc), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(&hr, d_trr, sizeof(hr), hipMemcpyDeviceToHost));
    msfm_extend_stats s = {};
    HIPCHK(ctx, fr.elapsed(&s.prepare_ms, &s.extend_ms));
    s.images_added = added;
    s.tracks_touched = (int64_t)hc.tracks_touched;
    s.continued = (int64_t)hc.continued;
    s.observations_added = (int64_t)hc.observations_added;
    s.observations_rejected = (int64_t)hc.observations_rejected;
    s.created_attempted = (int64_t)hc.created_attempted;
    s.created = (int64_t)(hc.created + hr.tri[5]);   // (every track the retry kernel rewrites is a created one)
    s.retried = (int64_t)hr.retried;
    s.succeeded = (int64_t)(hc.succeeded + hr.tri[5]);
    s.observations_used = (int64_t)(hc.observations_used + hr.tri[6]);
    if (stats) *stats = s;
    return MSFM_OK;
}

}  // namespace

