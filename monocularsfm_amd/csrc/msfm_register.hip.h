// msfm_register.hip.h -- image registration on the device (include/msfm_match.h "image registration"): the kernels
// and the host side of msfm_register_images / msfm_fetch_registrations (defined in msfm_match.hip).  The arithmetic is msfm_register.h,
// shared with the host twin RegisterImages: the same bits.  Included by msfm_match.hip behind msfm_triangulate.hip.h.
//
// Everything runs on the library's stream between two HIP events; the host waits once, for the number of correspondences (the size
// of the results), before the rounds, and never between rounds (the staged arrangement of msfm_verify_staged.hip.h, one "pair" = one
// listed image):
//   reg_key_kernel      one lane per keypoint slot of a listed image: the keypoint's kept track (the session's node -> track table)
//                       and that track's record; a usable one gives the 64-bit key (list position << 32 | track number) and the
//                       value keypoint index, every other slot the key of a position one past the list.
//   rocprim radix sort  by key: the correspondences of every listed image, images in list order, by ascending track number -- the
//                       definition's order -- compact at the front.
//   reg_offsets_kernel  one lane per list position: the lower bound of its first key = the image's offset; the count the stopping
//                       rule sees (0 for an image that is not ATTEMPTED: the staged core then never lists it).
//   reg_fill_kernel     one lane per correspondence: (u, v) by undistort, X from the record, the track number -- a structure of
//                       arrays in correspondence order, so that the rounds read independent coalesced data instead of section 15's
//                       three-deep gather.
//   staged_decide_kernel<3, 64>   the staged core by instantiation.
//   reg_round_kernel    64 lanes = the 64 hypotheses of round r of a listed image, kRegGroupsPerCU workgroups per CU walking the list.
//                       Each lane solves its sample (the quartic's coefficient arrays are indexed by compile-time constants only:
//                       registers), leaves its <= 4 poses in LDS (lane-interleaved, 24 KiB), then the image's correspondences pass
//                       through LDS in tiles of kRegTile (10 KiB) and every lane counts the inliers of each of its poses from
//                       broadcast reads.  34 KiB per workgroup: four workgroups, one wave per SIMD, fit a CU's 160 KiB.
//   reg_finish_kernel   one wave per listed image: the rounds the rule needed (lane r replays with the counts of r + 1 rounds), the
//                       winner re-solved, its best pose, the ordered inlier list by ballots, the refinement with lane j holding
//                       partial j and the butterfly by cross-lane shuffles, the final flags, residuals and record.
// Plain vector loads and stores; the stats' counters are reduced per wave and added with one vector atomic each.
#pragma once
#include "msfm_register.h"
#include "msfm_triangulate.hip.h"
#include "msfm_verify_staged.hip.h"

namespace msfm {

constexpr int kRegTile = 256;          // correspondences staged in LDS at a time (5 double arrays = 10 KiB)
constexpr int kRegGroupsPerCU = 4;     // reg_round_kernel workgroups resident per CU (LDS-bound: 34 KiB each)

struct RegImage {
    const float2* kxy;     // the image's keypoints
    long long slot_base;   // its first keypoint slot (the running sum of the listed images' rows)
    int node_base;         // its first node of the track session
    int image_id;
};

struct RegCounters {
    int attempted, succeeded;
};

__global__ __launch_bounds__(256) void reg_key_kernel(const RegImage* __restrict__ imgs, int n_images, long long n_slots,
                                                      const int* __restrict__ r_tid, const msfm_point3d* __restrict__ points,
                                                      unsigned long long* __restrict__ keys, int* __restrict__ vals) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n_slots; g += stride) {
        int lo = 0, hi = n_images - 1;   // the last image whose slot_base <= g
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (imgs[mid].slot_base <= g) lo = mid;
            else hi = mid - 1;
        }
        const int k = (int)(g - imgs[lo].slot_base);
        const int tid = r_tid[imgs[lo].node_base + k];
        bool use = tid >= 0;
        if (use) {
            const int want = MSFM_TRI_POINT | MSFM_TRI_ERROR_OK | MSFM_TRI_ANGLE_OK;
            use = (points[tid].status & want) == want;
        }
        keys[g] = use ? (((unsigned long long)lo << 32) | (unsigned long long)(unsigned)tid) : ((unsigned long long)n_images << 32);
        vals[g] = k;
    }
}

__device__ __forceinline__ long long reg_lower_bound(const unsigned long long* __restrict__ keys, long long n, unsigned long long key) {
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void reg_offsets_kernel(const unsigned long long* __restrict__ keys, long long n_slots, int n_images,
                                                          int min_inliers, long long* __restrict__ offsets, int* __restrict__ counts_eff) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_images) return;
    const long long b = reg_lower_bound(keys, n_slots, (unsigned long long)j << 32);
    offsets[j] = b;
    if (j < n_images) {
        const int n = (int)(reg_lower_bound(keys, n_slots, (unsigned long long)(j + 1) << 32) - b);
        counts_eff[j] = msfm_reg::attempted(n, min_inliers) ? n : 0;
    }
}

__global__ __launch_bounds__(256) void reg_fill_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ vals, long long M,
                                                       const RegImage* __restrict__ imgs, const msfm_point3d* __restrict__ points,
                                                       msfm_emat::Camera cam, double* __restrict__ cu, double* __restrict__ cv,
                                                       double* __restrict__ cX, double* __restrict__ cY, double* __restrict__ cZ,
                                                       int* __restrict__ ctid) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += stride) {
        const unsigned long long key = keys[i];
        const int j = (int)(key >> 32), tid = (int)(unsigned)(key & 0xffffffffull);
        const float2 q = imgs[j].kxy[vals[i]];
        double u, v;
        msfm_emat::undistort(cam, (double)q.x, (double)q.y, &u, &v);
        cu[i] = u;
        cv[i] = v;
        cX[i] = points[tid].X[0];
        cY[i] = points[tid].X[1];
        cZ[i] = points[tid].X[2];
        ctid[i] = tid;
    }
}

// the sample of hypothesis `it` of an image whose correspondences start at the given arrays
__device__ __forceinline__ void reg_load_sample(const double* __restrict__ cu, const double* __restrict__ cv, const double* __restrict__ cX,
                                                const double* __restrict__ cY, const double* __restrict__ cZ, int n, int image_id, int it,
                                                double u[3], double v[3], double X[9]) {
    int idx[3];
    msfm_reg::sample3(msfm_reg::reg_seed(image_id), it, n, idx);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u[k] = cu[idx[k]];
        v[k] = cv[idx[k]];
        X[3 * k] = cX[idx[k]];
        X[3 * k + 1] = cY[idx[k]];
        X[3 * k + 2] = cZ[idx[k]];
    }
}

// round prm.round of the images listed for it (list[(round & 1) * n ..], count[round & 1]); prm.thr2 = max_error^2
__global__ __launch_bounds__(msfm_reg::kRegRound) void reg_round_kernel(
    const long long* __restrict__ offsets, const int* __restrict__ counts_eff, const RegImage* __restrict__ imgs, const double* __restrict__ cu,
    const double* __restrict__ cv, const double* __restrict__ cX, const double* __restrict__ cY, const double* __restrict__ cZ,
    int* __restrict__ list, int n_images, int* __restrict__ hyp_counts, StagedParams prm, double f2, StagedStats* __restrict__ stats) {
    using namespace msfm_reg;
    __shared__ double ws[48 * kRegRound];
    __shared__ double su[kRegTile], sv[kRegTile], sX[kRegTile], sY[kRegTile], sZ[kRegTile];
    const int t = threadIdx.x;
    int* count = list + 2 * n_images;
    const int listed = count[prm.round & 1];
    const int* mine = list + (prm.round & 1) * n_images;
    if (blockIdx.x == 0 && t == 0) count[(prm.round + 1) & 1] = 0;   // (the next round's list: filled after this round)
    const int it = prm.round * kRegRound + t;
    const bool live = it < prm.max_iters;
    unsigned long long solved = 0;
    for (int k = blockIdx.x; k < listed; k += gridDim.x) {   // (uniform over the workgroup)
        const int p = mine[k];
        const int n = counts_eff[p];
        const long long base = offsets[p];
        int ns = 0;
        if (live) {
            double u[3], v[3], X[9];
            reg_load_sample(cu + base, cv + base, cX + base, cY + base, cZ + base, n, imgs[p].image_id, it, u, v, X);
            ns = p3p<kRegRound>(u, v, X, ws + t);
        }
        int c[4] = {0, 0, 0, 0};
        for (int c0 = 0; c0 < n; c0 += kRegTile) {
            const int m = min(kRegTile, n - c0);
            __syncthreads();
            for (int i = t; i < m; i += kRegRound) {
                su[i] = cu[base + c0 + i];
                sv[i] = cv[base + c0 + i];
                sX[i] = cX[base + c0 + i];
                sY[i] = cY[base + c0 + i];
                sZ[i] = cZ[base + c0 + i];
            }
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (s >= ns) continue;
                double R[9], tt[3];
#pragma unroll
                for (int q = 0; q < 9; ++q) R[q] = ws[(12 * s + q) * kRegRound + t];
#pragma unroll
                for (int q = 0; q < 3; ++q) tt[q] = ws[(12 * s + 9 + q) * kRegRound + t];
                int cc = 0;
                for (int i = 0; i < m; ++i)   // every lane reads the same address: LDS broadcast
                    cc += inlier(R, tt, su[i], sv[i], sX[i], sY[i], sZ[i], f2, prm.thr2) ? 1 : 0;
                c[s] += cc;
            }
        }
        const int best = max(max(c[0], c[1]), max(c[2], c[3]));
        if (live) hyp_counts[(long long)p * prm.max_iters + it] = best;
        solved += live ? 1 : 0;
        __syncthreads();   // (the next image's staging overwrites the tile)
    }
    const unsigned long long c[1] = {solved};
    wave_add_counters(c, &stats->solved);
}

// the number of set flags over the wave, the same in every lane
__device__ __forceinline__ int reg_wave_count(bool flag) { return __popcll(__ballot(flag)); }

__global__ __launch_bounds__(64) void reg_finish_kernel(const long long* __restrict__ offsets, const RegImage* __restrict__ imgs,
                                                        const double* __restrict__ cu_, const double* __restrict__ cv_,
                                                        const double* __restrict__ cX_, const double* __restrict__ cY_,
                                                        const double* __restrict__ cZ_, const int* __restrict__ hyp_counts,
                                                        msfm_reg::Params prm, double f, int* __restrict__ inl_list,
                                                        msfm_registration* __restrict__ records, unsigned char* __restrict__ flags,
                                                        double* __restrict__ residuals, RegCounters* __restrict__ counters) {
    using namespace msfm_reg;
    __shared__ double ws[48];
    __shared__ int s_ns;
    const int p = blockIdx.x, lane = threadIdx.x;
    const long long base = offsets[p];
    const int n = (int)(offsets[p + 1] - base);
    const int image_id = imgs[p].image_id;
    const double *cu = cu_ + base, *cv = cv_ + base, *cX = cX_ + base, *cY = cY_ + base, *cZ = cZ_ + base;
    msfm_registration rec;
    clear_record(&rec, image_id, n);
    for (int i = lane; i < n; i += 64) {
        flags[base + i] = 0;
        residuals[base + i] = -1.0;
    }
    if (!attempted(n, prm.min_inliers)) {
        if (lane == 0) records[p] = rec;
        return;
    }
    rec.status = MSFM_REG_ATTEMPTED;
    // the rounds the stopping rule needed: lane l replays with the counts of chunk * 64 + l + 1 rounds.  staged_decide_kernel has
    // the winner already (best_it) but not the ROUND it was decided in, which the record's `hypotheses` needs and which the shared
    // core has no slot for; the replay is repeated here, all candidate rounds at once, rather than changing the core.  Lanes past the
    // decided round read counts of rounds that never ran (zeroed by the host side); the first decided lane is taken, theirs are ignored.
    const int* hc = hyp_counts + (long long)p * prm.max_iters;
    const int total_rounds = (prm.max_iters + kRegRound - 1) / kRegRound;
    int best_it = -1, rounds = total_rounds;
    for (int chunk = 0; chunk * 64 < total_rounds; ++chunk) {
        const int r = chunk * 64 + lane + 1;
        bool decided = false;
        int bc = 0, bi = -1;
        if (r <= total_rounds) {
            const int avail = min(r * kRegRound, prm.max_iters);
            bi = msfm_fmat::replay_adaptive<3>(n, prm.max_iters, prm.confidence, [&](int i) { return hc[i]; }, &bc, avail, &decided);
        }
        const unsigned long long bal = __ballot(decided);
        if (bal) {
            const int first = __ffsll((long long)bal) - 1;
            best_it = __shfl(bi, first, 64);
            rounds = chunk * 64 + first + 1;
            break;
        }
    }
    rec.hypotheses = min(rounds * kRegRound, prm.max_iters);
    if (best_it < 0) {
        if (lane == 0) {
            records[p] = rec;
            atomicAdd(&counters->attempted, 1);
        }
        return;
    }
    const double f2 = f * f, thr2 = prm.max_error * prm.max_error;
    if (lane == 0) {
        double u[3], v[3], X[9];
        reg_load_sample(cu, cv, cX, cY, cZ, n, image_id, best_it, u, v, X);
        s_ns = p3p<1>(u, v, X, ws);
    }
    __syncthreads();
    const int ns = s_ns;
    int b = 0, bcount = 0;
    for (int s = 0; s < ns; ++s) {
        double R[9], t[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = ws[12 * s + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = ws[12 * s + 9 + k];
        int c = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            c += reg_wave_count(i < n && inlier(R, t, cu[i], cv[i], cX[i], cY[i], cZ[i], f2, thr2));
        }
        if (c > bcount) {
            bcount = c;
            b = s;
        }
    }
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = ns > 0 ? ws[12 * b + k] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = ns > 0 ? ws[12 * b + 9 + k] : 0.0;
    // the ordered inlier list of the winner
    int* list = inl_list + base;
    int ni = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < n && inlier(R, t, cu[i], cv[i], cX[i], cY[i], cZ[i], f2, thr2);
        const unsigned long long bal = __ballot(in);
        if (in) list[ni + __popcll(bal & ((1ull << lane) - 1ull))] = i;
        ni += __popcll(bal);
    }
    __threadfence_block();
    __syncthreads();
    int status = MSFM_REG_ATTEMPTED | MSFM_REG_POSE;
    if (prm.refine_iters > 0) {
        double Rr[9], tr[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rr[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tr[k] = t[k];
        for (int step = 0; step < prm.refine_iters; ++step) {
            double acc[kRegSums];
#pragma unroll
            for (int k = 0; k < kRegSums; ++k) acc[k] = 0.0;
            for (int pos = lane; pos < ni; pos += 64) {
                const int i = list[pos];
                gn_add(Rr, tr, cu[i], cv[i], cX[i], cY[i], cZ[i], acc);
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1)
#pragma unroll
                for (int k = 0; k < kRegSums; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], s, 64);
            if (!gn_step(acc, Rr, tr)) break;   // (uniform: every lane holds the same sums)
        }
        int cr = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            cr += reg_wave_count(i < n && inlier(Rr, tr, cu[i], cv[i], cX[i], cY[i], cZ[i], f2, thr2));
        }
        if (cr >= ni) {
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = Rr[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = tr[k];
            status |= MSFM_REG_REFINED;
        }
    }
    int nf = 0;
    double sum = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        bool in = false;
        double e = 0.0;
        if (i < n) {
            in = inlier(R, t, cu[i], cv[i], cX[i], cY[i], cZ[i], f2, thr2);
            e = residual(R, t, cu[i], cv[i], cX[i], cY[i], cZ[i], f);
            flags[base + i] = in ? 1 : 0;
            residuals[base + i] = msfm_pose::canonical(e);
        }
        unsigned long long bal = __ballot(in);
        nf += __popcll(bal);
        while (bal) {   // the inliers' residuals in list order (uniform over the wave)
            const int src = __ffsll((long long)bal) - 1;
            sum = sum + __shfl(e, src, 64);
            bal &= bal - 1ull;
        }
    }
    if (nf >= prm.min_inliers) status |= MSFM_REG_SUCCEEDED;
    if (lane == 0) {
        rec.status = status;
        rec.n_inliers = nf;
#pragma unroll
        for (int k = 0; k < 9; ++k) rec.R[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) rec.t[k] = t[k];
        rec.mean_residual = nf > 0 ? sum / (double)nf : 0.0;
        records[p] = rec;
        atomicAdd(&counters->attempted, 1);
        if (status & MSFM_REG_SUCCEEDED) atomicAdd(&counters->succeeded, 1);
    }
}

}  // namespace msfm

namespace {

int register_impl(msfm_ctx* ctx, const msfm_camera* camera, const int32_t* image_ids, int n_images, const msfm_register_params* params,
                  msfm_register_stats* stats) {
    TrackSession& ts = ctx->tracks;
    ts.reg_valid = false;   // whatever happens below, the previous registrations are gone
    if (const int rc = tri_session_check(ctx, "msfm_register_images", true)) return rc;
    if (!camera) return fail(ctx, MSFM_E_INVALID, "msfm_register_images: NULL camera");
    const msfm_camera c = *camera;
    for (double v : {c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2})
        if (!std::isfinite(v)) return fail(ctx, MSFM_E_INVALID, "msfm_register_images: camera parameters must be finite");
    if (!(c.fx > 0.0) || !(c.fy > 0.0)) return fail(ctx, MSFM_E_INVALID, "msfm_register_images: fx and fy must be positive");
    msfm_reg::Params prm = {4.0, 0.9999, 1024, 15, 10, 0};   // Registrant.h:22-26; max_iters is this library's
    if (params) prm = msfm_reg::Params{params->max_error, params->confidence, params->max_iters, params->min_inliers, params->refine_iters, 0};
    if (!std::isfinite(prm.max_error) || prm.max_error < 0.0) return fail(ctx, MSFM_E_INVALID, "msfm_register_images: max_error must be finite and not negative");
    if (!(prm.confidence > 0.0 && prm.confidence < 1.0)) return fail(ctx, MSFM_E_INVALID, "msfm_register_images: confidence must lie in (0, 1)");
    if (prm.max_iters < 1 || prm.max_iters > 65536) return fail(ctx, MSFM_E_INVALID, "msfm_register_images: max_iters must lie in 1 .. 65536");
    if (prm.min_inliers < 0) return fail(ctx, MSFM_E_INVALID, "msfm_register_images: min_inliers must not be negative");
    if (prm.refine_iters < 0 || prm.refine_iters > 100) return fail(ctx, MSFM_E_INVALID, "msfm_register_images: refine_iters must lie in 0 .. 100");
    if (n_images < 0 || (n_images > 0 && !image_ids)) return fail(ctx, MSFM_E_INVALID, "msfm_register_images: bad image list");
    std::vector<RegImage> imgs((size_t)std::max(n_images, 1), RegImage{nullptr, 0, 0, 0});
    std::vector<char> given((size_t)MSFM_MAX_IMAGES, 0);
    long long n_slots = 0;
    for (int k = 0; k < n_images; ++k) {
        const int id = image_ids[k];
        if (!ts.declares(id)) return fail(ctx, MSFM_E_NOIMAGE, "msfm_register_images: image not declared in the session: " + std::to_string(id));
        if (given[(size_t)id]) return fail(ctx, MSFM_E_INVALID, "msfm_register_images: an image is given twice: " + std::to_string(id));
        given[(size_t)id] = 1;
        const int r = ts.rank_of[(size_t)id], rows = ts.nd.rows[(size_t)r];
        const Image& im = ctx->images[(size_t)id];
        if (im.nk < rows || (rows > 0 && !im.kxy))
            return fail(ctx, MSFM_E_NOIMAGE, "msfm_register_images: image without keypoints (msfm_upload_keypoints): " + std::to_string(id));
        imgs[(size_t)k] = RegImage{im.kxy, n_slots, (int)ts.nd.base[(size_t)r], id};
        n_slots += rows;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    struct {   // (the temporaries are freed when the call returns, whatever it returns)
        TmpBuf imgs, keys, vals, keys2, vals2, sort_tmp, counts, cu, cv, cX, cY, cZ, hyp, state, best_it, best_count, sstats, inl, counters;
    } t;
    TmpEvents<2> ev;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, ev.create());
    const size_t N = (size_t)std::max(n_images, 1), S = (size_t)std::max<long long>(1, n_slots);
    HIPCHK(ctx, t.imgs.ensure(N * sizeof(RegImage)));
    HIPCHK(ctx, t.keys.ensure(S * 8));
    HIPCHK(ctx, t.keys2.ensure(S * 8));
    HIPCHK(ctx, t.vals.ensure(S * 4));
    HIPCHK(ctx, t.vals2.ensure(S * 4));
    HIPCHK(ctx, t.counts.ensure(N * 4));
    HIPCHK(ctx, t.counters.ensure(sizeof(RegCounters)));
    HIPCHK(ctx, t.sstats.ensure(sizeof(StagedStats)));
    HIPCHK(ctx, ts.g_offsets.ensure((N + 1) * 8));
    HIPCHK(ctx, ts.g_records.ensure(N * sizeof(msfm_registration)));
    // (a synchronous copy of the small table: nothing queued reads host memory that an early return below would free)
    HIPCHK(ctx, hipMemcpy(t.imgs.p, imgs.data(), N * sizeof(RegImage), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemsetAsync(t.counters.p, 0, sizeof(RegCounters), st));
    HIPCHK(ctx, hipMemsetAsync(t.sstats.p, 0, sizeof(StagedStats), st));
    HIPCHK(ctx, hipMemsetAsync(ts.g_offsets.p, 0, (N + 1) * 8, st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    const RegImage* d_imgs = t.imgs.as<RegImage>();
    const msfm_point3d* d_points = ts.t_points.as<msfm_point3d>();
    unsigned long long *keys = t.keys.as<unsigned long long>(), *keys2 = t.keys2.as<unsigned long long>();
    long long M = 0;
    if (n_images > 0 && n_slots > 0) {
        hipLaunchKernelGGL(reg_key_kernel, dim3(tk_grid(ctx, n_slots)), dim3(256), 0, st, d_imgs, n_images, n_slots, (const int*)ts.r_tid.as<int>(),
                           d_points, keys, t.vals.as<int>());
        HIPCHK(ctx, hipGetLastError());
        unsigned bits = 1;
        while (bits < 31 && (1ll << bits) <= (long long)n_images) ++bits;   // the position one past the list sorts too
        size_t tmp_bytes = 0;
        HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys, keys2, t.vals.as<int>(), t.vals2.as<int>(), (size_t)n_slots, 0u, 32u + bits, st));
        HIPCHK(ctx, t.sort_tmp.ensure(std::max<size_t>(tmp_bytes, 256)));
        HIPCHK(ctx, rocprim::radix_sort_pairs(t.sort_tmp.p, tmp_bytes, keys, keys2, t.vals.as<int>(), t.vals2.as<int>(), (size_t)n_slots, 0u, 32u + bits, st));
        hipLaunchKernelGGL(reg_offsets_kernel, dim3((unsigned)((n_images + 256) / 256)), dim3(256), 0, st, (const unsigned long long*)keys2, n_slots,
                           n_images, prm.min_inliers, ts.g_offsets.as<long long>(), t.counts.as<int>());
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&M, ts.g_offsets.as<long long>() + n_images, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));   // the one wait: the size of everything below
    } else {
        HIPCHK(ctx, hipMemsetAsync(t.counts.p, 0, N * 4, st));
    }
    const size_t Mz = (size_t)std::max<long long>(1, M);
    for (TmpBuf* b : {&t.cu, &t.cv, &t.cX, &t.cY, &t.cZ}) HIPCHK(ctx, b->ensure(Mz * 8));
    HIPCHK(ctx, t.inl.ensure(Mz * 4));
    HIPCHK(ctx, ts.g_tid.ensure(Mz * 4));
    HIPCHK(ctx, ts.g_inl.ensure(Mz));
    HIPCHK(ctx, ts.g_res.ensure(Mz * 8));
    const msfm_emat::Camera cam{c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2};
    const double f = (c.fx + c.fy) / 2.0;
    if (M > 0) {
        hipLaunchKernelGGL(reg_fill_kernel, dim3(tk_grid(ctx, M)), dim3(256), 0, st, (const unsigned long long*)keys2, (const int*)t.vals2.as<int>(), M,
                           d_imgs, d_points, cam, t.cu.as<double>(), t.cv.as<double>(), t.cX.as<double>(), t.cY.as<double>(), t.cZ.as<double>(),
                           ts.g_tid.as<int>());
        HIPCHK(ctx, hipGetLastError());
    }
    if (n_images > 0) {
        const size_t P = (size_t)n_images;
        HIPCHK(ctx, t.hyp.ensure(P * (size_t)prm.max_iters * 4));
        HIPCHK(ctx, t.state.ensure((3 * P + 2) * 4));   // state[P] | two image lists [P] | their two counts
        HIPCHK(ctx, t.best_it.ensure(P * 4));
        HIPCHK(ctx, t.best_count.ensure(P * 4));
        HIPCHK(ctx, hipMemsetAsync(t.state.p, 0, (3 * P + 2) * 4, st));
        HIPCHK(ctx, hipMemsetAsync(t.hyp.p, 0, P * (size_t)prm.max_iters * 4, st));   // (reg_finish_kernel's lanes past the decided round read defined zeros)
        int* state = t.state.as<int>();
        int* list = state + P;
        StagedStats* sstats = t.sstats.as<StagedStats>();
        StagedParams sp = {prm.max_error * prm.max_error, prm.confidence, prm.max_iters, -1, 0ull};
        const int rounds = (prm.max_iters + msfm_reg::kRegRound - 1) / msfm_reg::kRegRound;
        const unsigned grid = (unsigned)std::min<size_t>(P, (size_t)kRegGroupsPerCU * (size_t)std::max(1, ctx->cu_count));
        for (int r = -1; r < rounds; ++r) {
            sp.round = r;
            if (r >= 0) {
                hipLaunchKernelGGL(reg_round_kernel, dim3(grid), dim3(msfm_reg::kRegRound), 0, st, (const long long*)ts.g_offsets.as<long long>(),
                                   (const int*)t.counts.as<int>(), d_imgs, (const double*)t.cu.as<double>(), (const double*)t.cv.as<double>(),
                                   (const double*)t.cX.as<double>(), (const double*)t.cY.as<double>(), (const double*)t.cZ.as<double>(), list,
                                   n_images, t.hyp.as<int>(), sp, f * f, sstats);
                HIPCHK(ctx, hipGetLastError());
            }
            hipLaunchKernelGGL((staged_decide_kernel<3, msfm_reg::kRegRound>), dim3((unsigned)((P + 63) / 64)), dim3(64), 0, st,
                               (const int*)t.counts.as<int>(), (const int*)t.hyp.as<int>(), n_images, sp, state, list, t.best_it.as<int>(),
                               t.best_count.as<int>(), sstats);
            HIPCHK(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(reg_finish_kernel, dim3((unsigned)P), dim3(64), 0, st, (const long long*)ts.g_offsets.as<long long>(), d_imgs,
                           (const double*)t.cu.as<double>(), (const double*)t.cv.as<double>(), (const double*)t.cX.as<double>(),
                           (const double*)t.cY.as<double>(), (const double*)t.cZ.as<double>(), (const int*)t.hyp.as<int>(), prm, f, t.inl.as<int>(),
                           ts.g_records.as<msfm_registration>(), ts.g_inl.as<unsigned char>(), ts.g_res.as<double>(), t.counters.as<RegCounters>());
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    const hipError_t done = hipStreamSynchronize(st);   // (before anything returns: the temporaries die with this function)
    HIPCHK(ctx, done);
    RegCounters hc = {};
    StagedStats hs = {};
    HIPCHK(ctx, hipMemcpy(&hc, t.counters.p, sizeof(hc), hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(&hs, t.sstats.p, sizeof(hs), hipMemcpyDeviceToHost));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev[0], ev[1]));
    msfm_register_stats s = {};
    s.images = n_images;
    s.attempted = hc.attempted;
    s.succeeded = hc.succeeded;
    s.rounds = hs.rounds;
    s.correspondences = M;
    s.hypotheses = (int64_t)hs.solved;
    s.device_bytes = (int64_t)(ts.g_records.cap + ts.g_offsets.cap + ts.g_tid.cap + ts.g_inl.cap + ts.g_res.cap);
    s.register_ms = ms;
    ts.reg_valid = true;
    ts.reg_images = n_images;
    ts.reg_corr = M;
    if (stats) *stats = s;
    return MSFM_OK;
}

int fetch_registrations_impl(msfm_ctx* ctx, msfm_registration* out, int64_t* out_offsets, int32_t* out_track_ids, uint8_t* out_inlier,
                             double* out_residuals) {
    TrackSession& ts = ctx->tracks;
    if (!ts.open) return fail(ctx, MSFM_E_STATE, "msfm_fetch_registrations without a track session (msfm_tracks_begin)");
    if (!ts.finished || !ts.tri_valid || !ts.reg_valid)
        return fail(ctx, MSFM_E_STATE, "msfm_fetch_registrations without registrations: msfm_register_images has not run since the last msfm_triangulate_tracks");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)ts.reg_images, M = (size_t)ts.reg_corr;
    if (out && n) HIPCHK(ctx, hipMemcpy(out, ts.g_records.p, n * sizeof(msfm_registration), hipMemcpyDeviceToHost));
    if (out_offsets) HIPCHK(ctx, hipMemcpy(out_offsets, ts.g_offsets.p, (n + 1) * 8, hipMemcpyDeviceToHost));
    if (out_track_ids && M) HIPCHK(ctx, hipMemcpy(out_track_ids, ts.g_tid.p, M * 4, hipMemcpyDeviceToHost));
    if (out_inlier && M) HIPCHK(ctx, hipMemcpy(out_inlier, ts.g_inl.p, M, hipMemcpyDeviceToHost));
    if (out_residuals && M) HIPCHK(ctx, hipMemcpy(out_residuals, ts.g_res.p, M * 8, hipMemcpyDeviceToHost));
    return MSFM_OK;
}

}  // namespace
