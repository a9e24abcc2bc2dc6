// msfm_match.hip -- host side of the C ABI declared in include/msfm_match.h.
//
// Owns the device-resident descriptor store, schedules image pairs onto the gfx950 kernels in
// msfm_kernels.hip.h and returns match lists.  Mirrors what FeatureMatcher::MatchImagePairs
// (src/Feature/FeatureMatching.cpp:10-73 of the reference) does between its two
// Database::ReadDescriptors calls and FeatureUtils::FilterMatches, without the per-pair
// descriptor re-read.  No CPU fallback: every entry point that needs the GPU fails loudly
// when there is none.
#include "msfm_match.h"
#include "msfm_hostutil.h"
#include "msfm_guard.h"
#include "msfm_tracks.h"
#include "msfm_kernels.hip.h"
#include "msfm_prefilter.hip.h"
#include "msfm_verify.hip.h"
#include "msfm_verify_e.hip.h"
#include "msfm_verify_h.hip.h"
#include "msfm_verify_select.hip.h"
#include "msfm_verify_pose.hip.h"
#include "msfm_verify_pose_refine.hip.h"
#include "msfm_retrieval.hip.h"

#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

using namespace msfm;

#include "msfm_ctx.hip.h"
#include "msfm_store_host.hip.h"
#include "msfm_batch.hip.h"
#include "msfm_tracks.hip.h"
#include "msfm_triangulate.hip.h"
#include "msfm_triangulate_robust.hip.h"
#include "msfm_refine.hip.h"
#include "msfm_refine_poses.hip.h"
#include "msfm_refine_camera.hip.h"
#include "msfm_extend.hip.h"
#include "msfm_filter.hip.h"
#include "msfm_complete.hip.h"
#include "msfm_visibility.hip.h"
#include "msfm_align.hip.h"
#include "msfm_register.hip.h"

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

const char* msfm_version(void) { return "msfm-match 0.1 (gfx950)"; }

int msfm_device_count(void) {
    MSFM_API_BEGIN(nullptr)
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return 0;
    int usable = 0;
    for (int d = 0; d < count; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) break;
        ++usable;   // (ordinals are contiguous: the count of leading gfx950 devices)
    }
    return usable;
    MSFM_API_END
}

static void destroy_streams(msfm_ctx* ctx);
static MatchJob* new_match_job();
static void delete_match_job(MatchJob* j);

// The stream and the events of scratch set k exist.  A stream is a hardware queue: ~11 ms to create on this part -- msfm_create makes
// the first, a call that puts a second / third sub-batch in flight the others, at a moment when the device is busy with the sub-batch before
// and the host is ahead of it (the ComputeMatches executable on the South-Building job: one set for the pre-emptive filter, two for the
// pairs: 22 ms less in front of the first upload, 11 of them never spent).
int ensure_scratch_set(msfm_ctx* ctx, int k) {
    Scratch& sc = ctx->sc[k];
    if (sc.stream) return MSFM_OK;
    hipError_t e = hipSuccess;
    if ((e = hipStreamCreateWithFlags(&sc.stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sc.sweep1_done, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&sc.sweep2_done, hipEventDisableTiming)) != hipSuccess)
        return fail(ctx, MSFM_E_DEVICE, std::string("stream / events of a scratch set: ") + hipGetErrorString(e));
    return MSFM_OK;
}

// msfm_create behind the device checks: streams and events of the scratch sets, the kernels' LDS attributes, the zero row
static int create_rest(msfm_ctx* ctx) {
    auto bad = [ctx](const char* what, hipError_t e) { return fail(ctx, MSFM_E_DEVICE, std::string("msfm_create: ") + what + ": " + hipGetErrorString(e)); };
    hipError_t e = hipSuccess;
    // (the first scratch set's stream -- uploads and the store build use it as well; the other sets get theirs when a call first has
    // more than one sub-batch in flight: ensure_scratch_set)
    if (ensure_scratch_set(ctx, 0) != MSFM_OK) return MSFM_E_DEVICE;
    // dynamic LDS beyond 64 KiB: the brute-force kernel (108 KiB), the sweeps (94 / 124 KiB)
    struct { const void* f; int bytes; } attrs[] = {
        {reinterpret_cast<const void*>(dist_top2_kernel<0>), kLdsBytes},     {reinterpret_cast<const void*>(dist_top2_kernel<1>), kLdsBytes},
        {reinterpret_cast<const void*>(dist_top2_kernel<3>), kLdsBytesIdxStash},
        {reinterpret_cast<const void*>(sweep_kernel<1>), kPfLdsBytes},       {reinterpret_cast<const void*>(sweep_kernel<2>), kPfLdsBytes},
        {reinterpret_cast<const void*>(sweep_kernel<3>), kPfLdsBytes},       {reinterpret_cast<const void*>(sweep_kernel<4>), kPfLdsBytes},
        {reinterpret_cast<const void*>(sweep_i8_kernel<1>), kI8LdsBytes1},    {reinterpret_cast<const void*>(sweep_i8_kernel<3>), kI8LdsBytes3},
    };
    for (const auto& a : attrs)
        if ((e = hipFuncSetAttribute(a.f, hipFuncAttributeMaxDynamicSharedMemorySize, a.bytes)) != hipSuccess)
            return bad("cannot reserve the kernels' LDS", e);
    // the all-zero operand row the compacted sweep reads for rows without a source
    if ((e = ctx->d_zero_row.ensure(kPfRowBytes)) != hipSuccess || (e = hipMemset(ctx->d_zero_row.p, 0, kPfRowBytes)) != hipSuccess)
        return bad("the zero row", e);
    return MSFM_OK;
}

int msfm_create(int device_ordinal, msfm_ctx** out_ctx) {
    MSFM_API_BEGIN(nullptr)
    if (!out_ctx) return MSFM_E_INVALID;
    *out_ctx = nullptr;
    int count = 0;
    HostClock hc;   // MSFM_DEBUG_TIMING=1: where a context's creation goes (the runtime's own start-up is most of it)
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return MSFM_E_DEVICE;  // no GPU, no fallback
    hc.lap("create: hipGetDeviceCount");
    if (device_ordinal < 0 || device_ordinal >= count) return MSFM_E_INVALID;
    if (hipSetDevice(device_ordinal) != hipSuccess) return MSFM_E_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return MSFM_E_DEVICE;
    hc.lap("create: set device, properties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "msfm_create: device %d is %s, this library is built for gfx950 only\n",
                     device_ordinal, prop.gcnArchName);
        return MSFM_E_DEVICE;
    }
    msfm_ctx* ctx = new (std::nothrow) msfm_ctx();
    if (!ctx) return MSFM_E_DEVICE;
    ctx->device = device_ordinal;
    ctx->images.resize(kSlots);
    ctx->inbox.recycle = true;
    ctx->job = new_match_job();
    for (Scratch& sc : ctx->sc) {
        for (PinnedBuf& h : sc.h_up) h.pool = &ctx->pinned_pool;
        sc.h_summary.pool = sc.h_tail.pool = sc.h_tk_pairs.pool = &ctx->pinned_pool;
    }
    ctx->h_jobs.pool = ctx->h_store_maxima.pool = &ctx->pinned_pool;
    ctx->cu_count = prop.multiProcessorCount;
    ctx->clock_mhz = prop.clockRate / 1000;
    std::snprintf(ctx->dev_name, sizeof(ctx->dev_name), "%s (%s)", prop.name, prop.gcnArchName);
    // (Round 5 tried the streams of the other scratch sets, the kernel attributes and the zero row on a helper thread, joined by the first
    // matching call: 45 of msfm_create's 95 ms.  The runtime serialises them with the uploads the caller makes meanwhile -- the
    // ComputeMatches executable's bulk load went from 48 to 72 ms --, so nothing was gained: profiles/r05_cli_cold_call.txt.)
    if (create_rest(ctx) != MSFM_OK) {
        std::fprintf(stderr, "%s\n", ctx->err.c_str());
        destroy_streams(ctx);
        ctx->d_zero_row.release();
        delete_match_job(ctx->job);
        delete ctx;
        return MSFM_E_DEVICE;
    }
    hc.lap("create: streams, events, kernel attributes, zero row");
    if (const char* e = std::getenv("MSFM_PREFILTER")) ctx->prefilter = e[0] == '2' ? 2 : (e[0] != '0');
    if (const char* e = std::getenv("MSFM_MAX_PAIRS_PER_BATCH"))
        if (std::atoi(e) > 0) ctx->max_pairs_per_batch = std::min(std::atoi(e), kMaxPairsPerBatchLimit);
    if (const char* e = std::getenv("MSFM_PIPELINE_TAPER")) {
        const double t = std::atof(e);
        if (t >= 0.05 && t <= 1.0) ctx->pipeline_taper = t;
    }
    if (const char* e = std::getenv("MSFM_BYTE_DETECT")) ctx->byte_detect = e[0] != '0';
    if (const char* e = std::getenv("MSFM_UPLOAD_THREADS")) ctx->copy_helper = std::atoi(e) != 1;
    if (const char* e = std::getenv("MSFM_Q8_DIRECT")) ctx->q8_direct = e[0] == '2' ? 2 : (e[0] != '0');
    if (const char* e = std::getenv("MSFM_Q8")) ctx->q8_route = e[0] == '2' ? 2 : (e[0] != '0');
    if (const char* e = std::getenv("MSFM_IN_FLIGHT"))
        if (std::atoi(e) >= 1 && std::atoi(e) <= kInFlight) ctx->in_flight = std::atoi(e);
    if (const char* e = std::getenv("MSFM_PIPELINE"))
        if (std::atoi(e) > 0) ctx->pipeline = std::min(std::atoi(e), 64);
#ifdef MSFM_WG_TRACE   // (the diagnostic build of `make trace`)
    if (const char* e = std::getenv("MSFM_WG_TRACE")) ctx->wg_trace = e[0] != '0';
#endif
    if (const char* e = std::getenv("MSFM_SCRATCH_MIB"))
        if (std::atoll(e) > 0) ctx->scratch_bytes = std::atoll(e) * (1LL << 20);
    *out_ctx = ctx;
    return MSFM_OK;
    MSFM_API_END
}

static void destroy_streams(msfm_ctx* ctx) {
    for (Scratch& sc : ctx->sc) {
        if (sc.sweep1_done) (void)hipEventDestroy(sc.sweep1_done);
        if (sc.sweep2_done) (void)hipEventDestroy(sc.sweep2_done);
        sc.sweep2_done = nullptr;
        if (sc.stream) (void)hipStreamDestroy(sc.stream);
        sc.sweep1_done = nullptr;
        sc.stream = nullptr;
    }
}

void msfm_destroy(msfm_ctx* ctx) {
    if (!ctx) return;
    try {
    HostClock hc;   // MSFM_DEBUG_TIMING=1
    (void)hipSetDevice(ctx->device);
    for (Scratch& sc : ctx->sc)
        if (sc.stream) (void)hipStreamSynchronize(sc.stream);
    ctx->deferred.flush();
    ctx->tracks.release();
    ctx->store.release_all();
    ctx->inbox.release_all();
    hc.lap("destroy: store");
    for (Scratch& sc : ctx->sc) sc.release_all();
    hc.lap("destroy: scratch sets");
    DevBuf* bufs[] = {&ctx->d_jobs, &ctx->d_store_maxima, &ctx->d_zero_row, &ctx->ret_words, &ctx->ret_cn};
    for (DevBuf* b : bufs) b->release();
    for (OutSeg& s : ctx->out_segs) {
        s.qt.release();
        s.d.release();
    }
    ctx->res_qt.release();
    ctx->res_dist.release();
    ctx->up_ring.release();
    ctx->h_jobs.release();
    ctx->h_store_maxima.release();
    ctx->pinned_pool.release();   // (behind every buffer that holds a piece of it: the scratch sets' above)
    hc.lap("destroy: result lists, page-locked memory");
    for (hipEvent_t e : ctx->up_ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->jobs_ev) (void)hipEventDestroy(ctx->jobs_ev);
    delete_match_job(ctx->job);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    destroy_streams(ctx);
    hc.lap("destroy: events, streams");
    delete ctx;
    } catch (...) {   // (the C ABI never throws; nothing above is expected to)
    }
}

const char* msfm_last_error(const msfm_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int msfm_device_info(const msfm_ctx* ctx, char* name, int name_cap, int* cu_count, int* clock_mhz) {
    MSFM_API_BEGIN(nullptr)
    if (!ctx) return MSFM_E_INVALID;
    if (name && name_cap > 0) std::snprintf(name, (size_t)name_cap, "%s", ctx->dev_name);
    if (cu_count) *cu_count = ctx->cu_count;
    if (clock_mhz) *clock_mhz = ctx->clock_mhz;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_set_prefilter(msfm_ctx* ctx, int enable) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    ctx->prefilter = enable == 2 ? 2 : (enable ? 1 : 0);
    return MSFM_OK;
    MSFM_API_END
}

int msfm_set_limits(msfm_ctx* ctx, int max_pairs_per_batch, int64_t scratch_bytes) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    // (the pair index of a sub-batch is gridDim.y of several kernels: at most 65535)
    ctx->max_pairs_per_batch = max_pairs_per_batch > 0 ? std::min(max_pairs_per_batch, kMaxPairsPerBatchLimit) : kDefaultMaxPairsPerBatch;
    ctx->scratch_bytes = scratch_bytes > 0 ? scratch_bytes : 0;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_set_pipeline(msfm_ctx* ctx, int min_sub_batches) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    ctx->pipeline = min_sub_batches > 0 ? std::min(min_sub_batches, 64) : kDefaultPipeline;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_get_profile(const msfm_ctx* ctx, msfm_profile* out) {
    MSFM_API_BEGIN(nullptr)
    if (!ctx || !out) return MSFM_E_INVALID;
    *out = ctx->prof;
    return MSFM_OK;
    MSFM_API_END
}

// A matching entry point is returning rc: THE way out on failure.  An error return may leave launches of the failed batch in flight:
// the streams are drained before control goes back, so that the caller can free or reuse its buffers and a following call starts from
// idle streams; a series, open before the call or opened by it, is closed.
static int leave(msfm_ctx* ctx, int rc) {
    if (rc != MSFM_OK && ctx) {
        close_series(ctx);
        for (Scratch& sc : ctx->sc)
            if (sc.stream) (void)hipStreamSynchronize(sc.stream);
        ctx->cur = &ctx->sc[0];
    }
    return rc;
}

namespace {

// host state of one sub-batch in flight (parallel to ctx->sc[slot])
struct SubBatch {
    Batch b;
    int begin = 0, end = 0;
    size_t ev_base = 0;
    bool exact_launched = false;
    int begin_of_cost = -1;       // the pair index cost_begin belongs to (a re-built sub-batch keeps its start cost)
    long long cost_begin = 0;
    std::vector<int64_t> offsets; // streaming form: the completed sub-batch's CSR offsets (relative to the sub-batch) and
    std::vector<int32_t> sens;    //   order-certificate counts, until the caller asks for the next chunk
    std::vector<int32_t> sel;     //   and the model selection's records {model, nE, nH} per pair (msfm_fetch_model_selection)
    std::vector<msfm_two_view_record> tv;   //   and the two-view geometry's (msfm_fetch_two_view_geometry)
    std::vector<msfm_two_view_refinement> tvr;   //   and the two-view refinement's (msfm_fetch_two_view_refinements)
};

void add_profile(msfm_profile& to, const msfm_profile& d) {
    to.dist_kernel_ms += d.dist_kernel_ms;
    to.dist_kernel_launches += d.dist_kernel_launches;
    to.descriptor_pairs += d.descriptor_pairs;
    to.dist_algo_bytes += d.dist_algo_bytes;
    to.approx_kernel_ms += d.approx_kernel_ms;
    to.approx_kernel_launches += d.approx_kernel_launches;
    to.prefilter_pairs += d.prefilter_pairs;
    to.fallback_pairs += d.fallback_pairs;
    to.candidates += d.candidates;
    to.prefilter_descriptor_pairs += d.prefilter_descriptor_pairs;
    to.exact_descriptor_pairs += d.exact_descriptor_pairs;
    to.tie_rows += d.tie_rows;
    to.sweep2_ms += d.sweep2_ms;
    to.sweep2_launches += d.sweep2_launches;
    to.compacted_pairs += d.compacted_pairs;
    to.sweep2_descriptor_pairs += d.sweep2_descriptor_pairs;
    to.verify_ms += d.verify_ms;
    to.sub_batches += d.sub_batches;
    to.tie_queue_regrows += d.tie_queue_regrows;
    to.plan_regrows += d.plan_regrows;
    to.sweep1_i8_launches += d.sweep1_i8_launches;
    to.order_sensitive_rows += d.order_sensitive_rows;
    to.sweep1_q8_launches += d.sweep1_q8_launches;
    to.sweep1b_launches += d.sweep1b_launches;
    to.sweep1b_ms += d.sweep1b_ms;
    to.sweep1b_descriptor_pairs += d.sweep1b_descriptor_pairs;
    to.demoted_pairs += d.demoted_pairs;
    to.mixed_route_sub_batches += d.mixed_route_sub_batches;
    to.memory_shrinks += d.memory_shrinks;
}

int drain_streams(msfm_ctx* ctx) {
    for (Scratch& s : ctx->sc)
        if (s.stream) HIPCHK(ctx, hipStreamSynchronize(s.stream));
    return MSFM_OK;
}

}  // namespace

extern "C++" {   // (MatchJob has member templates)
#include "msfm_job.hip.h"
}

namespace {
// behind an exception caught at the C ABI (msfm_guard.h): the text for msfm_last_error, nothing left in flight, no series left open
void after_api_exception(msfm_ctx* ctx, int rc, const char* text) noexcept {
    if (!ctx) return;
    try {
        ctx->err = text ? text : "C++ exception";
    } catch (...) {
    }
    ctx->have_results = false;
    (void)leave(ctx, rc);
}
}  // namespace

// Any matching call ends a streaming series that was left open (msfm_match_pairs_begin without the msfm_match_pairs_next that returns
// n_pairs == 0): its sub-batches in flight are drained, the store is unlocked, a later msfm_match_pairs_next returns MSFM_E_STATE.
static int abandon_series(msfm_ctx* ctx) {
    if (!ctx->series_open) return MSFM_OK;
    close_series(ctx);
    return drain_streams(ctx);
}

// the verification parameters of a verified call: the reference's (FeatureUtils.cpp:196: FM_RANSAC, 3.0, 0.99; OpenCV's maxIters) unless
// the caller gives its own
static int verify_params(msfm_ctx* ctx, const msfm_verify_params* given, msfm_verify_params* v) {
    *v = msfm_verify_params{3.0, 0.99, 1000, 0x5eed5eedULL};
    if (given) *v = *given;
    if (!(v->threshold >= 0.0) || !(v->confidence > 0.0) || !(v->confidence < 1.0) || v->max_iters < 1 || v->max_iters > (1 << 16))
        return fail(ctx, MSFM_E_INVALID, "bad verification parameters");
    return MSFM_OK;
}

static int match_pairs_impl(msfm_ctx* ctx, const int32_t* pairs, int n_pairs, const msfm_match_params* params,
                            const msfm_verify_params* verify, int64_t* out_offsets) {
    if (!ctx) return MSFM_E_INVALID;
    if (n_pairs < 0 || (n_pairs > 0 && !pairs) || !out_offsets) return fail(ctx, MSFM_E_INVALID, "bad pair list");
    MatchJob& job = *ctx->job;
    int rc = abandon_series(ctx);   // a streaming series left open is abandoned: what it has in flight is drained first
    if (rc == MSFM_OK) rc = job.start(ctx, pairs, n_pairs, params, verify, false);
    if (rc != MSFM_OK) return rc;
    while (job.more()) {
        int slot = 0;
        rc = job.step(&slot);
        if (rc != MSFM_OK) return rc;
    }
    rc = job.finish();
    if (rc != MSFM_OK) return rc;
    std::memcpy(out_offsets, ctx->res_offsets.data(), ((size_t)n_pairs + 1) * sizeof(int64_t));
    ctx->have_results = true;   // what the blocking form hands out: set here and nowhere else
    ctx->sel_valid = job.select;
    ctx->tv_valid = job.pose;
    ctx->tvr_valid = job.refine;
    return MSFM_OK;
}

int msfm_match_pairs(msfm_ctx* ctx, const int32_t* pairs, int n_pairs, const msfm_match_params* params,
                     int64_t* out_offsets) {
    MSFM_API_BEGIN(ctx)
    return leave(ctx, match_pairs_impl(ctx, pairs, n_pairs, params, nullptr, out_offsets));
    MSFM_API_END
}

int msfm_match_pairs_verified(msfm_ctx* ctx, const int32_t* pairs, int n_pairs, const msfm_match_params* params,
                              const msfm_verify_params* verify, int64_t* out_offsets) {
    MSFM_API_BEGIN(ctx)
    msfm_verify_params v;
    const int rc = verify_params(ctx, verify, &v);
    if (rc != MSFM_OK) return rc;
    return leave(ctx, match_pairs_impl(ctx, pairs, n_pairs, params, &v, out_offsets));
    MSFM_API_END
}

int msfm_set_verification_model(msfm_ctx* ctx, int model, const msfm_camera* camera) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (ctx->series_open) return fail(ctx, MSFM_E_STATE, "a streaming series is open");
    if (ctx->two_view && model != MSFM_VERIFY_ESSENTIAL)
        return fail(ctx, MSFM_E_INVALID, "the two-view geometry is on and needs the essential-matrix model: switch it off first");
    if (model == MSFM_VERIFY_FUNDAMENTAL) {
        ctx->verify_model = model;
        return MSFM_OK;
    }
    if (model == MSFM_VERIFY_HOMOGRAPHY) {
        if (camera) return fail(ctx, MSFM_E_INVALID, "the homography model takes no camera");
        ctx->verify_model = model;
        return MSFM_OK;
    }
    if (model != MSFM_VERIFY_ESSENTIAL) return fail(ctx, MSFM_E_INVALID, "unknown verification model");
    if (!camera) return fail(ctx, MSFM_E_INVALID, "the essential-matrix model needs a camera");
    const msfm_camera c = *camera;
    const double all[8] = {c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2};
    for (double v : all)
        if (!std::isfinite(v)) return fail(ctx, MSFM_E_INVALID, "camera parameters must be finite");
    if (!(c.fx > 0.0) || !(c.fy > 0.0)) return fail(ctx, MSFM_E_INVALID, "fx and fy must be positive");
    ctx->verify_model = model;
    ctx->camera = msfm_emat::Camera{c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2};
    return MSFM_OK;
    MSFM_API_END
}

int msfm_set_model_selection(msfm_ctx* ctx, int enable, double h_ratio) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (ctx->series_open) return fail(ctx, MSFM_E_STATE, "a streaming series is open");
    if (enable != 0 && enable != 1) return fail(ctx, MSFM_E_INVALID, "enable must be 0 or 1");
    if (!std::isfinite(h_ratio) || !(h_ratio > 0.0)) return fail(ctx, MSFM_E_INVALID, "h_ratio must be finite and > 0");
    ctx->model_select = enable != 0;
    ctx->h_ratio = h_ratio;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_fetch_model_selection(msfm_ctx* ctx, int32_t* out_model, int32_t* out_n_epipolar, int32_t* out_n_homography) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (!ctx->sel_valid) return fail(ctx, MSFM_E_STATE, "the last verified call / chunk ran without the model selection");
    const size_t n = ctx->sel_records.size() / 3;
    for (size_t p = 0; p < n; ++p) {
        if (out_model) out_model[p] = ctx->sel_records[3 * p];
        if (out_n_epipolar) out_n_epipolar[p] = ctx->sel_records[3 * p + 1];
        if (out_n_homography) out_n_homography[p] = ctx->sel_records[3 * p + 2];
    }
    return MSFM_OK;
    MSFM_API_END
}

int msfm_set_two_view_geometry(msfm_ctx* ctx, int enable, const msfm_two_view_params* params) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (ctx->series_open) return fail(ctx, MSFM_E_STATE, "a streaming series is open");
    if (enable != 0 && enable != 1) return fail(ctx, MSFM_E_INVALID, "enable must be 0 or 1");
    msfm_two_view_params p = {100, 0, 2.0, 4.0};   // Initializer::Parameters (include/Reconstruction/Initializer.h:19-30)
    if (params) p = *params;
    if (p.min_num_inliers < 0 || !std::isfinite(p.tri_max_error) || p.tri_max_error < 0.0 || !std::isfinite(p.tri_min_angle) ||
        p.tri_min_angle < 0.0)
        return fail(ctx, MSFM_E_INVALID, "two-view parameters must be finite and not negative");
    if (enable && ctx->verify_model != MSFM_VERIFY_ESSENTIAL)
        return fail(ctx, MSFM_E_INVALID, "the two-view geometry needs the essential-matrix model (msfm_set_verification_model)");
    if (!enable && ctx->tv_refine)
        return fail(ctx, MSFM_E_INVALID, "the two-view refinement is on and needs the two-view geometry: switch it off first");
    p.reserved = 0;
    ctx->two_view = enable != 0;
    ctx->tv_params = p;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_fetch_two_view_geometry(msfm_ctx* ctx, msfm_two_view_record* out) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (!ctx->tv_valid) return fail(ctx, MSFM_E_STATE, "the last verified call / chunk ran without the two-view geometry");
    if (out && !ctx->tv_records.empty()) std::memcpy(out, ctx->tv_records.data(), ctx->tv_records.size() * sizeof(msfm_two_view_record));
    return MSFM_OK;
    MSFM_API_END
}

int msfm_set_two_view_refinement(msfm_ctx* ctx, int enable, const msfm_two_view_refine_params* params) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (ctx->series_open) return fail(ctx, MSFM_E_STATE, "a streaming series is open");
    if (enable != 0 && enable != 1) return fail(ctx, MSFM_E_INVALID, "enable must be 0 or 1");
    msfm_two_view_refine_params p = msfm_tvr::default_params();
    if (params) p = *params;
    if (p.max_iters < 1 || p.min_matches < 5 || !std::isfinite(p.step_tol) || p.step_tol < 0.0)
        return fail(ctx, MSFM_E_INVALID, "two-view refinement: max_iters >= 1, min_matches >= 5, step_tol finite and not negative");
    if (enable && !ctx->two_view)
        return fail(ctx, MSFM_E_INVALID, "the two-view refinement needs the two-view geometry (msfm_set_two_view_geometry)");
    ctx->tv_refine = enable != 0;
    ctx->tvr_params = p;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_fetch_two_view_refinements(msfm_ctx* ctx, msfm_two_view_refinement* out) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (!ctx->tvr_valid) return fail(ctx, MSFM_E_STATE, "the last verified call / chunk ran without the two-view refinement");
    if (out && !ctx->tvr_records.empty())
        std::memcpy(out, ctx->tvr_records.data(), ctx->tvr_records.size() * sizeof(msfm_two_view_refinement));
    return MSFM_OK;
    MSFM_API_END
}

int msfm_get_verification_stats(const msfm_ctx* ctx, int64_t* hypotheses_solved, int* rounds) {
    MSFM_API_BEGIN(nullptr)
    if (!ctx) return MSFM_E_INVALID;
    if (hypotheses_solved) *hypotheses_solved = ctx->staged_solved;
    if (rounds) *rounds = ctx->staged_rounds;
    return MSFM_OK;
    MSFM_API_END
}

static MatchJob* new_match_job() { return new (std::nothrow) MatchJob(); }
static void delete_match_job(MatchJob* j) { delete j; }

// ---- streaming form: one device sub-batch per call, nothing accumulates (include/msfm_match.h) -------------------------------------
static int begin_impl(msfm_ctx* ctx, const int32_t* pairs, int n_pairs, const msfm_match_params* params, int geometric_verification,
                      const msfm_verify_params* verify) {
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return fail(ctx, MSFM_E_INVALID, "bad pair list");
    msfm_verify_params v;
    int rc = geometric_verification ? verify_params(ctx, verify, &v) : MSFM_OK;
    if (rc == MSFM_OK) rc = abandon_series(ctx);
    if (rc != MSFM_OK) return rc;
    MatchJob& job = *ctx->job;
    job.pairs_own.assign(pairs, pairs + 2 * (size_t)n_pairs);
    return job.start(ctx, job.pairs_own.data(), n_pairs, params, geometric_verification ? &v : nullptr, true);
}

int msfm_match_pairs_begin(msfm_ctx* ctx, const int32_t* pairs, int n_pairs, const msfm_match_params* params, int geometric_verification,
                           const msfm_verify_params* verify) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return leave(ctx, begin_impl(ctx, pairs, n_pairs, params, geometric_verification, verify));
    MSFM_API_END
}

static int next_impl(msfm_ctx* ctx, msfm_chunk* out) {
    // (one thread may drive contexts on several devices in turn: step() allocates scratch and asks for the free memory)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->series_open) return fail(ctx, MSFM_E_STATE, "msfm_match_pairs_next without msfm_match_pairs_begin");
    MatchJob& job = *ctx->job;
    *out = msfm_chunk{};
    ctx->sel_valid = ctx->tv_valid = ctx->tvr_valid = false;   // (the chunk before is gone; a step that fails hands out nothing)
    const SubBatch* w = nullptr;   // the chunk; none: the series is complete, n_pairs == 0
    int slot = 0;
    if (job.more()) {
        const int rc = job.step(&slot);
        if (rc != MSFM_OK) return rc;
        w = &job.sb[slot];
    }
    // what the streaming form hands out, set here and nowhere else: the chunk's records, none behind the last chunk
    ctx->sel_records = w ? w->sel : std::vector<int32_t>();
    ctx->sel_valid = job.select;
    ctx->tv_records = w ? w->tv : std::vector<msfm_two_view_record>();
    ctx->tv_valid = job.pose;
    ctx->tvr_records = w ? w->tvr : std::vector<msfm_two_view_refinement>();
    ctx->tvr_valid = job.refine;
    if (!w) return job.finish();
    const Scratch& sc = ctx->sc[slot];
    out->first_pair = w->begin;
    out->n_pairs = w->end - w->begin;
    out->offsets = w->offsets.data();
    out->count = w->offsets.empty() ? 0 : w->offsets.back();
    out->qt = sc.h_sub_qt.as<int32_t>();
    out->dist = sc.h_sub_d.as<float>();
    out->d_qt = sc.d_sub_qt.as<int32_t>();
    out->d_dist = sc.d_sub_d.as<float>();
    out->sensitive_rows = w->sens.data();
    return MSFM_OK;
}

int msfm_match_pairs_next(msfm_ctx* ctx, msfm_chunk* out) {
    MSFM_API_BEGIN(ctx)
    if (!ctx || !out) return MSFM_E_INVALID;
    return leave(ctx, next_impl(ctx, out));
    MSFM_API_END
}

int msfm_match_pairs_end(msfm_ctx* ctx) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return abandon_series(ctx);
    MSFM_API_END
}

int msfm_fetch_matches(msfm_ctx* ctx, int32_t* out_qt, float* out_dist) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (!ctx->have_results) return fail(ctx, MSFM_E_STATE, "msfm_fetch_matches without a completed msfm_match_pairs");
    if (out_qt && ctx->res_count) std::memcpy(out_qt, ctx->res_qt.base, ctx->res_count * 8);
    if (out_dist && ctx->res_count) std::memcpy(out_dist, ctx->res_dist.base, ctx->res_count * 4);
    return MSFM_OK;
    MSFM_API_END
}

int msfm_fetch_matches_device(msfm_ctx* ctx, int32_t* d_out_qt, float* d_out_dist) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (!ctx->have_results) return fail(ctx, MSFM_E_STATE, "msfm_fetch_matches_device without a completed msfm_match_pairs");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    for (size_t k = 0; k < ctx->out_used; ++k) {
        const OutSeg& s = ctx->out_segs[k];
        if (!s.count) continue;
        if (d_out_qt) HIPCHK(ctx, hipMemcpyAsync(d_out_qt + 2 * s.first, s.qt.p, s.count * 8, hipMemcpyDeviceToDevice, SC.stream));
        if (d_out_dist) HIPCHK(ctx, hipMemcpyAsync(d_out_dist + s.first, s.d.p, s.count * 4, hipMemcpyDeviceToDevice, SC.stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(SC.stream));
    return MSFM_OK;
    MSFM_API_END
}

int msfm_memory_info(msfm_ctx* ctx, msfm_memory* out) {
    MSFM_API_BEGIN(ctx)
    if (!ctx || !out) return MSFM_E_INVALID;
    *out = msfm_memory{};
    HIPCHK(ctx, hipSetDevice(ctx->device));
    size_t free_b = 0, total_b = 0;
    HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
    out->device_free = (int64_t)free_b;
    out->device_total = (int64_t)total_b;
    out->store = (int64_t)ctx->store.bytes();
    out->inbox = (int64_t)ctx->inbox.bytes();
    // (buffers that are pieces of the context's pool count once, with the pool)
    auto own = [](const PinnedBuf& h) { return h.pooled ? (size_t)0 : h.cap; };
    size_t pinned = ctx->pinned_pool.cap + ctx->up_ring.cap + own(ctx->h_jobs) + own(ctx->h_store_maxima) + ctx->res_qt.pinned + ctx->res_dist.pinned;
    long long scratch = 0;
    for (Scratch& sc : ctx->sc) {
        scratch += sc.device_bytes();
        for (const PinnedBuf& h : sc.h_up) pinned += own(h);
        pinned += own(sc.h_summary) + own(sc.h_tail) + own(sc.h_tk_pairs) + sc.h_sub_qt.cap + sc.h_sub_d.cap + sc.h_tv.cap;
    }
    out->scratch = scratch;
    for (const OutSeg& s : ctx->out_segs) out->results_device += (int64_t)(s.qt.cap + s.d.cap);
    out->page_locked_host = (int64_t)pinned;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_read_device(msfm_ctx* ctx, void* host_dst, const void* device_src, int64_t bytes) {
    MSFM_API_BEGIN(ctx)
    if (!ctx || bytes < 0 || (bytes > 0 && (!host_dst || !device_src))) return MSFM_E_INVALID;
    if (bytes == 0) return MSFM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpy(host_dst, device_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return MSFM_OK;
    MSFM_API_END
}

int msfm_fetch_order_certificate(msfm_ctx* ctx, int32_t* out_sensitive_rows) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (!ctx->have_results) return fail(ctx, MSFM_E_STATE, "msfm_fetch_order_certificate without a completed msfm_match_pairs");
    if (out_sensitive_rows && !ctx->res_sens.empty()) std::memcpy(out_sensitive_rows, ctx->res_sens.data(), ctx->res_sens.size() * 4);
    return MSFM_OK;
    MSFM_API_END
}

int msfm_view_matches(msfm_ctx* ctx, const int32_t** out_qt, const float** out_dist, int64_t* out_count) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (!ctx->have_results) return fail(ctx, MSFM_E_STATE, "msfm_view_matches without a completed msfm_match_pairs");
    if (out_qt) *out_qt = ctx->res_qt.as<int32_t>();
    if (out_dist) *out_dist = ctx->res_dist.as<float>();
    if (out_count) *out_count = (int64_t)ctx->res_count;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_match_pair(msfm_ctx* ctx, int id1, int id2, float ratio, int cross_check, double max_distance,
                    int32_t* out_qt, float* out_dist, int* out_count) {
    MSFM_API_BEGIN(ctx)
    if (!ctx || !out_count) return MSFM_E_INVALID;
    const int32_t pr[2] = {id1, id2};
    msfm_match_params prm = {ratio, cross_check, max_distance};
    int64_t offs[2] = {0, 0};
    ctx->tracks.suppress = true;   // (the operator-level call takes no part in a track session)
    int rc = msfm_match_pairs(ctx, pr, 1, &prm, offs);
    ctx->tracks.suppress = false;
    if (rc != MSFM_OK) return rc;
    *out_count = (int)offs[1];
    return msfm_fetch_matches(ctx, out_qt, out_dist);
    MSFM_API_END
}

static int knn2_pair_impl(msfm_ctx* ctx, int id1, int id2, int32_t* fwd_idx0, float* fwd_d0, float* fwd_d1,
                          int32_t* rev_idx0, float* rev_d0, float* rev_d1);

int msfm_knn2_pair(msfm_ctx* ctx, int id1, int id2, int32_t* fwd_idx0, float* fwd_d0, float* fwd_d1,
                   int32_t* rev_idx0, float* rev_d0, float* rev_d1) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return leave(ctx, knn2_pair_impl(ctx, id1, id2, fwd_idx0, fwd_d0, fwd_d1, rev_idx0, rev_d0, rev_d1));
    MSFM_API_END
}

static int knn2_pair_impl(msfm_ctx* ctx, int id1, int id2, int32_t* fwd_idx0, float* fwd_d0, float* fwd_d1,
                          int32_t* rev_idx0, float* rev_d0, float* rev_d1) {
    // a streaming series left open is abandoned (include/msfm_match.h): what it has in flight is drained first -- this call runs on
    // scratch set 0 and would otherwise overwrite the tail words of a sub-batch the series still has to complete
    int rc = abandon_series(ctx);
    if (rc != MSFM_OK) return rc;
    ctx->prof = msfm_profile{};
    rc = call_prologue(ctx);
    if (rc != MSFM_OK) return rc;
    Batch b;
    PairDesc pd;
    PfPair pp;
    rc = fill_pair(ctx, id1, id2, pd, pp);
    if (rc != MSFM_OK) return rc;
    b.pairs.push_back(pd);
    b.pf.push_back(pp);
    b.id1.push_back(id1);
    b.id2.push_back(id2);
    bool exact_launched = false;
    int regrows = 0, fallbacks = 0;
    std::vector<char> force_exact(1, 0);
    // the knnMatch twin: nothing is pruned (the float forms), every row keeps its neighbours, no CSR
    auto attempt = [&](bool* again) {
        b.n_items = 0;
        b.rp_elems = b.cp_elems = b.kf_elems = b.kr_elems = b.out_elems = b.cand_elems = 0;
        b.desc_pairs = b.algo_bytes = 0;
        b.pairs[0].path = b.pf[0].use = force_exact[0] ? 0 : pp.use;
        int r = prepare_batch_images(ctx, b, PruneParams{0, 0.f, 0.f});
        if (r != MSFM_OK) return r;
        SC.prof = msfm_profile{};   // only the attempt that is kept counts
        r = run_knn(ctx, b, 2, &exact_launched, PruneParams{0, 0.f, 0.f}, true, false);
        if (r != MSFM_OK) return r;
        SC.d_offsets.release();   // (the export kernel skips absent segments)
        SC.d_sens.release();
        r = queue_tail_copies(ctx, 1);
        if (r != MSFM_OK) return r;
        HIPCHK(ctx, hipStreamSynchronize(SC.stream));
        bool retry = false, retry_pf = false;
        r = check_fix_overflow(ctx, &retry);
        if (r == MSFM_OK) r = finish_prefilter(ctx, b, force_exact, &retry_pf);
        if (r != MSFM_OK) return r;
        if (retry) ++regrows;
        if (retry_pf) fallbacks += SC.prof.fallback_pairs;
        *again = retry || retry_pf;
        return (int)MSFM_OK;
    };
    bool again = false;
    rc = attempt(&again);
    if (rc == MSFM_OK && again) rc = rerun_alone(ctx, attempt);
    if (rc != MSFM_OK) return rc;
    rc = accumulate_kernel_time(ctx, 2, exact_launched);
    if (rc != MSFM_OK) return rc;
    ctx->prof = SC.prof;
    ctx->prof.tie_queue_regrows = regrows;
    ctx->prof.fallback_pairs = fallbacks;
    ctx->prof.sub_batches = 1;
    ctx->prof.descriptor_pairs += b.desc_pairs;
    ctx->prof.dist_algo_bytes += b.algo_bytes;
    const PairDesc& q = b.pairs[0];
    const int n1 = ctx->images[id1].n, n2 = ctx->images[id2].n;
    if (!q.valid) {
        // an empty side: no neighbours
        for (int i = 0; i < n1; ++i) {
            if (fwd_idx0) fwd_idx0[i] = -1;
            if (fwd_d0) fwd_d0[i] = 3.402823466e+38f;
            if (fwd_d1) fwd_d1[i] = 3.402823466e+38f;
        }
        for (int i = 0; i < n2; ++i) {
            if (rev_idx0) rev_idx0[i] = -1;
            if (rev_d0) rev_d0[i] = 3.402823466e+38f;
            if (rev_d1) rev_d1[i] = 3.402823466e+38f;
        }
        return MSFM_OK;
    }
    struct Cp { void* dst; const DevBuf* src; long long off; int n; };
    const Cp cps[6] = {{fwd_idx0, &SC.d_k_i0, q.kf_off, n1}, {fwd_d0, &SC.d_k_d0, q.kf_off, n1},
                       {fwd_d1, &SC.d_k_d1, q.kf_off, n1},   {rev_idx0, &SC.d_k_i0, q.kr_off, n2},
                       {rev_d0, &SC.d_k_d0, q.kr_off, n2},   {rev_d1, &SC.d_k_d1, q.kr_off, n2}};
    for (const Cp& c : cps)
        if (c.dst && c.n > 0)
            HIPCHK(ctx, hipMemcpyAsync(c.dst, c.src->as<char>() + c.off * 4, (size_t)c.n * 4, hipMemcpyDeviceToHost, SC.stream));
    HIPCHK(ctx, hipStreamSynchronize(SC.stream));
    return MSFM_OK;
}

// ---- feature tracks (msfm_tracks.hip.h) ---------------------------------------------------------------------------------------------

int msfm_tracks_begin(msfm_ctx* ctx, const int32_t* ids, int n, const msfm_track_params* params) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return tracks_begin_impl(ctx, ids, n, params);
    MSFM_API_END
}

int msfm_tracks_add(msfm_ctx* ctx, const int32_t* pairs, int n_pairs, const int64_t* offsets, const int32_t* qt) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return tracks_add_impl(ctx, pairs, n_pairs, offsets, qt);
    MSFM_API_END
}

int msfm_tracks_export_forest(msfm_ctx* ctx, int32_t* parent) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return tracks_export_impl(ctx, parent);
    MSFM_API_END
}

int msfm_tracks_import_forest(msfm_ctx* ctx, const int32_t* parent) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return tracks_import_impl(ctx, parent);
    MSFM_API_END
}

int msfm_tracks_finish(msfm_ctx* ctx, const msfm_track_filter* filter, msfm_track_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return tracks_finish_impl(ctx, filter, stats);
    MSFM_API_END
}

int msfm_fetch_tracks(msfm_ctx* ctx, int64_t* offsets, int32_t* image_ids, int32_t* point_idx, uint8_t* consistent) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return tracks_fetch_impl(ctx, offsets, image_ids, point_idx, consistent);
    MSFM_API_END
}

int msfm_fetch_track_ids(msfm_ctx* ctx, int image_id, int32_t* out) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return tracks_fetch_ids_impl(ctx, image_id, out);
    MSFM_API_END
}

int msfm_tracks_end(msfm_ctx* ctx) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return tracks_end_impl(ctx);
    MSFM_API_END
}

// ---- track triangulation (msfm_triangulate.hip.h) -----------------------------------------------------------------------------------

int msfm_triangulate_tracks(msfm_ctx* ctx, const msfm_camera* camera, const int32_t* image_ids, const msfm_pose_rt* poses, int n_poses,
                            const msfm_triangulation_params* params, msfm_triangulation_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return triangulate_impl(ctx, camera, image_ids, poses, n_poses, params, stats);
    MSFM_API_END
}

int msfm_fetch_points3d(msfm_ctx* ctx, msfm_point3d* out_points, double* out_residuals) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return fetch_points3d_impl(ctx, out_points, out_residuals);
    MSFM_API_END
}

// ---- robust track triangulation (msfm_triangulate_robust.hip.h) ---------------------------------------------------------------------

int msfm_triangulate_tracks_robust(msfm_ctx* ctx, const msfm_camera* camera, const int32_t* image_ids, const msfm_pose_rt* poses,
                                   int n_poses, const msfm_robust_triangulation_params* params, msfm_triangulation_stats* stats,
                                   msfm_robust_stats* robust_stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return triangulate_robust_impl(ctx, camera, image_ids, poses, n_poses, params, stats, robust_stats);
    MSFM_API_END
}

int msfm_fetch_point_inliers(msfm_ctx* ctx, uint8_t* out) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return fetch_point_inliers_impl(ctx, out);
    MSFM_API_END
}

// ---- point refinement (msfm_refine.hip.h) ---------------------------------------------------------------------------------------------

int msfm_refine_points(msfm_ctx* ctx, const msfm_refine_params* params, msfm_refine_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return refine_impl(ctx, params, stats);
    MSFM_API_END
}

// ---- pose refinement (msfm_refine_poses.hip.h) -----------------------------------------------------------------------------------------

int msfm_refine_poses(msfm_ctx* ctx, const msfm_pose_refine_params* params, const int32_t* fixed_image_ids, int n_fixed,
                      msfm_pose_refine_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return refine_poses_impl(ctx, params, fixed_image_ids, n_fixed, stats);
    MSFM_API_END
}

int msfm_fetch_poses(msfm_ctx* ctx, int32_t* out_ids, msfm_pose_rt* out_poses, int* n) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return fetch_poses_impl(ctx, out_ids, out_poses, n);
    MSFM_API_END
}

int msfm_fetch_pose_refinements(msfm_ctx* ctx, msfm_pose_refinement* out) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return fetch_pose_refinements_impl(ctx, out);
    MSFM_API_END
}

// ---- camera refinement (msfm_refine_camera.hip.h) ----------------------------------------------------------------------------------------

int msfm_refine_camera(msfm_ctx* ctx, const msfm_camera_refine_params* params, msfm_camera_refine_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return refine_camera_impl(ctx, params, stats);
    MSFM_API_END
}

int msfm_fetch_camera(msfm_ctx* ctx, msfm_camera* out) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return fetch_camera_impl(ctx, out);
    MSFM_API_END
}

// ---- map extension (msfm_extend.hip.h) -------------------------------------------------------------------------------------------------

int msfm_extend_points(msfm_ctx* ctx, const int32_t* image_ids, const msfm_pose_rt* poses, int n_poses, const msfm_extend_params* params,
                       msfm_extend_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return extend_impl(ctx, image_ids, poses, n_poses, params, stats);
    MSFM_API_END
}

// ---- map filtering (msfm_filter.hip.h) -------------------------------------------------------------------------------------------------

int msfm_filter_points(msfm_ctx* ctx, const msfm_filter_params* params, const int32_t* image_ids, int n_images, msfm_filter_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return filter_impl(ctx, params, image_ids, n_images, stats);
    MSFM_API_END
}

// ---- map completion (msfm_complete.hip.h) -----------------------------------------------------------------------------------------------

int msfm_complete_points(msfm_ctx* ctx, const msfm_complete_params* params, const int32_t* image_ids, int n_images,
                         msfm_complete_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return complete_impl(ctx, params, image_ids, n_images, stats);
    MSFM_API_END
}

// ---- map visibility (msfm_visibility.hip.h) ------------------------------------------------------------------------------------------------

int msfm_map_visibility(msfm_ctx* ctx, const msfm_visibility_params* params, const int32_t* query_ids, int n_query,
                        msfm_image_visibility* out_images, uint32_t* out_covisible, msfm_visibility_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return visibility_impl(ctx, params, query_ids, n_query, out_images, out_covisible, stats);
    MSFM_API_END
}

// ---- map alignment (msfm_align.hip.h) ----------------------------------------------------------------------------------------------------

int msfm_estimate_alignment(msfm_ctx* ctx, const int32_t* image_ids, const double* positions, int n, const msfm_alignment_params* params,
                            msfm_alignment* out, msfm_alignment_residual* out_per_prior) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return estimate_alignment_impl(ctx, image_ids, positions, n, params, out, out_per_prior);
    MSFM_API_END
}

int msfm_transform_map(msfm_ctx* ctx, const msfm_similarity* similarity, msfm_transform_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return transform_map_impl(ctx, similarity, stats);
    MSFM_API_END
}

// ---- image registration (msfm_register.hip.h) ---------------------------------------------------------------------------------------

int msfm_register_images(msfm_ctx* ctx, const msfm_camera* camera, const int32_t* image_ids, int n_images,
                         const msfm_register_params* params, msfm_register_stats* stats) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return register_impl(ctx, camera, image_ids, n_images, params, stats);
    MSFM_API_END
}

int msfm_fetch_registrations(msfm_ctx* ctx, msfm_registration* out, int64_t* out_offsets, int32_t* out_track_ids, uint8_t* out_inlier,
                             double* out_residuals) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return fetch_registrations_impl(ctx, out, out_offsets, out_track_ids, out_inlier, out_residuals);
    MSFM_API_END
}

// ---- host-only helpers --------------------------------------------------------------------

int msfm_topscale_select(const float* kpts, int n, int k, int32_t* out_idx, int* out_count) {
    MSFM_API_BEGIN(nullptr)
    if (n < 0 || k < 0 || !out_idx || !out_count || (n > 0 && !kpts)) return MSFM_E_INVALID;
    if (k > n) {  // "if(num_features > kpts.size()) top_scale_descriptors = descriptors"
        for (int i = 0; i < n; ++i) out_idx[i] = i;
        *out_count = n;
        return MSFM_OK;
    }
    std::vector<int32_t> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    // documented tie rule: size descending, then index ascending (the reference's
    // std::partial_sort leaves the order of equal sizes unspecified)
    std::partial_sort(order.begin(), order.begin() + k, order.end(), [kpts](int32_t a, int32_t b) {
        const float sa = kpts[(size_t)a * 4 + 2], sb = kpts[(size_t)b * 4 + 2];
        if (sa != sb) return sa > sb;
        return a < b;
    });
    for (int i = 0; i < k; ++i) out_idx[i] = order[(size_t)i];
    *out_count = k;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_swap_image_pair(int id1, int id2) { return id1 > id2 ? 1 : 0; }

int msfm_pair_id(int id1, int id2, int32_t* out_pair_id) {
    MSFM_API_BEGIN(nullptr)
    if (!out_pair_id || id1 < 0 || id2 < 0 || id1 >= MSFM_MAX_IMAGES || id2 >= MSFM_MAX_IMAGES) return MSFM_E_INVALID;
    *out_pair_id = msfm_swap_image_pair(id1, id2) ? MSFM_MAX_IMAGES * id2 + id1 : MSFM_MAX_IMAGES * id1 + id2;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_pair_from_id(int32_t pair_id, int* out_id1, int* out_id2) {
    MSFM_API_BEGIN(nullptr)
    if (!out_id1 || !out_id2 || pair_id < 0) return MSFM_E_INVALID;
    *out_id2 = pair_id % MSFM_MAX_IMAGES;
    *out_id1 = (pair_id - *out_id2) / MSFM_MAX_IMAGES;
    return MSFM_OK;
    MSFM_API_END
}

}  // extern "C"

// ---- vocabulary retrieval (matching mode 2) ---------------------------------------------------------------------------------------
#include "msfm_retrieval_host.hip.h"

extern "C" {

int msfm_train_vocabulary(msfm_ctx* ctx, const int32_t* ids, int n, const msfm_retrieval_params* params, uint8_t* out_words,
                          int* out_num_words) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return ret_drained(ctx, train_impl(ctx, ids, n, params, out_words, out_num_words));
    MSFM_API_END
}

int msfm_set_vocabulary(msfm_ctx* ctx, const uint8_t* words, int n_words) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    if (!words || n_words < 1 || n_words > kRetMaxWords) return fail(ctx, MSFM_E_INVALID, "msfm_set_vocabulary: bad vocabulary");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = ret_alloc_vocab(ctx, n_words);
    if (rc != MSFM_OK) return ret_drained(ctx, rc);
    std::vector<unsigned char> q((size_t)n_words * kDim);
    for (size_t k = 0; k < q.size(); ++k) q[k] = words[k] ^ 0x80;   // c' = c - 128
    HIPCHK(ctx, hipStreamSynchronize(store_stream(ctx)));
    HIPCHK(ctx, hipMemcpy(ctx->ret_words.p, q.data(), q.size(), hipMemcpyHostToDevice));
    ctx->ret_v = n_words;
    rc = ret_norms(ctx);
    if (rc != MSFM_OK) {
        ctx->ret_v = 0;
        return ret_drained(ctx, rc);
    }
    HIPCHK(ctx, hipStreamSynchronize(store_stream(ctx)));
    ctx->ret_prof.num_words = n_words;
    return MSFM_OK;
    MSFM_API_END
}

int msfm_image_words(msfm_ctx* ctx, int image_id, int32_t* out_word) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return ret_drained(ctx, image_words_impl(ctx, image_id, out_word));
    MSFM_API_END
}

int msfm_retrieve_pairs(msfm_ctx* ctx, const int32_t* ids, int n, int num_nearest, int32_t* out_pairs, float* out_scores, int* out_n_pairs,
                        float* out_score_matrix) {
    MSFM_API_BEGIN(ctx)
    if (!ctx) return MSFM_E_INVALID;
    return ret_drained(ctx, retrieve_impl(ctx, ids, n, num_nearest, out_pairs, out_scores, out_n_pairs, out_score_matrix));
    MSFM_API_END
}

int msfm_get_retrieval_profile(const msfm_ctx* ctx, msfm_retrieval_profile* out) {
    MSFM_API_BEGIN(nullptr)
    if (!ctx || !out) return MSFM_E_INVALID;
    *out = ctx->ret_prof;
    return MSFM_OK;
    MSFM_API_END
}

}  // extern "C"
