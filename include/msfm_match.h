/*
 * msfm_match.h -- C ABI of the MI355X (gfx950) ComputeMatches hot path.
 *
 * Drop-in boundary for nebula-beta/MonocularSfM's descriptor matcher: every entry point
 * replaces one C++ interface of the reference (cited per function, paths relative to the
 * reference checkout).  The reference has no FFI layer of its own; its seams are the static
 * FeatureUtils operators (include/Feature/FeatureUtils.h:94-108) called from
 * src/Feature/FeatureMatching.cpp:36-49 and :163-170, and the Database blobs on either side.
 *
 * Conventions
 *   - plain C types only; every call returns an int status (MSFM_OK == 0), never throws
 *     (every entry point runs behind one exception barrier, csrc/msfm_guard.h: an allocation
 *     failure inside the library comes back as MSFM_E_DEVICE, the context stays usable),
 *     never exits.  msfm_last_error() gives the text of the last failure on a context.
 *   - the caller owns all host buffers; the library owns all device memory.
 *   - descriptors are row-major, contiguous, 128 columns (cv::Mat CV_32F n x 128 as read by
 *     Database::ReadDescriptors, src/Database/Database.cpp:510-523), or uint8 with the same shape.
 *   - a context is bound to one GPU and is not thread-safe; distinct contexts may be driven
 *     from distinct threads (one per GPU).
 *   - there is NO CPU fallback: without a usable gfx950 device msfm_create() fails.
 */
#ifndef MSFM_MATCH_H
#define MSFM_MATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSFM_DIM 128
#define MSFM_MAX_IMAGES 10000 /* kMaxNumImages, src/Database/Database.cpp:6 */

enum {
    MSFM_OK = 0,
    MSFM_E_INVALID = 1,   /* bad argument */
    MSFM_E_DEVICE = 2,    /* HIP error (text in msfm_last_error) */
    MSFM_E_NOIMAGE = 3,   /* image id not uploaded */
    MSFM_E_CAPACITY = 4,  /* caller buffer too small */
    MSFM_E_STATE = 5      /* call sequence error (e.g. fetch without a prior match) */
};

enum { MSFM_DTYPE_F32 = 0, MSFM_DTYPE_U8 = 1 };

/* fp32 accumulation order of S(q,t) = sum_c (a_c-b_c)^2, i.e. which build of
 * cv::hal::normL2Sqr_ (called through BFMatcher::knnMatch at src/Feature/FeatureUtils.cpp:149)
 * the bits are identical to.  Integer-valued descriptors give identical bits under all. */
enum {
    MSFM_ORDER_SSE4X4 = 0,   /* OpenCV 4.x SSE baseline: 16 lane partials, mul and add rounded apart */
    MSFM_ORDER_AVX2_FMA = 1, /* OpenCV 4.x AVX2+FMA3 baseline: 32 lane partials, fused */
    MSFM_ORDER_AVX512_FMA = 3 /* AVX-512+FMA3 build of the same loop: 64 lane partials, fused (a third named order: the
                                 cross-check of the order-invariance certificate, msfm_fetch_order_certificate) */
};

typedef struct msfm_ctx msfm_ctx;

/* Matching parameters = the FeatureMatcher constructor arguments that reach the operators
 * (include/Feature/FeatureMatching.h:28-32): distance_ratio (passed on as float),
 * cross_check, max_distance (double). */
typedef struct msfm_match_params {
    float ratio;          /* default 0.8f */
    int cross_check;      /* default 1    */
    double max_distance;  /* default 0.7  */
} msfm_match_params;

/* Kernel-side timing of the last msfm_match_pairs / msfm_match_pair / msfm_knn2_pair call,
 * measured with HIP events on the library's own stream. */
typedef struct msfm_profile {
    double dist_kernel_ms;     /* sum over launches of the distance/top-2 kernel */
    int dist_kernel_launches;
    double total_device_ms;    /* first launch -> last result copy of the call */
    int64_t descriptor_pairs;  /* sum n1*n2 over the pairs of the call */
    int64_t dist_algo_bytes;   /* compulsory HBM bytes of the distance kernel */
    /* MFMA prefilter path (two sweep_kernel launches per batch + exact re-check of the candidates) */
    double approx_kernel_ms;   /* sum over batches of sweep 1 (sweep_kernel<1> / sweep_i8_kernel<1>: every descriptor pair once; the field keeps its round-1 name) */
    int approx_kernel_launches;
    int prefilter_pairs;       /* pairs answered through the prefilter path */
    int fallback_pairs;        /* pairs whose candidate list overflowed -> brute-force exact kernel */
    int64_t candidates;        /* exact distances evaluated for prefiltered pairs */
    int64_t prefilter_descriptor_pairs;
    int64_t exact_descriptor_pairs; /* descriptor pairs that went through the brute-force kernel */
    int64_t tie_rows;          /* rows re-scanned by the sqrt-space tie fix-up */
    double sweep2_ms;          /* sum over batches of sweep 2 (sweep_kernel<2> dense / <3> compacted live rows, sweep_i8_kernel<3>) */
    int sweep2_launches;
    int compacted_pairs;       /* pairs whose sweep 2 ran on the compacted live rows only */
    int64_t sweep2_descriptor_pairs; /* descriptor pairs sweep 2 actually multiplied (padded rows included) */
    double verify_ms;          /* geometric verification kernels (msfm_match_pairs_verified) */
    int sub_batches;           /* device sub-batches the call was cut into (msfm_set_limits) */
    int tie_queue_regrows;     /* sub-batches re-run because the sqrt-space tie queue had to grow */
    int plan_regrows;          /* sub-batches re-run because the device-side sweep-2 plan outgrew its predicted buffers */
    int sweep1_i8_launches;     /* sweep-1 launches on the integer matrix cores (byte stores, msfm_sweep_i8.hip.h) */
    /* route Q: float images with byte twins (all values in [0, 1]) -- sweep 1 on the twins, on the integer matrix cores */
    int sweep1_q8_launches;     /* sweep-1 launches on byte TWINS of float images (counted in sweep1_i8_launches too) */
    int sweep1b_launches;       /* fp16 sweep 1' launches (coarse twins only -- values beyond 0.625, or MSFM_Q8_DIRECT=0: the S~ top-2 of the
                                   rows the twins' sweep left alive, sweep_kernel<4>); 0 when the twins give sweep 2 its thresholds directly */
    double sweep1b_ms;
    int64_t sweep1b_descriptor_pairs; /* descriptor pairs sweep 1' multiplied (padded compacted rows included) */
    int64_t order_sensitive_rows; /* rows / columns of the call WITHOUT an order-invariance certificate (see
                                     msfm_fetch_order_certificate); 0 => the stored (queryIdx, trainIdx) rows are the same
                                     under any conforming fp32 evaluation order of hal::normL2Sqr_ */
    int demoted_pairs;            /* pairs of two byte images (or of two images with byte twins) whose first sweep ran on the fp16 cores
                                     all the same, because their SUB-BATCH also held a pair that could not take the integer route (a
                                     mixed store: byte stores and coarse twins choose the route per sub-batch; fine twins do not, see
                                     mixed_route_sub_batches).  Same results, ~1.6 x the sweep time; 0 on a homogeneous store */
    int mixed_route_sub_batches;  /* sub-batches that ran TWO first sweeps: the integer one on the pairs whose images both have fine byte
                                     twins, the fp16 one on the rest (an image with a value beyond [0, 1] among twinned ones) -- the twins'
                                     pairs are not demoted then.  Byte stores and coarse twins still choose one route per sub-batch */
    int memory_shrinks;           /* times the call found the device OUT OF MEMORY while sizing a sub-batch's scratch (another tenant of the GPU,
                                     several contexts on one device: the budget of msfm_set_limits is derived from the free memory once per
                                     state of the store), gave every idle buffer back, halved the scratch share of a sub-batch and cut again from
                                     the same pair.  Same results, more sub-batches; 0 normally.  After four of them the call fails with MSFM_E_DEVICE */
} msfm_profile;

/* ---- context ------------------------------------------------------------------------- */
/* msfm_create: ~85 ms in a fresh process, 52 of them the HIP runtime's own start-up (its first call), the rest one stream (a hardware
 * queue), the kernels' attributes and a first allocation; the streams of the second and third scratch set are created by the first call
 * that keeps more than one sub-batch in flight.  MSFM_DEBUG_TIMING=1 in the environment: the library's host-side clocks on stderr
 * (context creation and destruction, store build, every sub-batch's phases, allocations per call). */
int msfm_create(int device_ordinal, msfm_ctx** out_ctx);
void msfm_destroy(msfm_ctx* ctx);
const char* msfm_last_error(const msfm_ctx* ctx);
/* device name + CU count of the context's GPU (for bench reports); name_cap >= 64 */
int msfm_device_info(const msfm_ctx* ctx, char* name, int name_cap, int* cu_count, int* clock_mhz);
int msfm_set_accum_order(msfm_ctx* ctx, int order);
/* 1 (default): MFMA prefilter + exact re-check where safe -- byte images (MSFM_DTYPE_U8 uploads, and MSFM_DTYPE_F32
 * uploads whose every value is an integer in [0, 255]: raw OpenCV SIFT stored as CV_32F, recognised on the device at
 * upload; MSFM_BYTE_DETECT=0 at msfm_create: off) on the integer matrix cores (v_mfma_i32_32x32x32_i8); float images whose values all lie in [0, 1] (RootSIFT) get a byte twin at upload and
 * their FIRST sweep on the integer cores too; fine twins (the store's values stay below 0.625) hand the second sweep its thresholds
 * directly, coarse ones are refined by an fp16 sweep of the ~6 % of rows left alive first (route Q; MSFM_Q8=0 in the environment
 * at msfm_create: off, MSFM_Q8_DIRECT=0: always refine); everything else on the fp16 cores; 2: fp16 matrix cores for every
 * image; 0: always the brute-force exact kernel.  Results are bit-identical in all.
 * Env: MSFM_PREFILTER=0|1|2. */
int msfm_set_prefilter(msfm_ctx* ctx, int enable);
int msfm_get_profile(const msfm_ctx* ctx, msfm_profile* out);
/* msfm_match_pairs cuts a call into device sub-batches of at most `max_pairs_per_batch` image pairs (default 16384) and of
 * at most `scratch_bytes` of device scratch for ALL sub-batches in flight TOGETHER (three scratch sets share it, a third each;
 * what a pair needs: msfm_pair_scratch_bytes in csrc/msfm_hostutil.h -- on the matrix-core route ~2 MB per pair of 8192-row
 * images).  scratch_bytes <= 0 (default): 64 GiB, but never more than a quarter of what the device has free when the call starts
 * (hipMemGetInfo + what the sets already hold); an explicit value is honoured up to half of that (the per-pair figure is what a call is CUT by, not a cap: buffers that turn out too small are re-grown and the sub-batch re-run).  The device is asked once per state of the store, not per call.  The call's result
 * lists (12 bytes per match, device + page-locked host) and the descriptor store are NOT part of this budget.  Also
 * MSFM_MAX_PAIRS_PER_BATCH and MSFM_SCRATCH_MIB in the environment at msfm_create.  Results do not depend on the cut (tests force
 * small limits to cross it).  The reference's counterpart is the 100-pair flush of BruteFeatureMatcher::RunMatching
 * (src/Feature/FeatureMatching.cpp:118-139, max_pairs_size_). */
int msfm_set_limits(msfm_ctx* ctx, int max_pairs_per_batch, int64_t scratch_bytes);
/* A call of enough work (>= 1.5e10 descriptor pairs per part) is cut into at least `min_sub_batches` sub-batches, launched round-robin
 * on three streams / scratch sets: the bandwidth-bound tail of one (thresholds, sweep-2 plan, exact re-check, epilogue, copy-out)
 * runs while the sweeps of the next ones own the matrix cores.  Default 2 equal parts (round 3: 6 parts shrinking to 0.3 of the
 * average; with round 4's smaller tails a further cut costs more than it hides); 1 = one sub-batch where memory allows (no overlap);
 * <= 0 restores the default.  Env: MSFM_PIPELINE, MSFM_PIPELINE_TAPER (size of the last part relative to the average, default 1),
 * MSFM_IN_FLIGHT.  Results do not depend on any of it. */
int msfm_set_pipeline(msfm_ctx* ctx, int min_sub_batches);

/* ---- descriptor store -------------------------------------------------------------------
 * Replaces the per-pair Database::ReadDescriptors calls of MatchImagePairs
 * (src/Feature/FeatureMatching.cpp:32-33, "TODO: cache"): every image is uploaded once and
 * stays resident in HBM.  ids are Database image ids, 0 <= id < MSFM_MAX_IMAGES.
 * msfm_upload_image COPIES the rows (the caller's buffer is free when it returns) and returns without building anything: the
 * images of all uploads since the last use are built together -- classification (byte store? values in [0, 1]?), ONE device
 * allocation, table-driven layout kernels -- by the next call that needs them (any matching call, msfm_subset_image of a
 * pending source) or by msfm_finalize_store.  A device error of that build (out of memory) is therefore reported by THAT call.
 * Resident per row: 184 B for a byte image (the 176-byte operand row of the integer matrix cores + norms; the fp32 / fp16 forms
 * are derived on the device the first time a route needs them: a pair with a float image, msfm_knn2_pair, ratio > 0.95,
 * msfm_set_prefilter 0 / 2), 788 B for a float image (+ 184 B with a byte twin); + 512 B per row of 128-row panels for
 * images that take the brute-force route.  csrc/msfm_store.hip.h has the table. */
int msfm_upload_image(msfm_ctx* ctx, int image_id, const void* desc, int n, int dim, int dtype);
/* A new store entry from rows of a resident one, entirely on the device: the sub-matrix
 * FeatureUtils::ExtractTopScaleDescriptors builds (src/Feature/FeatureUtils.cpp:84-95, rows picked by
 * msfm_topscale_select) without reading the descriptors from the database a second time
 * (BruteFeatureMatcher::GetTopScaleDescriptors, FeatureMatching.cpp:181-196, does re-read them).
 * rows: `count` indices into src, any order, repeats allowed; dst != src (usually MSFM_MAX_IMAGES + id). */
int msfm_subset_image(msfm_ctx* ctx, int src_image_id, int dst_image_id, const int32_t* rows, int count);
int msfm_image_rows(const msfm_ctx* ctx, int image_id, int* out_n);
int msfm_clear_images(msfm_ctx* ctx);
/* Build everything uploaded so far now (otherwise the first matching call does it): the end of a bulk load, e.g. of
 * FeatureMatcher::PreloadAllImages' one SELECT sweep over the descriptors table (host/FeatureMatching.cpp). */
int msfm_finalize_store(msfm_ctx* ctx);
/* Device bytes the store holds (its chunks, incl. forms derived on demand and keypoints), descriptor rows resident, images still
 * waiting for msfm_finalize_store.  Any pointer may be NULL. */
int msfm_store_info(const msfm_ctx* ctx, int64_t* out_device_bytes, int64_t* out_rows, int64_t* out_pending_images);

/* ---- one pair ---------------------------------------------------------------------------
 * Twin of FeatureUtils::ComputeCrossMatches / ComputeMatches (src/Feature/FeatureUtils.cpp:
 * 141-174) followed by FilterMatchesByDistance (:208-218), i.e. lines 36-49 of
 * FeatureMatching.cpp.  query = id1, train = id2.  out_qt receives (queryIdx, trainIdx) int32
 * pairs in ascending queryIdx (capacity: rows(id1) pairs); out_dist (nullable) the DMatch
 * distances.  The reference indexes the 2nd neighbour unconditionally (FeatureUtils.cpp:152), so a
 * direction whose train set has < 2 rows is undefined there; here it yields no matches, and a
 * cross-checked pair with such a direction yields none at all.  Empty sides => no matches. */
int msfm_match_pair(msfm_ctx* ctx, int id1, int id2, float ratio, int cross_check,
                    double max_distance, int32_t* out_qt, float* out_dist, int* out_count);

/* ---- batch of pairs ---------------------------------------------------------------------
 * Twin of the loop body of FeatureMatcher::MatchImagePairs (FeatureMatching.cpp:14-49) over
 * independent pairs; results keep the input order.  pairs = P x 2 int32 (id1, id2).
 * out_offsets (P+1 int64) receives the CSR offsets of each pair's match list; the lists
 * themselves stay on the context until msfm_fetch_matches copies them out
 * (out_qt: 2*out_offsets[P] int32, out_dist nullable: out_offsets[P] float). */
int msfm_match_pairs(msfm_ctx* ctx, const int32_t* pairs, int n_pairs,
                     const msfm_match_params* params, int64_t* out_offsets);
int msfm_fetch_matches(msfm_ctx* ctx, int32_t* out_qt, float* out_dist);
/* Order-invariance certificate of the last msfm_match_pairs / _verified call: per pair the number of query rows (and,
 * with cross_check, train rows) for which a decision the reference makes -- which element is the first neighbour,
 * d0 < ratio * d1, d0 <= max_distance -- has a margin below the worst-case fp32 reassociation bound of a 128-term sum
 * of squares (relative 1e-5 on a distance, derivation in csrc/msfm_kernels.hip.h).  The reference delegates S(q,t) to an
 * unpinned OpenCV (cv::BFMatcher::knnMatch, src/Feature/FeatureUtils.cpp:146-149) whose accumulation order depends on the
 * build; a pair with 0 sensitive rows has the same (queryIdx, trainIdx) list under ANY such build.  Pairs of byte images
 * are exact integers under every order (always 0).  out_sensitive_rows: n_pairs int32.
 * The TIE RULE, the other thing SURVEY App. C restates from memory (batchDistance keeps the lower train index among equal
 * distances): with ratio <= 1 the match LISTS do not depend on it either.  A row whose two smallest distances are equal
 * (d0 == d1, which is when the rule decides the first neighbour) fails `d0 < ratio * d1` under either index order, in both
 * directions, so its index never reaches a list; a tie for the SECOND place leaves the value d1 unchanged.  So a job with 0
 * order-sensitive rows and ratio <= 1 stores the same rows under any conforming accumulation order AND either tie order
 * (tests/test_gpu_certificate.py::test_match_lists_do_not_depend_on_the_tie_rule flips the rule in the integer reference on
 * the planted-tie fixture; only the knnMatch-level API msfm_knn2_pair and ratio > 1 see the rule, and implement the lower
 * index: tie_fixup_kernel). */
int msfm_fetch_order_certificate(msfm_ctx* ctx, int32_t* out_sensitive_rows);
/* The same lists without the copy: pointers into the context's page-locked result buffers
 * (2 * count int32, count float), valid until the next matching call on this context or msfm_destroy. */
int msfm_view_matches(msfm_ctx* ctx, const int32_t** out_qt, const float** out_dist, int64_t* out_count);
/* The same lists copied device-to-device into CALLER-OWNED DEVICE memory on the context's GPU (2 * count int32 /
 * count float; either pointer may be NULL): the multi-GPU exchange step sends them over RCCL straight from HBM
 * instead of staging them through the host.  Complete when the call returns. */
int msfm_fetch_matches_device(msfm_ctx* ctx, int32_t* d_out_qt, float* d_out_dist);

/* ---- batch of pairs, STREAMING form (bounded memory) ----------------------------------------
 * msfm_match_pairs keeps the whole call's lists resident (12 bytes per match in HBM and the same page-locked): BASELINE's
 * largest config produces 6.9e9 matches.  The reference streams by construction -- one transaction per <= 100 pairs,
 * BruteFeatureMatcher::RunMatching (src/Feature/FeatureMatching.cpp:13, 70-72, 118-139).  Same here:
 *   msfm_match_pairs_begin   takes the pair list (copied) and the parameters (geometric_verification != 0: the lists are verified
 *                            on the device as in msfm_match_pairs_verified, `verify` NULL = the reference's constants);
 *   msfm_match_pairs_next    completes ONE device sub-batch -- the next `n_pairs` pairs of the list, in order -- and hands out its
 *                            lists: CSR offsets relative to the chunk, (q, t) rows and distances in page-locked host memory AND in
 *                            device memory (for an RCCL send straight from HBM), the order-certificate counts.  The pointers are valid
 *                            until the next msfm_match_pairs_next / any other matching call on the context.  n_pairs == 0: done.
 * Between two calls the library keeps up to three sub-batches in flight exactly as msfm_match_pairs does; what is resident at any time
 * is the scratch of those (msfm_set_limits) plus their lists.  msfm_get_profile accumulates over the series.  While a series is open
 * (until the call that returns n_pairs == 0) the store must not change: uploads, msfm_subset_image and msfm_clear_images return
 * MSFM_E_STATE; another matching call abandons the series (what it has in flight is drained first). */
typedef struct msfm_chunk {
    int first_pair;                 /* index into the pair list given to msfm_match_pairs_begin */
    int n_pairs;                    /* 0: the series is complete */
    int64_t count;                  /* matches of the chunk = offsets[n_pairs] */
    const int64_t* offsets;         /* n_pairs + 1 */
    const int32_t* qt;              /* host (page-locked): 2 * count */
    const float* dist;              /* host: count */
    const int32_t* d_qt;            /* device: 2 * count */
    const float* d_dist;            /* device: count */
    const int32_t* sensitive_rows;  /* n_pairs (msfm_fetch_order_certificate) */
} msfm_chunk;
struct msfm_verify_params;
int msfm_match_pairs_begin(msfm_ctx* ctx, const int32_t* pairs, int n_pairs, const msfm_match_params* params,
                           int geometric_verification, const struct msfm_verify_params* verify);
int msfm_match_pairs_next(msfm_ctx* ctx, msfm_chunk* out);
/* Ends a series before its last chunk (a consumer that stops early, an error in the consumer's own loop): drains what the series has
 * in flight, unlocks the store; a following msfm_match_pairs_next returns MSFM_E_STATE.  No series open: MSFM_OK, nothing happens.
 * (The reference's counterpart is leaving the pair loop of FeatureMatcher::MatchImagePairs, src/Feature/FeatureMatching.cpp:14-72.) */
int msfm_match_pairs_end(msfm_ctx* ctx);
/* What the context holds right now, in bytes: the descriptor store, uploads waiting in the inbox, the scratch of the sub-batches in
 * flight (grow-only: its high-water mark), the call-wide result lists on the device (msfm_match_pairs; the streaming form has none),
 * page-locked host memory (result lists, staging); and the device's free / total memory (hipMemGetInfo). */
typedef struct msfm_memory {
    int64_t device_free, device_total;
    int64_t store, inbox, scratch, results_device;
    int64_t page_locked_host;
} msfm_memory;
int msfm_memory_info(msfm_ctx* ctx, msfm_memory* out);
/* Plain device -> host copy through the library's own runtime (a caller without a HIP runtime of its own -- a ctypes binding --
 * reading msfm_chunk::d_qt / d_dist or a buffer msfm_fetch_matches_device filled). */
int msfm_read_device(msfm_ctx* ctx, void* host_dst, const void* device_src, int64_t bytes);

/* ---- batch of pairs with the geometric verification hand-off -------------------------------
 * Lines 36-60 of FeatureMatching.cpp in one call: matching as above, then FeatureUtils::FilterMatches
 * (src/Feature/FeatureUtils.cpp:176-206: GetAlignedPointsFromMatches + cv::findFundamentalMat(FM_RANSAC,
 * 3.0, 0.99) + keep the inliers) for every pair, on the device, before the lists are copied out.
 * Needs the keypoint coordinates of every image of the batch: msfm_upload_keypoints after msfm_upload_image
 * (kpts: n rows of `stride_floats` floats, x and y first -- the Database's keypoint blob has stride 4:
 * x, y, size, angle; n >= descriptor rows).  NULL `verify` = the reference's constants (3.0 px, 0.99, OpenCV's
 * 1000-iteration cap).  OpenCV's RANSAC (RNG, 7-point solver) cannot be reproduced without OpenCV: this entry
 * point is OUTSIDE the bit-parity claim; it is bit-identical to the host twin
 * monocularsfm_amd/host/GeometricVerification.cpp (shared arithmetic, csrc/msfm_fmat.h).
 * Cases as in findFundamentalMat: no matches -> none; < 7 -> none; exactly 7 -> all; otherwise RANSAC with
 * the adaptive iteration bound, and a consensus set below 8 keeps none.
 * THE COORDINATES ARE NOT VALIDATED: msfm_upload_keypoints checks the row count and nothing else (the reference does not validate
 * them either, and dropping rows would change the row indices).  A NaN, an infinity or a huge coordinate reaches the verification, the
 * two-view records, the triangulations, the registration, the refinements and the map extension, and there it makes ITS OWN
 * OBSERVATION FAIL every test it takes part in -- it is never a kept match of a sample-based model's consensus, never an inlier of a
 * point or of a pose, no loop's bound depends on it, and the tests (tests/test_nonfinite_reference.py, tests/test_gpu_nonfinite.py) hold the calls to
 * treating it byte for byte as they treat the same coordinate at 1e6 px.  (A plain,
 * non-robust triangulation whose DLT takes such an observation in gives ATTEMPTED without ERROR_OK -- without a point for a
 * non-finite coordinate -- as for any gross outlier.)  The only doubles of an output that can be NaN are that observation's own
 * error slots (msfm_fetch_points3d's and msfm_fetch_registrations' residuals), and a NaN there is always 0x7ff8000000000000
 * (csrc/msfm_pose.h, "THE NaN RULE").  The denormals and -0.0 are the pixel coordinate 0. */
typedef struct msfm_verify_params {
    double threshold;            /* pixels (reference: 3.0) */
    double confidence;           /* (reference: 0.99) */
    int max_iters;               /* hypotheses per pair at most (OpenCV default: 1000) */
    unsigned long long seed;     /* sampling stream, the same for every pair */
} msfm_verify_params;
int msfm_upload_keypoints(msfm_ctx* ctx, int image_id, const float* kpts, int n, int stride_floats);

/* ---- verification model --------------------------------------------------------------------
 * MSFM_VERIFY_FUNDAMENTAL (the default) is FeatureUtils::FilterMatches as above.  MSFM_VERIFY_ESSENTIAL verifies with the camera
 * instead (the reference's TODO at src/Feature/FeatureMatching.cpp:59; its reconstruction runs cv::findEssentialMat on the same
 * camera): 5-point essential-matrix RANSAC on normalised, undistorted coordinates, Sampson error <= (threshold / ((fx + fy) / 2))^2,
 * the same adaptive stopping rule with sample size 5, no refit; < 5 matches or a consensus below 5 keeps none.  Bit-identical to the
 * host twin EssentialRansacMask (csrc/msfm_emat.h).  One camera for every image; per context; honoured by msfm_match_pairs_verified
 * and msfm_match_pairs_begin(.., geometric_verification = 1, ..).  MSFM_E_INVALID: unknown model, NULL camera for model 1,
 * fx / fy <= 0 or any parameter non-finite; MSFM_E_STATE while a streaming series is open.
 * MSFM_VERIFY_HOMOGRAPHY verifies planar scenes and rotation-only views, where F and E are degenerate (the reference runs
 * cv::findHomography beside findFundamentalMat on its initial pairs, src/Reconstruction/Initializer.cpp:38-66): 4-point homography
 * RANSAC on the keypoints' pixel coordinates (OpenCV's subset check, Hartley-normalised DLT), one-sided reprojection error
 * |x2 - H x1|^2 <= threshold^2, the same adaptive stopping rule with sample size 4, no refit; < 4 matches or a consensus below 4
 * keeps none.  Bit-identical to the host twin HomographyRansacMask (csrc/msfm_hmat.h).  It takes no camera: a non-NULL camera is
 * MSFM_E_INVALID.
 * msfm_get_verification_stats: hypotheses solved and rounds run (the largest over the pairs; kVeRound = 32 hypotheses per round
 * under model 1, kVhRound = 64 under model 2) by the last verified call / series (0 under model 0). */
#define MSFM_VERIFY_FUNDAMENTAL 0
#define MSFM_VERIFY_ESSENTIAL 1
#define MSFM_VERIFY_HOMOGRAPHY 2
typedef struct msfm_camera {
    double fx, fy, cx, cy, k1, k2, p1, p2;
} msfm_camera;
int msfm_set_verification_model(msfm_ctx* ctx, int model, const msfm_camera* camera);
int msfm_get_verification_stats(const msfm_ctx* ctx, int64_t* hypotheses_solved, int* rounds);

/* ---- two-view model selection -----------------------------------------------------------------
 * Off by default.  When on and the verification model is MSFM_VERIFY_FUNDAMENTAL or MSFM_VERIFY_ESSENTIAL, every verified pair runs
 * two RANSACs on its matches: that epipolar model, exactly as above, and the homography, exactly as MSFM_VERIFY_HOMOGRAPHY.  With
 * nE and nH the lengths of the two lists, the pair keeps the homography's list iff nE > 0 and (double)nH >= h_ratio * (double)nE
 * (one rounded product), else the epipolar one: the choice of the reference's Initializer, F when nH / nF < 0.7
 * (src/Reconstruction/Initializer.cpp:38-66).  So every pair's list is bit for bit the model 0 / 1 list or the model 2 list of the
 * same call parameters.  Under MSFM_VERIFY_HOMOGRAPHY the selection has no effect.  msfm_get_verification_stats then sums the
 * hypotheses of the staged models that ran (H, and E under model 1) and reports the larger rounds count.
 * msfm_set_model_selection: enable 0 / 1, h_ratio finite and > 0 (the reference: 0.7), else MSFM_E_INVALID; MSFM_E_STATE while a
 * streaming series is open.  Per context.
 * msfm_fetch_model_selection: per pair of the last msfm_match_pairs_verified call, or of the chunk the last msfm_match_pairs_next
 * returned (verified streaming form): the model whose list was kept (MSFM_VERIFY_FUNDAMENTAL / _ESSENTIAL / _HOMOGRAPHY), nE, nH.
 * Any pointer may be NULL.  MSFM_E_STATE if that call / chunk ran without the selection. */
int msfm_set_model_selection(msfm_ctx* ctx, int enable, double h_ratio);
int msfm_fetch_model_selection(msfm_ctx* ctx, int32_t* out_model, int32_t* out_n_epipolar, int32_t* out_n_homography);

/* ---- two-view geometry --------------------------------------------------------------------------
 * Off by default; MSFM_VERIFY_ESSENTIAL only.  When on, every verified pair also gets a record of what the reference's
 * Initializer::RecoverPoseFromFundanmental computes after its model choice (src/Reconstruction/Initializer.cpp:300-420): the
 * winning E of the pair's RANSAC is decomposed, the four-fold ambiguity resolved by cheirality over the pair's kept matches
 * (the nE E-inliers, in list order), each kept match triangulated by the reference's DLT under the winner, and the reference's
 * statistics and its test for an initial pair reduced from them.  The arithmetic is csrc/msfm_pose.h, bit-identical to the host
 * twin TwoViewGeometry.  The match lists, the statistics and the selection records do not change.
 *   R, t              x2 ~ R x1 + t in normalised camera coordinates, R row-major and proper, |t| = 1
 *   n_kept            nE
 *   n_positive_depth  kept matches in front of both cameras under (R, t)
 *   n_triangulated    of those, the ones with a reprojection error < tri_max_error: the mean of the two views' Euclidean errors
 *                     against the undistorted observations, in pixels through (fx + fy) / 2
 *   median_tri_angle  over all nE kept matches (the mean of the two middle ones for an even nE), degrees
 *   mean_tri_angle, mean_residual   over the n_triangulated matches (0 when there are none)
 *   is_initial_candidate   n_triangulated >= min_num_inliers && median_tri_angle >= tri_min_angle && mean_tri_angle >= tri_min_angle
 *                          && mean_residual <= tri_max_error
 * valid = 0 and everything else 0: the pair has fewer than 5 staged matches or its RANSAC has no winner (a consensus below 5), no candidate puts a match in front of both cameras, E has
 * fewer than two non-zero singular values, or the model selection kept the homography's list for the pair (the pose of a
 * homography is not computed).
 * msfm_set_two_view_geometry: enable 0 / 1; params NULL = the reference's defaults {100, 2.0 px, 4.0 degrees}.  MSFM_E_INVALID for a
 * negative or non-finite parameter and when enabled under another model than MSFM_VERIFY_ESSENTIAL; MSFM_E_STATE while a streaming
 * series is open.  msfm_set_verification_model away from MSFM_VERIFY_ESSENTIAL while this is on is MSFM_E_INVALID: switch it off first.
 * msfm_fetch_two_view_geometry: one record per pair of the last msfm_match_pairs_verified call, or of the chunk the last
 * msfm_match_pairs_next returned (verified streaming form); out may be NULL.  MSFM_E_STATE if that call / chunk ran without it. */
typedef struct msfm_two_view_params {
    int32_t min_num_inliers;     /* Initializer::Parameters::rel_pose_min_num_inlier: 100 */
    int32_t reserved;
    double tri_max_error;        /* init_tri_max_error: 2.0 pixels */
    double tri_min_angle;        /* init_tri_min_angle: 4.0 degrees */
} msfm_two_view_params;
typedef struct msfm_two_view_record {   /* 144 bytes, no implicit padding */
    int32_t valid;
    int32_t reserved;
    double R[9];
    double t[3];
    int32_t n_kept;
    int32_t n_positive_depth;
    int32_t n_triangulated;
    int32_t is_initial_candidate;
    double median_tri_angle;
    double mean_tri_angle;
    double mean_residual;
} msfm_two_view_record;
int msfm_set_two_view_geometry(msfm_ctx* ctx, int enable, const msfm_two_view_params* params);
int msfm_fetch_two_view_geometry(msfm_ctx* ctx, msfm_two_view_record* out);

/* ---- two-view pose refinement ---------------------------------------------------------------------
 * Off by default; needs the two-view geometry.  When on, the pose of every valid record with n_kept >= min_matches is polished over
 * ALL the pair's kept matches: Levenberg-Marquardt on the Sampson error (pixels through (fx + fy) / 2) in five unknowns, three of
 * the rotation (R <- C(a) R, Cayley) and two of the translation direction (|t| = 1 is kept), one 5 x 5 system per pair.  The
 * record's statistics are then computed again under the refined pose, and the refined record replaces the record iff a step was
 * accepted and neither n_positive_depth nor n_triangulated is lower than before; otherwise not one byte of the record changes.
 * n_kept, the match lists, the statistics and the selection records never change.  The arithmetic is csrc/msfm_pose_refine.h,
 * bit-identical to the host twin RefineTwoView.  The layout of msfm_two_view_record does not change: what the refinement did is in
 * a record of its own per pair, all zero for a pair that is not eligible (an invalid record, or n_kept < min_matches):
 *   status       MSFM_TVR_ELIGIBLE | MSFM_TVR_STEP_ACCEPTED (the loop accepted a step) | MSFM_TVR_REFINED (the record was replaced)
 *   stop         why the loop ended: 1 the step fell below step_tol, 2 max_iters steps were evaluated, 3 the damping passed its ceiling
 *   steps, accepted   evaluated steps, and those of them that lowered the cost
 *   n_positive_depth_before, n_triangulated_before   the counts of the record that went in
 *   cost_before, cost_after   the sum of squared Sampson residuals in px^2 at the record's pose and at the pose that stands
 *                             (cost_after = cost_before when the record was not replaced)
 * msfm_set_two_view_refinement: enable 0 / 1; params NULL = {10, 15, 1e-6}.  MSFM_E_INVALID for max_iters < 1, min_matches < 5, a
 * negative or non-finite step_tol, and when enabled while the two-view geometry is off; MSFM_E_STATE while a streaming series is
 * open.  msfm_set_two_view_geometry(0) while this is on is MSFM_E_INVALID: switch this off first.
 * msfm_fetch_two_view_refinements: one record per pair of the last msfm_match_pairs_verified call, or of the chunk the last
 * msfm_match_pairs_next returned; out may be NULL.  MSFM_E_STATE if that call / chunk ran without the refinement. */
#define MSFM_TVR_ELIGIBLE 1
#define MSFM_TVR_STEP_ACCEPTED 2
#define MSFM_TVR_REFINED 4
typedef struct msfm_two_view_refine_params {   /* 16 bytes */
    int32_t max_iters;           /* evaluated steps per pair at most: 10 */
    int32_t min_matches;         /* kept matches a pair needs: 15 */
    double step_tol;             /* the loop ends when |delta|^2 <= step_tol^2: 1e-6 */
} msfm_two_view_refine_params;
typedef struct msfm_two_view_refinement {   /* 40 bytes, no implicit padding */
    int32_t status;
    int32_t stop;
    int32_t steps, accepted;
    int32_t n_positive_depth_before, n_triangulated_before;
    double cost_before, cost_after;
} msfm_two_view_refinement;
int msfm_set_two_view_refinement(msfm_ctx* ctx, int enable, const msfm_two_view_refine_params* params);
int msfm_fetch_two_view_refinements(msfm_ctx* ctx, msfm_two_view_refinement* out);
int msfm_match_pairs_verified(msfm_ctx* ctx, const int32_t* pairs, int n_pairs,
                              const msfm_match_params* params, const msfm_verify_params* verify,
                              int64_t* out_offsets);

/* ---- knnMatch(k=2) twin (parity/debug) ----------------------------------------------------
 * Both directions of cv::BFMatcher(NORM_L2).knnMatch(.., 2) for one pair
 * (call site src/Feature/FeatureUtils.cpp:146-149), from ONE pass over the distance matrix.
 * fwd_* have rows(id1) entries (train index into id2), rev_* rows(id2) entries.
 * idx = -1 and d = FLT_MAX where fewer than 1 / 2 neighbours exist.  Any pointer may be NULL. */
int msfm_knn2_pair(msfm_ctx* ctx, int id1, int id2,
                   int32_t* fwd_idx0, float* fwd_d0, float* fwd_d1,
                   int32_t* rev_idx0, float* rev_d0, float* rev_d1);

/* ---- vocabulary retrieval: the pairs of matching mode 2 -------------------------------------
 * The reference's configuration reserves SIFTmatch.match_type 2 for "vocabulary tree match" (not implemented there).  Here it is a FLAT
 * visual vocabulary: every row's word is found by exhaustive search on the integer matrix cores, so every row gets its EXACT nearest
 * word (a tree would only approximate it).  Pairs are the images that a tf-idf comparison of their word histograms says overlap.
 * Everything up to the scores is integer arithmetic (a numpy reference reproduces it bit for bit: tests/retrieval_ref.py).
 *   quantised row q (128 x u8), per image: an image whose values are all integers in 0..255 (u8 or f32 uploads) uses q = x; an image
 *     whose values all lie in [0, 1] (RootSIFT, L2- or L1-root) uses q = (u8) rintf(x * 255.0f) (fp32 multiply, round half to even);
 *     any other image fails the call with MSFM_E_INVALID (msfm_last_error names it).  (The store's byte twins of float images use a
 *     store-wide level instead of 255: a different quantisation, not used here.)
 *   nearest word of a row: argmin_w sum (q - c_w)^2, exact in int32; the lower w wins a tie.  With q' = q - 128, c' = c - 128 this is
 *     argmin_w |c'_w|^2 - 2 q'.c'_w: one v_mfma_i32_32x32x32_i8 dot product and a constant per word.
 *   training sample: the call's images by ascending id, rows concatenated, R rows; s = max(1, R / M); the rows at 0, s, 2s, ... (at most
 *     M of them, Ms in all).  V' = min(V, max(1, Ms / 8)) words; word k starts as sample row (k Ms) / V' (64-bit integers).
 *   k-means: at most T Lloyd iterations on the sample, integer sums and counts; a word with cnt > 0 rows becomes
 *     c = floor((2 sum + cnt) / (2 cnt)) per dimension, a word without rows keeps its centroid; an iteration that changes no centroid ends
 *     the training early (the result is the same).
 *   scores: c_iw = rows of image i with word w, n_w = images of the call containing w, idf_w = ln(N / n_w), v_iw = c_iw idf_w,
 *     s_ij = v_i.v_j / (|v_i| |v_j|), 0 for a zero norm -- that is the fp64 definition.  The device evaluates a_iw = fl32(v_iw / |v_i|)
 *     (idf and |v_i| in fp64) and s_ij = one fp32 fmaf chain over w ascending: the same bits on every call and in any id order,
 *     s_ij == s_ji bit for bit, and |s_dev - s| <= (m + 4) 2^-23 with m = min(nnz(v_i), nnz(v_j)).
 *   selection: image i takes the first K images j != i with s_ij > 0, by device score, highest first, the lower id on equal scores; the
 *     pairs are the union of (max(i, j), min(i, j)) -- brute mode's orientation --, by first id, then second id, ascending.
 * Errors: no vocabulary, or a streaming series open: MSFM_E_STATE; an id that is not resident, twice in the list, an unsupported image,
 * n > MSFM_MAX_IMAGES, K outside 1..1024: MSFM_E_INVALID.  The context stays usable after any of them; a pending store build is done
 * first.  Only the vocabulary stays resident (V' x 144 B); the scratch of a call (words of every row, the n x V' histograms, the n x n
 * scores) is freed when it returns. */
typedef struct msfm_retrieval_params {
    int num_words;      /* V, 0 = 16384 (at most 65536) */
    int train_iters;    /* T, 0 = 8 */
    int64_t train_rows; /* M, 0 = 64 V (at most 2^24: the sums stay in 32 bits) */
} msfm_retrieval_params;
/* Device time of the phases of the last msfm_train_vocabulary / msfm_retrieve_pairs calls (HIP events on the library's stream). */
typedef struct msfm_retrieval_profile {
    double train_ms;         /* sample gather + every Lloyd iteration */
    int train_iterations;    /* iterations run (an unchanged iteration ends the training) */
    double assign_ms;        /* the nearest word of every row of the retrieval call (ret_assign_kernel) */
    double score_ms;         /* histograms, idf, norms, S = A A^T */
    double topk_ms;          /* per-image top-K */
    int64_t rows;            /* rows assigned by the retrieval call */
    int num_words;           /* V' of the resident vocabulary */
} msfm_retrieval_profile;
/* Trains the vocabulary on the images `ids` (any order) and keeps it resident.  out_words (nullable): V' x 128 bytes c. */
int msfm_train_vocabulary(msfm_ctx* ctx, const int32_t* ids, int n, const msfm_retrieval_params* params, uint8_t* out_words,
                          int* out_num_words);
/* A caller's vocabulary (n_words x 128 bytes c, 1 <= n_words <= 65536) instead of training. */
int msfm_set_vocabulary(msfm_ctx* ctx, const uint8_t* words, int n_words);
/* The word of every row of one image (parity / debug): out_word = rows(image_id) int32. */
int msfm_image_words(msfm_ctx* ctx, int image_id, int32_t* out_word);
/* The retrieved pairs of the images `ids`: out_pairs (capacity n * num_nearest pairs) = (id1 > id2) int32 pairs in brute mode's order,
 * out_scores (nullable) their s, out_score_matrix (nullable, n x n in the order of `ids`, debug) every s_ij (0 on the diagonal). */
int msfm_retrieve_pairs(msfm_ctx* ctx, const int32_t* ids, int n, int num_nearest, int32_t* out_pairs, float* out_scores,
                        int* out_n_pairs, float* out_score_matrix);
int msfm_get_retrieval_profile(const msfm_ctx* ctx, msfm_retrieval_profile* out);

/* ---- feature tracks: the kept matches of a run, joined across pairs --------------------------------
 * Off by default.  What every consumer of a `matches` table does first is join the pairwise matches into multi-view correspondences:
 * the reference in SceneGraph::Load -> AddCorrespondences (src/Reconstruction/SceneGraph.cpp:11-85, 170-251: per-keypoint lists over the
 * pairs with at least min_num_matches = 10 matches, include/Reconstruction/MapBuilder.h:48), walked transitively while MapBuilder grows
 * its Tracks (src/Reconstruction/MapBuilder.cpp:333-340, 469-488).  A TRACK SESSION does it on the device while the lists are still in
 * HBM: one resident union-find forest, 4 bytes per keypoint, into which every sub-batch's final lists are folded as the sub-batch
 * completes -- in the streaming form too, so a job whose lists never fit memory still gets its tracks.  Exact integer work: the result
 * equals the host twin (csrc/msfm_tracks.h) and the numpy reference (tests/tracks_ref.py) element for element.
 *   nodes       msfm_tracks_begin declares the images (any order, distinct, resident).  Ranked by ascending id, the image of rank p has
 *               rows_p keypoints (its descriptor rows, msfm_image_rows) and base_p = rows_0 + .. + rows_(p-1); keypoint k of it is NODE
 *               base_p + k.
 *   edges       a match (q, t) of the pair (id1, id2) joins node (id1, q) and node (id2, t).  Per pair, in this order: an image outside
 *               the declared set (the pre-emptive filter's subsets live at MSFM_MAX_IMAGES + id) -> the pair is SKIPPED; id1 == id2 ->
 *               all its matches are IGNORED; a list shorter than min_pair_matches -> the pair contributes nothing (SceneGraph::Load's
 *               rule, SceneGraph.cpp:35, 68; 0 = every pair); else the pair is folded in, a match with an index outside [0, rows) of
 *               its image IGNORED as AddCorrespondences ignores it (SceneGraph.cpp:172-176, 198-248), every other one an edge (counted
 *               with its multiplicity: folding a list twice changes `edges`, not the tracks).
 *   while open  EVERY batch matching call on the context folds the lists it hands out: msfm_match_pairs, msfm_match_pairs_verified
 *               (the lists after verification / model selection), every chunk of msfm_match_pairs_begin / _next.  msfm_match_pair and
 *               msfm_knn2_pair do not take part.  msfm_tracks_add folds HOST lists in (CSR as msfm_match_pairs returns them): rows
 *               already in the database on a resumed run, lists verified on the host, lists of another process.
 *   forests     msfm_tracks_export_forest: one int32 per node, a node of the same component (no particular one);
 *               msfm_tracks_import_forest: every node v is joined with parent[v].  Contexts that declared the same images join their
 *               sessions this way (one context per GPU: the others' forests imported into the first).
 *   result      msfm_tracks_finish closes the accumulation (matching calls no longer fold, msfm_tracks_add / _import_forest return
 *               MSFM_E_STATE) and builds the result; it may be called again with another filter.  COMPONENT: a connected component of
 *               the node graph.  TRACK: a component of at least 2 nodes.  A track is CONSISTENT iff no two of its nodes belong to one
 *               image.  Kept: max(2, min_length) <= length, length <= max_length (0 = no bound), and consistent unless
 *               keep_inconsistent.  Kept tracks are numbered 0 .. T-1 by ascending smallest node, the elements of a track listed by
 *               ascending node, i.e. by (image id, keypoint index): a function of the SET of edges alone -- not of pair order,
 *               sub-batch cuts, streams, the number of contexts or the scheduling of atomics.
 *   stats       tracks_total / _inconsistent / _over_max_length count all tracks (before the filter); longest_track is the longest
 *               KEPT one; device_bytes what the session holds when msfm_tracks_finish returns (forest + result); fold_ms the summed HIP-event
 *               time of the fold kernels so far, finish_ms that of the last msfm_tracks_finish.
 * Errors: msfm_tracks_begin -- an id outside [0, MSFM_MAX_IMAGES), twice in the list, n < 0, 2^31 nodes or more: MSFM_E_INVALID; an id
 * not resident: MSFM_E_NOIMAGE; a session or a streaming series open: MSFM_E_STATE (a pending store build is done first).  Without a
 * session every other entry point here returns MSFM_E_STATE; so do the fetches before msfm_tracks_finish, msfm_tracks_finish while a
 * streaming series is open, and -- while a session is open -- msfm_clear_images and msfm_upload_image / msfm_subset_image INTO a
 * declared image.  msfm_tracks_import_forest: an entry outside [0, nodes) is MSFM_E_INVALID (nothing is joined then).
 * A matching call that FAILS (any status but MSFM_OK, in any of its sub-batches) may already have folded the sub-batches it completed
 * before the failure -- lists the caller never received; a repeat of the call leaves the tracks right (unions are idempotent) but
 * counts those edges and pairs twice.  After a failed matching call the session's content is therefore unspecified: msfm_tracks_end
 * it and begin again.  A msfm_tracks_finish that fails leaves the accumulation closed and no result (the fetches return MSFM_E_STATE
 * until a finish succeeds).
 * msfm_fetch_tracks: offsets T + 1 entries, image_ids / point_idx `observations_kept` entries, consistent T entries; any pointer may
 * be NULL.  msfm_fetch_track_ids: per keypoint of a declared image its kept track's number or -1.  msfm_tracks_end frees the session
 * (no session: MSFM_OK); msfm_destroy does too. */
typedef struct msfm_track_params {
    int32_t min_pair_matches;    /* 0 = every pair (the reference's MapBuilder::Parameters::min_num_matches: 10) */
    int32_t add_only;            /* != 0: the matching calls on the context do NOT fold; only msfm_tracks_add / _import_forest do (a caller
                                    whose stored lists are not the device's: host-side verification, rows filtered before they are written) */
} msfm_track_params;
typedef struct msfm_track_filter {
    int32_t min_length;          /* values below 2 mean 2 */
    int32_t max_length;          /* 0 = no bound */
    int32_t keep_inconsistent;
    int32_t reserved;
} msfm_track_filter;
typedef struct msfm_track_stats {   /* 120 bytes, no implicit padding */
    int64_t nodes;
    int64_t edges;                   /* matches folded in */
    int64_t pairs;                   /* pairs folded in */
    int64_t pairs_skipped;           /* an image outside the declared set */
    int64_t pairs_below_min;         /* shorter than min_pair_matches */
    int64_t matches_ignored;         /* index out of range, or a pair with id1 == id2 */
    int64_t tracks_total;
    int64_t tracks_inconsistent;
    int64_t tracks_over_max_length;
    int64_t tracks_kept;             /* T */
    int64_t observations_kept;
    int64_t longest_track;
    int64_t device_bytes;
    double fold_ms;
    double finish_ms;
} msfm_track_stats;
int msfm_tracks_begin(msfm_ctx* ctx, const int32_t* ids, int n, const msfm_track_params* params);
int msfm_tracks_add(msfm_ctx* ctx, const int32_t* pairs, int n_pairs, const int64_t* offsets, const int32_t* qt);
int msfm_tracks_export_forest(msfm_ctx* ctx, int32_t* parent);
int msfm_tracks_import_forest(msfm_ctx* ctx, const int32_t* parent);
int msfm_tracks_finish(msfm_ctx* ctx, const msfm_track_filter* filter, msfm_track_stats* stats);
int msfm_fetch_tracks(msfm_ctx* ctx, int64_t* offsets, int32_t* image_ids, int32_t* point_idx, uint8_t* consistent);
int msfm_fetch_track_ids(msfm_ctx* ctx, int image_id, int32_t* out);
int msfm_tracks_end(msfm_ctx* ctx);

/* ---- track triangulation: 3-D points from the kept tracks and known poses --------------------------
 * Off by default; needs a track session with a successful msfm_tracks_finish.  What the reference's MapBuilder::Triangulate ->
 * Triangulator::Triangulate does with a multi-view correspondence (src/Reconstruction/Triangulator.cpp:15-117, MapBuilder.cpp:516-560):
 * the multi-view DLT point, the reprojection test in every view, the parallax test -- for every kept track at once, on the device,
 * from the track result, the uploaded keypoints and a pose table given with the call (poses of a rig, an INS, an earlier
 * reconstruction, the two-view record of an initial pair).  The arithmetic is csrc/msfm_triangulate.h, bit-identical to the host twin
 * TriangulateTracks.  Nothing else changes: not the tracks, not the match lists.
 *   poses       n_poses entries, image_ids[k] (declared in the session, each at most once) with poses[k]: x_cam = R X + t, R row-major.
 *               R is taken as given: it is NOT re-orthogonalised.  valid == 0: the image counts as unposed (as every declared image
 *               that is not listed).
 *   attempted   a track is attempted iff it is consistent and at least max(2, min_views) of its elements lie in posed images; those
 *               are its USED OBSERVATIONS, in element order; the others are skipped.  Else status = 0 and every field 0.
 *   observation pixel (fp32 -> fp64) -> normalised undistorted (u, v) with `camera`; errors are measured against it and scaled by
 *               f = (fx + fy) / 2 (the two-view records' convention; the reference folds K into P and uses the distorted pixels).
 *   point       A = sum over the used observations of r1^T r1 + r2^T r2, r1 = u P.row(2) - P.row(0), r2 = v P.row(2) - P.row(1),
 *               P = [R | t]; the right singular vector of the smallest singular value, X = h[0..2] / h[3]; h[3] == 0 or a non-finite
 *               X: no point.
 *   errors      per used observation err = |proj(R X + t) - (u, v)| f; ERROR_OK iff every err <= max_error (NaN fails);
 *               mean_residual = their sum in observation order / n_views.  Every error is reported: out_residuals is aligned with
 *               the tracks' observations (observations_kept doubles), -1.0 where none was computed (unposed elements, tracks not
 *               attempted or without a point).
 *   parallax    pairs of used observations in the order for i: for j < i; the first pair whose angle at X between the two camera
 *               centres (-R^T t) is >= min_angle ends the scan: tri_angle is its angle and ANGLE_OK is set; if none reaches it,
 *               tri_angle is the largest angle seen.  Degrees, min(a, pi - a).
 *   status      MSFM_TRI_ATTEMPTED | _POINT | _ERROR_OK | _ANGLE_OK | _DEPTH_OK.  The reference's is_succeed is POINT & ERROR_OK &
 *               ANGLE_OK.  DEPTH_OK (every used view has the point in front of it, depth > DBL_EPSILON) is extra information: the
 *               reference has no depth test, and it is not part of the verdict.
 * params NULL = the reference's Triangulator::Parameters {2.0 px, 1.5 degrees} and min_views 2.
 * Errors: MSFM_E_STATE -- no track session, before a successful msfm_tracks_finish, or while a streaming series is open.
 * MSFM_E_INVALID -- NULL camera; fx / fy <= 0; a non-finite camera or triangulation parameter; a non-finite R or t of a valid pose; an
 * image id that is not declared in the session, or given twice; a negative max_error or min_angle; n_poses < 0.  MSFM_E_NOIMAGE -- a
 * posed image without uploaded keypoints (fewer keypoints than rows).  After an error the previous points (if any) are gone.
 * A later msfm_tracks_finish invalidates the points: msfm_fetch_points3d returns MSFM_E_STATE until msfm_triangulate_tracks has run
 * again.  msfm_tracks_end frees them.  msfm_fetch_points3d: T = tracks_kept records, observations_kept doubles; either may be NULL. */
enum { MSFM_TRI_ATTEMPTED = 1, MSFM_TRI_POINT = 2, MSFM_TRI_ERROR_OK = 4, MSFM_TRI_ANGLE_OK = 8, MSFM_TRI_DEPTH_OK = 16 };
typedef struct msfm_pose_rt {   /* 104 bytes, no implicit padding */
    int32_t valid;
    int32_t reserved;
    double R[9];
    double t[3];
} msfm_pose_rt;
typedef struct msfm_triangulation_params {
    double max_error;            /* Triangulator::Parameters::regis_tri_max_error: 2.0 pixels */
    double min_angle;            /* regis_tri_min_angle: 1.5 degrees */
    int32_t min_views;           /* values below 2 mean 2 */
    int32_t reserved;
} msfm_triangulation_params;
typedef struct msfm_point3d {   /* 48 bytes, no implicit padding */
    int32_t status;
    int32_t n_views;             /* used observations */
    double X[3];
    double mean_residual;
    double tri_angle;
} msfm_point3d;
typedef struct msfm_triangulation_stats {   /* 80 bytes, no implicit padding */
    int64_t tracks;              /* T: records written */
    int64_t attempted;           /* counts per status bit ... */
    int64_t with_point;
    int64_t error_ok;
    int64_t angle_ok;
    int64_t depth_ok;
    int64_t succeeded;           /* ... and of POINT & ERROR_OK & ANGLE_OK */
    int64_t observations_used;   /* summed n_views */
    int64_t device_bytes;        /* records + residuals held by the session */
    double triangulate_ms;       /* HIP events around the two kernels */
} msfm_triangulation_stats;
int msfm_triangulate_tracks(msfm_ctx* ctx, const msfm_camera* camera, const int32_t* image_ids, const msfm_pose_rt* poses, int n_poses,
                            const msfm_triangulation_params* params, msfm_triangulation_stats* stats);
int msfm_fetch_points3d(msfm_ctx* ctx, msfm_point3d* out_points, double* out_residuals);

/* ---- robust track triangulation: reject outlier observations per track (opt-in) ---------------
 * msfm_triangulate_tracks is all or nothing: one observation beyond max_error clears ERROR_OK and the whole track is lost.  This
 * second entry point takes the same inputs, writes the same session outputs (msfm_fetch_points3d, msfm_register_images work after it
 * unchanged) and adds one inlier byte per kept observation.  The arithmetic is csrc/msfm_triangulate.h, bit-identical to the host twin
 * TriangulateTracksRobust.  For a track with the used observations 0 .. m - 1, need = max(2, min_views):
 *   plain pass   P0 = the record of msfm_triangulate_tracks.  Not ATTEMPTED, or POINT & ERROR_OK, or m < 3: the record is P0 bit for
 *                bit, the inlier byte is 1 on every used observation, MSFM_TRI_ROBUST is clear.  Every other track is RETRIED:
 *   hypotheses   H = min(m (m - 1) / 2, max_hypotheses) pairs of used observations: all pairs in the order for i: for j < i when they
 *                fit, else distinct positions from the counter stream keyed by the track number.  X_h = the two-view DLT point; valid
 *                iff it exists, lies in front of both views and subtends >= min_angle at their centres.  Its count: the used
 *                observations with depth > DBL_EPSILON and err <= max_error.  Best = the largest count, the lowest h among equals.
 *                None valid, or a best count < need: status = ATTEMPTED | ROBUST, every other field 0, residuals -1, inlier bytes 0.
 *   refit, once  the DLT over the inliers of X_best stands iff it has a point and at least max(|inliers of X_best|, need) inliers
 *                among all used observations (the rule of MSFM_REG_REFINED); else X_best stands with its inliers.
 *   record       an error for EVERY used observation (the caller sees why one was dropped), n_views = the number of inliers,
 *                mean_residual and the parallax scan over the inliers only, ERROR_OK set, DEPTH_OK over the inliers, ROBUST set.
 * Inconsistent tracks stay unattempted.  params NULL = {2.0 px, 1.5 degrees, 2, 64}.  Errors: every check of msfm_triangulate_tracks
 * with the same codes; MSFM_E_INVALID also for max_hypotheses outside 1 .. 1024.  The call invalidates earlier points and
 * registrations like msfm_triangulate_tracks.  msfm_fetch_point_inliers copies observations_kept bytes aligned with the tracks'
 * observations; MSFM_E_STATE unless the last successful triangulation of the session was the robust one (msfm_tracks_finish and
 * msfm_triangulate_tracks invalidate the bytes, msfm_tracks_end frees them). */
enum { MSFM_TRI_ROBUST = 32 };
typedef struct msfm_robust_triangulation_params {   /* 24 bytes, no implicit padding */
    double max_error;
    double min_angle;
    int32_t min_views;           /* values below 2 mean 2 */
    int32_t max_hypotheses;      /* 1 .. 1024 */
} msfm_robust_triangulation_params;
typedef struct msfm_robust_stats {   /* 40 bytes, no implicit padding */
    int64_t retried;                 /* tracks that went through the hypotheses */
    int64_t rescued;                 /* ... of which end with POINT & ANGLE_OK */
    int64_t observations_rejected;   /* used observations with inlier byte 0 on tracks that have a point */
    int64_t hypotheses;              /* summed H of the retried tracks */
    double robust_ms;                /* HIP events around all launches of the call (the wait for the retry list included) */
} msfm_robust_stats;
int msfm_triangulate_tracks_robust(msfm_ctx* ctx, const msfm_camera* camera, const int32_t* image_ids, const msfm_pose_rt* poses,
                                   int n_poses, const msfm_robust_triangulation_params* params, msfm_triangulation_stats* stats,
                                   msfm_robust_stats* robust_stats);
int msfm_fetch_point_inliers(msfm_ctx* ctx, uint8_t* out);

/* ---- point refinement: per-track Levenberg-Marquardt on the reprojection error (opt-in) ---------------
 * The triangulation calls return the DLT point, which minimises an algebraic error.  msfm_refine_points moves every point of the
 * session's last successful triangulation to the minimum of its reprojection error under the FIXED poses of that call: one 3 x 3
 * system per point, nothing shared between tracks, no pose is ever changed.  The arithmetic is csrc/msfm_refine.h, bit-identical to
 * the host twin RefinePoints.
 *   inputs       none besides the context: the session keeps a host copy of the camera, the thresholds and the (image id, pose) list
 *                of the last successful msfm_triangulate_tracks / _robust; the call rebuilds its device tables from them (keypoint
 *                pointers are looked up fresh) and frees them when it returns.
 *   eligible     a track whose record has ATTEMPTED | POINT.  Its fitting set: its used observations -- after the robust call those
 *                whose inlier byte is 1.
 *   cost         the sum over the fitting set of |proj(R X + t) - (u, v)|^2 f^2, (u, v) and f as msfm_triangulate_tracks defines them.
 *   LM           H = sum J^T J, g = sum J^T r in observation order; (H + lambda diag H) delta = -g by a 3 x 3 Cholesky (a pivot that
 *                is not > 0 or a non-finite delta is a rejected step); a step is accepted iff its cost is finite, strictly lower and
 *                every fitting view keeps depth > DBL_EPSILON; accept: lambda / 10 (floor 1e-12), reject: 10 lambda; lambda starts
 *                at 1e-3.  A track stops after max_iters evaluated steps, after an accepted step with
 *                |delta|^2 <= step_tol^2 (|X|^2 + step_tol), or when a rejected step raises lambda past 1e4.
 *   verdict      recomputed at the refined point with the triangulation's code and thresholds: an error for EVERY used observation;
 *                mean_residual, the parallax scan, ERROR_OK and DEPTH_OK over the fitting set.  The refined point STANDS iff a step
 *                was accepted (its cost is strictly lower) and none of ERROR_OK, ANGLE_OK, DEPTH_OK that the record had is cleared.
 *                Then the record gets the new X, errors, mean_residual, tri_angle and bits plus MSFM_TRI_REFINED (ROBUST is kept).
 *                Otherwise the record and its residuals stay bit for bit what they were, an earlier REFINED bit included.
 * n_views, the inlier bytes, the tracks and the match lists never change; the succeeded set can only grow; max_iters = 0 changes
 * nothing.  The call may be repeated: it refines from the current records.  It invalidates registrations like a triangulation call
 * (msfm_fetch_registrations returns MSFM_E_STATE until msfm_register_images has run again); points and inlier bytes stay valid.
 * params NULL = {1e-10, 10}.  Errors: MSFM_E_STATE -- no track session, no successful msfm_triangulate_tracks / _robust since the last
 * msfm_tracks_finish, a streaming series open.  MSFM_E_INVALID -- max_iters outside 0 .. 100, a non-finite or negative step_tol.
 * MSFM_E_NOIMAGE -- a posed image whose keypoints have been replaced by fewer than its rows.
 * cost_before / cost_after: the eligible tracks' costs at the records' points before and after the call, information only (each
 * wave's tracks are summed in a fixed order, the waves' sums in wave order on the host: reproducible on one device, not bit-equal to
 * the twin's sum in track order). */
enum { MSFM_TRI_REFINED = 64 };
typedef struct msfm_refine_params {   /* 16 bytes, no implicit padding */
    double step_tol;
    int32_t max_iters;               /* 0 .. 100 evaluated steps per track */
    int32_t reserved;
} msfm_refine_params;
typedef struct msfm_refine_stats {   /* 72 bytes, no implicit padding */
    int64_t eligible;                /* tracks with ATTEMPTED | POINT */
    int64_t refined;                 /* ... whose refined point stands */
    int64_t gained_error_ok;         /* ... of which gain ERROR_OK */
    int64_t rejected_by_verdict;     /* tracks with an accepted step whose refined point would clear a status bit */
    int64_t iterations;              /* evaluated steps, summed */
    double cost_before;
    double cost_after;
    double refine_ms;                /* HIP events around all launches of the call */
    double prepare_ms;               /* ... of which the pose table and the per-observation array */
} msfm_refine_stats;
int msfm_refine_points(msfm_ctx* ctx, const msfm_refine_params* params, msfm_refine_stats* stats);

/* ---- pose refinement: per-image Levenberg-Marquardt on the reprojection error (opt-in) ---------------
 * The other block of the alternation: msfm_refine_poses moves every posed image of the session's last successful triangulation to
 * the minimum of the SAME pixel cost under FIXED points: one 6 x 6 system per image, nothing shared between images, no point's X is
 * ever changed.  The arithmetic is csrc/msfm_refine_poses.h, bit-identical to the host twin RefinePoses.
 *   inputs       none besides the context and the images to hold fixed: like msfm_refine_points the call works on what the last
 *                successful msfm_triangulate_tracks / _robust left in the session (camera, thresholds, pose list, records, residuals,
 *                inlier bytes), with the poses as earlier msfm_refine_poses calls left them.
 *   fitting set  of a listed image with a valid pose that is not fixed: its observations (after the robust call those whose inlier
 *                byte is 1) of tracks whose record has ATTEMPTED | POINT | ERROR_OK | ANGLE_OK, by ascending track number.
 *   eligible     such an image with at least min_observations entries.
 *   cost         the sum over the fitting set of |proj(R X + t) - (u, v)|^2 f^2: msfm_refine_points' cost.
 *   LM           27 sums (J^T J, J^T r of the unknowns (a, dt):  R <- C(a) R,  t <- C(a) t + dt,  C Cayley's rotation), 64 partials by
 *                list position modulo 64, then a butterfly;  (H + lambda diag H) delta = -g by a 6 x 6 Cholesky (a pivot that is not
 *                > 0, a non-finite delta or pose is a rejected step); a step is accepted iff its cost is finite, strictly lower and
 *                every fitting observation keeps depth > DBL_EPSILON; accept: lambda / 10 (floor 1e-12), reject: 10 lambda; lambda
 *                starts at 1e-3.  An image stops after max_iters evaluated steps, after an accepted step with
 *                |delta|^2 <= step_tol^2 (1 + |t|^2), or when a rejected step raises lambda past 1e4.
 *   standing     the refined pose STANDS iff a step was accepted and it has at least as many fitting observations with positive depth
 *                and err <= the triangulation's max_error as the old pose (the rule of MSFM_REG_REFINED).  It then replaces the
 *                session's pose of that image; otherwise not one byte of that pose changes.
 *   re-verdict   every track with ATTEMPTED | POINT and a used observation in an image whose pose changed is evaluated again at its
 *                unchanged X under the new poses (camera centres included) with the triangulation's code and thresholds: an error for
 *                every used observation, mean_residual, tri_angle, ERROR_OK, ANGLE_OK, DEPTH_OK over the fitting set, plus
 *                MSFM_TRI_REPOSED.  ROBUST, REFINED, n_views, X and the inlier bytes are kept; the succeeded set may shrink or grow
 *                (points_lost / points_gained).  Tracks that touch no changed image stay bit for bit.
 * max_iters = 0 changes nothing.  The call may be repeated.  It invalidates registrations like msfm_refine_points; points and inlier
 * bytes stay valid; a following msfm_refine_points / msfm_register_images sees the new poses and records.
 * params NULL = {1e-6, 10, 15}.  Errors: MSFM_E_STATE -- as msfm_refine_points.  MSFM_E_INVALID -- max_iters outside 0 .. 100, a
 * non-finite or negative step_tol, min_observations < 3, n_fixed < 0 or a NULL list with n_fixed > 0, a fixed id that is not declared
 * in the session or given twice.  MSFM_E_NOIMAGE -- as msfm_refine_points.
 * cost_before / cost_after: the records' costs added in list order (a record that was not attempted adds 0): bit-equal to the twin's.
 * msfm_fetch_poses: the session's current pose list in the triangulation call's order; *n receives its length, NULL arrays return it
 * alone.  Valid after any successful triangulation (it then returns the caller's poses bit for bit); MSFM_E_STATE otherwise.
 * msfm_fetch_pose_refinements: one record per listed image in that order; MSFM_E_STATE unless msfm_refine_poses was the last
 * successful call that rebuilt the session's pose tables (a triangulation or msfm_refine_points after it invalidates the records).
 *   record       status MSFM_POSE_FIXED: the image is in the fixed list; _ATTEMPTED: eligible; _REFINED: its refined pose stands.
 *                n_observations: the fitting set (0 for an image that is fixed or has no valid pose); iterations: evaluated steps;
 *                stop: 0 not attempted, 1 step criterion, 2 max_iters, 3 lambda ceiling; inliers_before / _after: the standing
 *                rule's counts; cost_before / cost_after: the cost at the old pose and at the pose that stands. */
enum { MSFM_TRI_REPOSED = 128 };
enum { MSFM_POSE_ATTEMPTED = 1, MSFM_POSE_REFINED = 2, MSFM_POSE_FIXED = 4 };
typedef struct msfm_pose_refine_params {   /* 16 bytes, no implicit padding */
    double step_tol;
    int32_t max_iters;               /* 0 .. 100 evaluated steps per image */
    int32_t min_observations;        /* >= 3 */
} msfm_pose_refine_params;
typedef struct msfm_pose_refine_stats {   /* 104 bytes, no implicit padding */
    int64_t images;                  /* listed images */
    int64_t eligible;
    int64_t refined;                 /* ... whose refined pose stands */
    int64_t rejected_by_inliers;     /* images with an accepted step whose refined pose would lose an inlier */
    int64_t iterations;              /* evaluated steps, summed */
    int64_t observations;            /* the fitting sets, summed */
    int64_t points_reposed;          /* tracks that went through the re-verdict */
    int64_t points_lost;             /* ... of which had POINT & ERROR_OK & ANGLE_OK and lost it */
    int64_t points_gained;           /* ... of which gained it */
    double cost_before;
    double cost_after;
    double refine_ms;                /* HIP events around all launches of the call */
    double prepare_ms;               /* ... of which the pose table, the per-observation array and the image-major list */
} msfm_pose_refine_stats;
typedef struct msfm_pose_refinement {   /* 48 bytes, no implicit padding */
    int32_t image_id;
    int32_t status;
    int32_t n_observations;
    int32_t iterations;
    int32_t stop;
    int32_t inliers_before;
    int32_t inliers_after;
    int32_t reserved;
    double cost_before;
    double cost_after;
} msfm_pose_refinement;
int msfm_refine_poses(msfm_ctx* ctx, const msfm_pose_refine_params* params, const int32_t* fixed_image_ids, int n_fixed,
                      msfm_pose_refine_stats* stats);
int msfm_fetch_poses(msfm_ctx* ctx, int32_t* out_ids, msfm_pose_rt* out_poses, int* n);
int msfm_fetch_pose_refinements(msfm_ctx* ctx, msfm_pose_refinement* out);

/* ---- camera refinement: Levenberg-Marquardt on focal length, centre and distortion (opt-in) ---------------
 * The third block of the alternation, the reference's refine_focal_length (CeresBundleOptimizer's shared focal block) and a little
 * more: msfm_refine_camera moves the session's ONE camera -- the msfm_camera that msfm_triangulate_tracks was given and every later
 * call reads back -- to the minimum of the SAME pixel cost under FIXED poses and FIXED points: one dense system of at most 6 unknowns
 * per call, no coupling to any other block.  The arithmetic is csrc/msfm_refine_camera.h, bit-identical to the host twin RefineCamera
 * (DESIGN.md section 25).
 *   unknowns     params.mask: MSFM_CAM_FX_FY (fx and fy, the default), MSFM_CAM_F (one scale s: fx <- fx (1 + s), fy <- fy (1 + s);
 *                exclusive with FX_FY), MSFM_CAM_CX_CY, MSFM_CAM_K1_K2.  p1 and p2 never move.
 *   contributing an observation of a track whose record has ATTEMPTED | POINT | ERROR_OK | ANGLE_OK, in an image with a valid pose,
 *                whose inlier byte is 1 after a robust call, with positive depth (`behind` counts those left out by depth alone).
 *                The set does not depend on the camera and is fixed for the call.
 *   cost         the sum over the set of |proj(R X + t) - undistort(camera; keypoint)|^2 f^2, f = (fx + fy) / 2: msfm_refine_points'
 *                and msfm_refine_poses' cost with the camera as the variable.
 *   LM           28 sums (J^T J, J^T r, the cost; the Jacobian in closed form through the implicit function theorem on the Brown
 *                model) added in an order fixed by the data -- chunks of 256 observations in the tracks' order, a fixed tree inside
 *                a chunk, 256 strided partials over the chunks, the same tree -- so that neither the grid nor the CU count reaches a
 *                bit;  (H + lambda diag H) delta = -g by the 6 x 6 Cholesky of the pose refinement (an unknown that is not selected
 *                has H_ii = 1, g_i = 0); a pivot that is not > 0, a non-finite delta or camera, fx or fy not > 0 is a rejected step;
 *                a step is accepted iff its cost is finite and strictly lower; accept: lambda / 10 (floor 1e-12), reject: 10 lambda;
 *                lambda starts at 1e-3.  The call stops after max_iters evaluated steps, after an accepted step with
 *                (dfx / fx)^2 + (dfy / fy)^2 + (dcx / f)^2 + (dcy / f)^2 + dk1^2 + dk2^2 <= step_tol^2, or when a rejected step
 *                raises lambda past 1e4.  There are no box constraints: strict descent and the standing rule are the protection.
 *   eligible     at least min_observations contributing observations and a finite starting cost; otherwise nothing is attempted.
 *   standing     the refined camera STANDS iff a step was accepted and it has at least as many contributing observations with
 *                err <= the triangulation's max_error as the old camera.  It then replaces the session's camera; otherwise not one
 *                byte of the session's camera, points, residuals or poses changes.
 *   re-verdict   when it stands, EVERY track with ATTEMPTED | POINT is evaluated again at its unchanged X under the unchanged poses
 *                and the new camera with the triangulation's code and thresholds: an error for every used observation,
 *                mean_residual, tri_angle, ERROR_OK, ANGLE_OK, DEPTH_OK over the fitting set, plus MSFM_TRI_RECALIBRATED.  ROBUST,
 *                REFINED, REPOSED, EXTENDED, FILTERED, COMPLETED, n_views, X and the inlier bytes are kept; the succeeded set may
 *                shrink or grow (points_lost / points_gained).
 * max_iters = 0 changes nothing.  The call may be repeated.  It invalidates registrations and pose-refinement records like
 * msfm_refine_points; points, inlier bytes and poses stay valid.  Every following msfm_refine_points / msfm_refine_poses /
 * msfm_extend_points / msfm_filter_points / msfm_complete_points / msfm_map_visibility works under the new camera.  A later
 * msfm_refine_points / msfm_refine_poses / msfm_filter_points / msfm_complete_points CLEARS MSFM_TRI_RECALIBRATED on every record it
 * rewrites (the filter and the completion too, which keep EXTENDED); msfm_extend_points keeps it on a point it continues, as it keeps
 * every bit, and a track it creates has none: the bit says that the record is as a camera refinement left it, but for observations
 * continued into new images.  msfm_register_images takes its own camera: pass
 * msfm_fetch_camera's.
 * params NULL = {1e-6, MSFM_CAM_FX_FY, 10, 100}.  Errors: MSFM_E_STATE -- as msfm_refine_points.  MSFM_E_INVALID -- mask 0, a bit
 * outside the four, FX_FY together with F, max_iters outside 0 .. 100, a non-finite or negative step_tol, min_observations < 6.
 * MSFM_E_NOIMAGE -- as msfm_refine_points.
 *   stats        observations: the contributing set; stop: 0 none, 1 step criterion, 2 max_iters, 3 lambda ceiling, 4 fewer than
 *                min_observations contribute, 5 the starting cost is not finite; refined: 1 iff the camera stands;
 *                rejected_by_inliers: 1 iff a step was accepted and the camera does not stand; cost_before / cost_after: the cost at
 *                the old camera and at the camera that stands (0 where nothing was attempted); camera_after = camera_before unless
 *                it stands.  All but refine_ms are bit-equal to the twin's.
 * msfm_fetch_camera: the session's current camera; MSFM_E_STATE before a successful triangulation. */
enum { MSFM_TRI_RECALIBRATED = 2048 };
enum { MSFM_CAM_FX_FY = 1, MSFM_CAM_F = 2, MSFM_CAM_CX_CY = 4, MSFM_CAM_K1_K2 = 8 };
typedef struct msfm_camera_refine_params {   /* 24 bytes, no implicit padding */
    double step_tol;
    int32_t mask;                    /* MSFM_CAM_* */
    int32_t max_iters;               /* 0 .. 100 evaluated steps */
    int32_t min_observations;        /* >= 6 */
    int32_t reserved;
} msfm_camera_refine_params;
typedef struct msfm_camera_refine_stats {   /* 248 bytes, no implicit padding */
    int64_t observations;            /* the contributing set */
    int64_t behind;                  /* otherwise fitting observations left out by depth */
    int64_t iterations;              /* evaluated steps */
    int64_t accepted_steps;
    int64_t stop;
    int64_t refined;                 /* 0 / 1: the refined camera stands */
    int64_t rejected_by_inliers;     /* 0 / 1: a step was accepted and the refined camera would lose an inlier */
    int64_t inliers_before;
    int64_t inliers_after;
    int64_t points_recalibrated;     /* tracks that went through the re-verdict */
    int64_t points_lost;             /* ... of which had POINT & ERROR_OK & ANGLE_OK and lost it */
    int64_t points_gained;           /* ... of which gained it */
    double cost_before;
    double cost_after;
    msfm_camera camera_before;
    msfm_camera camera_after;
    double refine_ms;                /* HIP events around all launches of the call */
} msfm_camera_refine_stats;
int msfm_refine_camera(msfm_ctx* ctx, const msfm_camera_refine_params* params, msfm_camera_refine_stats* stats);
int msfm_fetch_camera(msfm_ctx* ctx, msfm_camera* out);

/* ---- map extension: continue and create points under new poses (opt-in) ---------------
 * The step that makes the blocks above an INCREMENTAL reconstruction (the reference's MapBuilder::TryRegisterNextImage after the
 * pose is found: AddObservation, Map::CompletePoint3D, MapBuilder::Triangulate).  msfm_extend_points takes the poses of newly
 * registered images, continues the session's standing points into those images WITHOUT moving them, and triangulates the tracks that
 * only now have enough posed views.  A track that sees none of the new images stays bit for bit.  The arithmetic is
 * csrc/msfm_extend.h, bit-identical to the host twin ExtendPoints.
 *   inputs       the (image id, pose) list of the NEW images only; no camera and no thresholds: like msfm_refine_points the call
 *                works on what the last successful msfm_triangulate_tracks / _robust left in the session (camera, thresholds, pose
 *                list, records, residuals, inlier bytes), with the poses as msfm_refine_poses left them.
 *   new images   every listed id is declared in the session, listed once, and UNPOSED in the session's pose list (absent, or present
 *                with valid == 0).  An entry with valid == 0 is accepted and changes nothing.  On success an absent image with a
 *                valid pose is appended to the session's pose list in the call's order, a valid == 0 entry of the session's list is
 *                replaced in place; msfm_fetch_poses returns the enlarged list.
 *   inlier bytes the call needs one byte per kept observation.  A session whose points are the plain call's gets them first: 1 on
 *                every used observation of an attempted track, else 0 (what the robust call gives a track that passes its plain
 *                test).  After a successful call the bytes are valid whatever the triangulation was: msfm_fetch_point_inliers works
 *                and msfm_refine_points / msfm_refine_poses take their fitting sets from them (on a plain session this changes none
 *                of their results: every used observation has byte 1).
 *   new observation   an element of a kept track in an image that gained a valid pose in this call.
 *   untouched    a track without a new observation, an inconsistent track, every track at n_poses == 0: record, residual slots and
 *                inlier bytes stay bit for bit.
 *   continue     the record has POINT | ERROR_OK | ANGLE_OK.  X never changes.  Per new observation: err = the reprojection error
 *                at X under the new pose (pixels, f = (fx + fy) / 2); its residual slot = err; its inlier byte = 1 iff depth >
 *                DBL_EPSILON and err <= the SESSION'S max_error, else 0.  (The reference's complete_max_reproj_error is a looser
 *                4 px; the session's own threshold is used so that a continued point never fails the test it was admitted by.  The
 *                registration's inlier flags are not consulted: the poses may come from any source.)  At least one accepted:
 *                n_views = the byte-1 observations; mean_residual = their residual slots summed in element order / n_views (old
 *                slots are read, not recomputed, and never rewritten); tri_angle = the parallax scan over them in element order;
 *                status = every bit it had | MSFM_TRI_EXTENDED (ERROR_OK, DEPTH_OK and ANGLE_OK cannot be lost).  None accepted:
 *                the record stays bit for bit, only the new slots and bytes are written.
 *   create       every other consistent track with a new observation is triangulated afresh over all its elements in posed images
 *                under the enlarged pose list: max_hypotheses == 0 by msfm_triangulate_tracks' rule, 1 .. 1024 by
 *                msfm_triangulate_tracks_robust's.  Record, residual slots and inlier bytes are replaced by that result |
 *                MSFM_TRI_EXTENDED (an earlier REFINED / REPOSED bit goes with the old record): apart from that one bit a created
 *                track is byte for byte what the full triangulation call gives it under the enlarged pose list.
 * The call invalidates registrations and pose-refinement records like msfm_refine_points.  params NULL = {0}.
 * Errors, after each of which the session is exactly what it was: MSFM_E_STATE -- as msfm_refine_points.  MSFM_E_INVALID --
 * max_hypotheses outside 0 .. 1024, n_poses < 0 or a NULL list with n_poses > 0, an id that is not declared in the session, given
 * twice or already posed in the session (changing a pose is msfm_refine_poses' or a full triangulation's job), non-finite R or t of a
 * valid pose.  MSFM_E_NOIMAGE -- a posed image with fewer keypoints than rows.
 * The counters only count: no order reaches an output. */
enum { MSFM_TRI_EXTENDED = 256 };
typedef struct msfm_extend_params {   /* 8 bytes, no implicit padding */
    int32_t max_hypotheses;          /* 0: created tracks take the plain route; 1 .. 1024: the robust one */
    int32_t reserved;
} msfm_extend_params;
typedef struct msfm_extend_stats {   /* 96 bytes, no implicit padding */
    int64_t images_added;            /* listed images that gained a valid pose */
    int64_t tracks_touched;          /* consistent tracks with a new observation */
    int64_t continued;               /* ... whose standing point accepted at least one */
    int64_t observations_added;      /* new observations accepted by standing points */
    int64_t observations_rejected;   /* ... and rejected by them (by error or depth) */
    int64_t created_attempted;       /* touched tracks that were triangulated afresh */
    int64_t created;                 /* ... of which end with POINT & ERROR_OK & ANGLE_OK */
    int64_t retried;                 /* ... of which went through the robust hypotheses */
    int64_t succeeded;               /* POINT & ERROR_OK & ANGLE_OK over all tracks after the call */
    int64_t observations_used;       /* n_views summed over all tracks after the call */
    double extend_ms;                /* HIP events around all launches of the call (the wait for the retry list included) */
    double prepare_ms;               /* ... of which the pose table, the inlier bytes and the per-observation array */
} msfm_extend_stats;
int msfm_extend_points(msfm_ctx* ctx, const int32_t* image_ids, const msfm_pose_rt* poses, int n_poses,
                       const msfm_extend_params* params, msfm_extend_stats* stats);

/* ---- map filtering: drop outlier observations and weak points (opt-in) ---------------
 * The step the reference runs after every local or global adjustment (MapBuilder::FilterTracks / FilterAllTracks ->
 * Map::FilterPoints3DWithLargeReprojectionError, then ...WithSmallTriangulationAngle).  msfm_filter_points takes observations that no
 * longer fit their point out of its fitting set and removes the points that are left with fewer than two observations or without a
 * wide pair: the only call of this library that takes anything out of the map.  No X and no pose ever changes.  The arithmetic is
 * csrc/msfm_filter.h, bit-identical to the host twin FilterPoints.
 *   inputs       none besides the context, the thresholds and the scope: like msfm_refine_points the call works on what the last
 *                successful msfm_triangulate_tracks / _robust left in the session (camera, thresholds, pose list, records, residuals,
 *                inlier bytes), with the poses as msfm_refine_poses and msfm_extend_points left them.
 *   thresholds   max_error in pixels, min_angle in degrees.  params NULL = the SESSION's own max_error and min_angle: a point is
 *                judged by the test it was admitted by (the reference's filtered_max_reproj_error is a looser 4 px).  Explicit
 *                values may be tighter or looser than the session's.
 *   inlier bytes the call needs one byte per kept observation.  A session without them gets them first, exactly as
 *                msfm_extend_points creates them: 1 on every used observation of an attempted track, else 0.  After a successful
 *                call the bytes are valid whatever the triangulation was.
 *   scope        n_images == 0: every track.  Otherwise only the tracks with a fitting observation in a listed image (the
 *                reference's FilterPoints3DInImage / GetModifiedPoint3DIds).  A listed image without a valid pose selects nothing.
 *   eligible     a consistent track whose record has ATTEMPTED | POINT and which is in scope.  Its fitting set F: its used
 *                observations whose inlier byte is 1, in element order.  Every other track stays bit for bit.
 *   drop         per observation of F: err = the reprojection error at the record's X under the current pose (pixels, f = (fx + fy)
 *                / 2).  Dropped by depth iff its depth is not > DBL_EPSILON; otherwise dropped by error iff !(err <= max_error) (a
 *                NaN is dropped).  K: the survivors.
 *   removed      by views iff |K| < 2; otherwise by angle iff the parallax scan over K in element order with the CALL's min_angle
 *                finds no pair, whether or not anything was dropped.  The record becomes status = MSFM_TRI_ATTEMPTED |
 *                MSFM_TRI_FILTERED with every other field 0, every residual slot of the track -1.0 and every inlier byte of the
 *                track 0 (the robust call's "no consensus" record).  It is no longer POINT: registration and the refinements skip
 *                it, msfm_extend_points creates it afresh when a new image sees it.
 *   untouched    nothing dropped and not removed: not one byte is written, the residual slots included.
 *   trimmed      something dropped and not removed.  The dropped observations' bytes become 0.  The record is evaluated again over K
 *                at the unchanged X with the SESSION's thresholds and the triangulation's code: an error for every used observation
 *                (the dropped ones keep theirs), n_views = |K|, mean_residual = the errors of K summed in element order / |K|,
 *                tri_angle, ERROR_OK, ANGLE_OK, DEPTH_OK over K;  status = ATTEMPTED | POINT | those bits | the record's ROBUST,
 *                REFINED, REPOSED, EXTENDED | MSFM_TRI_FILTERED.  regained: a trimmed track that did not have POINT & ERROR_OK &
 *                ANGLE_OK and now has it.
 * The call is idempotent: repeated with the same thresholds and scope it changes not one byte.  Under NULL params every trimmed
 * record has ERROR_OK | ANGLE_OK | DEPTH_OK.  Information is lost on purpose: a point without ANGLE_OK that the triangulation kept as
 * a diagnostic record is removed by the angle rule.  A later msfm_refine_points / msfm_refine_poses / msfm_extend_points treats
 * MSFM_TRI_FILTERED as it treats MSFM_TRI_EXTENDED when it rewrites a record.
 * The call invalidates registrations and pose-refinement records like msfm_refine_points; points, inlier bytes and the pose list stay
 * valid.  Errors, after each of which the session is exactly what it was: MSFM_E_STATE -- as msfm_refine_points.  MSFM_E_INVALID -- a
 * non-finite or negative max_error or min_angle, n_images < 0 or a NULL list with n_images > 0, an id that is not declared in the
 * session or given twice.  MSFM_E_NOIMAGE -- as msfm_refine_points.
 * The counters only count: no order reaches an output. */
enum { MSFM_TRI_FILTERED = 512 };
typedef struct msfm_filter_params {   /* 16 bytes, no implicit padding */
    double max_error;                /* pixels */
    double min_angle;                /* degrees */
} msfm_filter_params;
typedef struct msfm_filter_stats {   /* 88 bytes, no implicit padding */
    int64_t eligible;                /* consistent tracks with ATTEMPTED | POINT in scope */
    int64_t dropped_by_depth;        /* fitting observations of eligible tracks behind their camera */
    int64_t dropped_by_error;        /* ... in front of it with an error that is not <= max_error */
    int64_t trimmed;                 /* eligible tracks that lost an observation and stand */
    int64_t regained;                /* ... of which gain POINT & ERROR_OK & ANGLE_OK */
    int64_t removed_by_views;        /* eligible tracks left with fewer than two observations */
    int64_t removed_by_angle;        /* ... with two or more and no pair that reaches min_angle */
    int64_t succeeded;               /* POINT & ERROR_OK & ANGLE_OK over all tracks after the call */
    int64_t observations_used;       /* n_views summed over all tracks after the call */
    double filter_ms;                /* HIP events around all launches of the call */
    double prepare_ms;               /* ... of which the pose table, the inlier bytes and the per-observation array */
} msfm_filter_stats;
int msfm_filter_points(msfm_ctx* ctx, const msfm_filter_params* params, const int32_t* image_ids, int n_images,
                       msfm_filter_stats* stats);

/* ---- map completion: re-admit observations that fit again (opt-in) ---------------
 * The step the reference runs behind its filter after every local adjustment (MapBuilder::CompleteTracks -> Map::CompletePoints3D /
 * CompletePoint3D).  An observation that msfm_extend_points, msfm_triangulate_tracks_robust or msfm_filter_points rejected keeps
 * inlier byte 0 whatever the refinements do to its pose and its point afterwards; msfm_complete_points tests such observations of the
 * standing points again and re-admits those that fit: the only call that sets an inlier byte of an existing point back to 1.  No X
 * and no pose ever changes.  The arithmetic is csrc/msfm_complete.h, bit-identical to the host twin CompletePoints (DESIGN.md section
 * 23).  The tracks are whole connected components of the match graph, so the reference's walk over further correspondences has
 * nothing to discover and its MergeTracks has no counterpart: two tracks never share a correspondence.
 *   inputs       none besides the context, the threshold and the scope: as msfm_filter_points.
 *   threshold    max_error in pixels.  params NULL = the SESSION's own max_error.  An explicit value may be tighter than the
 *                session's, not looser: an observation admitted above it would clear ERROR_OK of the point it joins when the record
 *                is evaluated again (the reference's 4 px completion threshold sits beside a 4 px filter and no such bit).
 *   inlier bytes as msfm_filter_points: a session without them gets them first, 1 on every used observation of an attempted track,
 *                else 0.  On such a session there is no candidate and the call's only effect is that the bytes exist.
 *   candidate    a used observation (its image has a valid pose) whose inlier byte is 0.  n_images == 0: every image.  Otherwise
 *                only the candidates IN a listed image -- unlike msfm_filter_points, whose list selects tracks by where their
 *                fitting observations lie: "image 7's pose has just been refined: test what image 7 had rejected".  A listed image
 *                without a valid pose selects nothing.
 *   eligible     a consistent track whose record has POINT & ERROR_OK & ANGLE_OK.  Every other track stays bit for bit: a point
 *                that does not stand is filtered or extended, not completed.
 *   admission    per candidate, in element order: err = the reprojection error at the record's X under the current pose (pixels, f =
 *                (fx + fy) / 2).  Rejected by depth iff its depth is not > DBL_EPSILON; otherwise rejected by error iff !(err <=
 *                max_error) (a NaN is rejected); otherwise admitted: its inlier byte becomes 1.  X does not move, so candidates do
 *                not depend on each other and one pass is a fixed point.
 *   untouched    nothing admitted: not one byte is written, the residual slots of the rejected candidates included.
 *   completed    something admitted.  The record is evaluated again over the enlarged fitting set K at the unchanged X with the
 *                SESSION's thresholds and the triangulation's code: an error for every used observation, n_views = |K|,
 *                mean_residual = the errors of K summed in element order / |K|, tri_angle, ERROR_OK, ANGLE_OK, DEPTH_OK over K;
 *                status = ATTEMPTED | POINT | those bits | the record's ROBUST, REFINED, REPOSED, EXTENDED, FILTERED |
 *                MSFM_TRI_COMPLETED.
 * The call is idempotent: repeated with the same threshold and scope it changes not one byte and admits nothing.  Inlier bytes only
 * rise.  A later msfm_refine_points / msfm_refine_poses / msfm_extend_points / msfm_filter_points treats MSFM_TRI_COMPLETED as it
 * treats MSFM_TRI_FILTERED when it rewrites a record.
 * The call invalidates registrations and pose-refinement records like msfm_filter_points; points, inlier bytes and the pose list stay
 * valid.  Errors, after each of which the session is exactly what it was: MSFM_E_STATE -- as msfm_refine_points.  MSFM_E_INVALID -- a
 * non-finite or negative max_error or one above the session's, n_images < 0 or a NULL list with n_images > 0, an id that is not
 * declared in the session or given twice.  MSFM_E_NOIMAGE -- as msfm_refine_points.
 * The counters only count: no order reaches an output. */
enum { MSFM_TRI_COMPLETED = 1024 };
typedef struct msfm_complete_params {   /* 8 bytes, no implicit padding */
    double max_error;                /* pixels; not above the session's */
} msfm_complete_params;
typedef struct msfm_complete_stats {   /* 80 bytes, no implicit padding */
    int64_t eligible;                /* consistent tracks with POINT & ERROR_OK & ANGLE_OK */
    int64_t candidates;              /* their used observations with inlier byte 0 in scope: tested */
    int64_t admitted;                /* ... in front of their camera with an error <= max_error */
    int64_t rejected_by_depth;       /* ... behind their camera */
    int64_t rejected_by_error;       /* ... in front of it with an error that is not <= max_error */
    int64_t completed;               /* eligible tracks that admitted an observation */
    int64_t succeeded;               /* POINT & ERROR_OK & ANGLE_OK over all tracks after the call */
    int64_t observations_used;       /* n_views summed over all tracks after the call */
    double complete_ms;              /* HIP events around all launches of the call */
    double prepare_ms;               /* ... of which the pose table, the inlier bytes and the per-observation array */
} msfm_complete_stats;
int msfm_complete_points(msfm_ctx* ctx, const msfm_complete_params* params, const int32_t* image_ids, int n_images,
                         msfm_complete_stats* stats);

/* ---- map visibility: covisibility counts for the builder's decisions (opt-in, read-only) ---------------
 * The one quantity the reference's MapBuilder derives its decisions from: how many tracks or points two images share.  Where to start
 * (TryInitialize: FindFirstInitialImage orders images by their correspondences, FindSecondInitialImage by those shared with the
 * first), which image next (Map::GetNextImageIds: unregistered images by how much of the map they see), what to adjust
 * (Map::GetLocalBAData: the new image and its most covisible neighbours).  msfm_map_visibility counts all of it on the device from
 * the track CSR, the records' status words and the inlier bytes; nothing is fetched to the host but the counts.  Integer counting:
 * every output is a sum of ones, identical to the host twin MapVisibility (csrc/msfm_visibility.h).
 * Let n be the number of images declared in the session, in rank order (ascending id).
 *   standing track   basis MSFM_VIS_TRACKS: every kept consistent track of the last msfm_tracks_finish -- no points are needed, the
 *                    call works right after msfm_tracks_finish.  Basis MSFM_VIS_MAP: a kept consistent track whose record has POINT &
 *                    ERROR_OK & ANGLE_OK, the test msfm_complete_points and msfm_register_images use.  Inconsistent tracks kept by
 *                    keep_inconsistent never count.
 *   counting element of a standing track.  TRACKS: every element.  MAP, image without a valid pose in the session's pose list (listed
 *                    without one or not listed at all): every element -- a correspondence a registration would use.  MAP, image with
 *                    a valid pose: iff its observation is fitting -- inlier byte 1 where the session has bytes, otherwise every
 *                    used observation.
 *   per image I      n_elements: elements of kept consistent tracks in I, the same under both bases.  n_visible: elements of
 *                    standing tracks in I, counting or not.  n_points: counting elements in I if I is posed, else 0 (TRACKS: 0).
 *                    flags: MSFM_VIS_POSED iff I has a valid pose (MAP only), MSFM_VIS_QUERIED iff I is in the list.
 *   matrix           out_covisible[r * n + j]: the standing tracks in which the r-th query image and the image of rank j both have a
 *                    counting element; at the query image's own rank, its number of counting elements.
 *   stats            tracks_counted: standing tracks.  elements_counted: all counting elements.  pair_increments: the sum of the
 *                    matrix.  route: the one that ran.  device_bytes: the peak of the call's temporaries, all freed on return.
 *   route            MSFM_VIS_ROUTE_GLOBAL: agent-scope adds in global memory.  MSFM_VIS_ROUTE_LDS: the per-image counters, and the
 *                    matrix rows where they fit, are privatised per workgroup in LDS and flushed once.  MSFM_VIS_ROUTE_AUTO picks
 *                    (msfm_vis::vis_route).  All give the same counts.
 * params NULL = {MSFM_VIS_MAP, MSFM_VIS_ROUTE_AUTO}.  out_images (n records) and out_covisible (n_query x n, row-major) may be NULL.
 * The call is READ-ONLY: not one byte of the session changes -- points, residuals, inlier bytes and the pose list stay as they are, the
 * registrations and the pose-refinement records stay valid, and a session without inlier bytes still has none.  It may run between
 * msfm_register_images and msfm_fetch_registrations.
 * Errors, after each of which the session is what it was: MSFM_E_STATE -- no finished track session, basis MAP without valid points,
 * a streaming series open.  MSFM_E_INVALID -- an unknown basis or route, n_query < 0 or a NULL list with n_query > 0, an id that is not
 * declared in the session or given twice, MSFM_VIS_ROUTE_LDS at a shape whose per-image counters do not fit one workgroup's LDS. */
enum { MSFM_VIS_TRACKS = 0, MSFM_VIS_MAP = 1 };                                            /* basis */
enum { MSFM_VIS_ROUTE_AUTO = 0, MSFM_VIS_ROUTE_GLOBAL = 1, MSFM_VIS_ROUTE_LDS = 2 };
enum { MSFM_VIS_POSED = 1, MSFM_VIS_QUERIED = 2 };                                         /* record flags */
typedef struct msfm_visibility_params {   /* 8 bytes, no implicit padding */
    int32_t basis;
    int32_t route;
} msfm_visibility_params;
typedef struct msfm_image_visibility {   /* 24 bytes, no implicit padding */
    int32_t image_id;
    int32_t flags;
    int32_t n_elements;
    int32_t n_visible;
    int32_t n_points;
    int32_t reserved;
} msfm_image_visibility;
typedef struct msfm_visibility_stats {   /* 56 bytes, no implicit padding */
    int64_t tracks_counted;
    int64_t elements_counted;
    int64_t pair_increments;
    int64_t device_bytes;
    int32_t images;                  /* n */
    int32_t posed;                   /* images with a valid pose (MAP) */
    int32_t query;                   /* n_query */
    int32_t route;                   /* the one that ran */
    double visibility_ms;            /* HIP events around the launches */
} msfm_visibility_stats;
int msfm_map_visibility(msfm_ctx* ctx, const msfm_visibility_params* params, const int32_t* query_ids, int n_query,
                        msfm_image_visibility* out_images, uint32_t* out_covisible, msfm_visibility_stats* stats);

/* ---- map alignment: a robust similarity to known camera positions, and the edit that applies one (opt-in) ---------------
 * A map lives in the gauge of its initial pair: the first image at the identity, a baseline of length 1, an arbitrary orientation.
 * Captures with position priors (a rig, an INS, an earlier reconstruction) want it in the priors' frame and units, the step every SfM
 * tool has (COLMAP's model_aligner, OpenSfM's align).  msfm_estimate_alignment finds the similarity from the session's camera centres
 * to the caller's positions; msfm_transform_map moves every pose and every point by a similarity, that one or any other (a
 * normalisation).  The arithmetic is csrc/msfm_align.h, bit-identical to the host twins EstimateAlignment / TransformMap (DESIGN.md
 * section 28).
 *   similarity   world' = s Q X + d: s > 0, Q row-major and a proper rotation.
 *   priors       positions[3 k ..] is the position of image_ids[k].  A listed image without a valid pose in the session is reported as
 *                not used and is no error: callers pass the priors of all images.  m: the usable ones, in list order.  ATTEMPTED iff
 *                m >= 3.
 *   fit          Umeyama's closed form over pairs (camera centre, position): one 3 x 3 decomposition.  Valid iff every number is finite,
 *                the centres are not all one point, s > 0 and the second singular value is above 1e-6 of the first (centres on a line
 *                leave the rotation about it free).
 *   error        of a prior: |position - (s Q centre + d)|, in the prior's units; an inlier iff error <= max_error.
 *   robust       hypotheses it = 0 .. : the fit of three distinct priors from the counter stream keyed by `it`, counted by its
 *                inliers among all m; the sequential adaptive rule (w^3, confidence) over at most max_hypotheses hypotheses, scored in
 *                rounds of 256; the winner is the lowest iteration among the largest count (MODEL).  Then at most four refits over the
 *                current inlier set, each standing (REFIT) iff it is valid and has at least as many inliers.  SUCCEEDED iff the final
 *                model has at least max(3, min_inliers) inliers.
 *   least squares max_hypotheses == 0 (and params NULL): one fit of all m priors (LEAST_SQUARES); every usable prior is reported as an
 *                inlier, max_error is not read.
 *   record       hypotheses: those the stopping rule evaluated (at most max_hypotheses); refits: those that stood; rms over the
 *                inliers.  A failed estimate is MSFM_OK with SUCCEEDED clear, an all-zero similarity and error -1.0 on every prior.
 *   per prior    out_per_prior[k] (may be NULL), in list order: MSFM_ALN_USED, MSFM_ALN_INLIER and the error under the final model
 *                (-1.0 when not used or when the estimate failed).
 * msfm_estimate_alignment is READ-ONLY like msfm_map_visibility: not one byte of the session changes and no validity flag drops; it may
 * run between msfm_register_images and msfm_fetch_registrations.  Errors: MSFM_E_STATE -- as msfm_refine_points.  MSFM_E_INVALID -- n < 0
 * or a NULL list with n > 0, NULL out, an id that is not declared in the session or given twice, a non-finite position, max_hypotheses
 * outside 0 .. 4096, a robust call whose max_error is not finite and positive, confidence outside (0, 1).
 *
 * msfm_transform_map EDITS the map.  Every valid pose becomes R' = R Q^T, t' = s t - R' d (the camera frame is scaled by s: depths
 * scale, projections do not change; R is not re-orthogonalised).  Every record with ATTEMPTED | POINT gets X' = s (Q X) + d and is
 * evaluated again at X' under the new poses with the session's camera and thresholds, as msfm_refine_camera's re-verdict does: the
 * residual slots of its used observations, mean_residual, tri_angle and the three verdict bits are rewritten, n_views and the inlier
 * bytes are kept; status = ATTEMPTED | POINT | those bits | the record's ROBUST .. COMPLETED bits | MSFM_TRI_ALIGNED.  A non-finite X'
 * (only an overflow gives one) leaves ATTEMPTED | those kept bits | ALIGNED, every other field 0 and every residual slot of the track
 * -1.0: the shape msfm_filter_points gives a removed point; it counts in points_lost.  The identity leaves every X and every pose bit
 * for bit.  MSFM_TRI_ALIGNED needs no rule in any other call: every call that rewrites a record builds its status from an explicit
 * mask of the bits it keeps and thereby clears it (as it clears MSFM_TRI_RECALIBRATED, which this call clears too).
 * The call invalidates registrations and pose-refinement records as every edit does -- they hold poses of the old frame -- and replaces
 * the session's pose list; points, inlier bytes and camera stay valid.  Errors, after each of which the session is exactly what it
 * was: MSFM_E_STATE -- as msfm_refine_points.  MSFM_E_INVALID -- NULL similarity, s not finite and positive, d not finite,
 * max |Q Q^T - I| > 1e-9 or det Q <= 0, a new pose that would not be finite.  MSFM_E_NOIMAGE -- as msfm_refine_points. */
enum { MSFM_TRI_ALIGNED = 4096 };
enum { MSFM_ALN_ATTEMPTED = 1, MSFM_ALN_MODEL = 2, MSFM_ALN_SUCCEEDED = 4, MSFM_ALN_REFIT = 8, MSFM_ALN_LEAST_SQUARES = 16 };   /* status */
enum { MSFM_ALN_USED = 1, MSFM_ALN_INLIER = 2 };                                                                                /* per prior */
typedef struct msfm_similarity {   /* 104 bytes, no implicit padding */
    double s;
    double Q[9];                     /* row-major */
    double d[3];
} msfm_similarity;
typedef struct msfm_alignment_params {   /* 24 bytes, no implicit padding */
    double max_error;                /* the prior's units; not read when max_hypotheses == 0 */
    double confidence;               /* 0.9999 */
    int32_t max_hypotheses;          /* 1024; 0 .. 4096, 0 = least squares */
    int32_t min_inliers;             /* 3 */
} msfm_alignment_params;
typedef struct msfm_alignment {   /* 144 bytes, no implicit padding */
    int32_t status;                  /* MSFM_ALN_* */
    int32_t n_listed;                /* n */
    int32_t n_used;                  /* m: listed images with a valid pose */
    int32_t n_inliers;
    int32_t hypotheses;              /* evaluated by the stopping rule */
    int32_t refits;                  /* that stood */
    msfm_similarity similarity;      /* all zero unless SUCCEEDED */
    double rms;                      /* over the inliers */
    double estimate_ms;              /* HIP events around the launch */
} msfm_alignment;
typedef struct msfm_alignment_residual {   /* 16 bytes, no implicit padding */
    int32_t flags;                   /* MSFM_ALN_USED | MSFM_ALN_INLIER */
    int32_t reserved;
    double error;                    /* -1.0 when not used */
} msfm_alignment_residual;
typedef struct msfm_transform_stats {   /* 48 bytes, no implicit padding */
    int64_t poses_transformed;       /* valid poses of the session's list */
    int64_t points_transformed;      /* records with ATTEMPTED | POINT */
    int64_t points_lost;             /* ... that had POINT & ERROR_OK & ANGLE_OK and no longer have it */
    int64_t points_gained;           /* ... that did not have it and now do */
    int64_t succeeded;               /* POINT & ERROR_OK & ANGLE_OK over all tracks after the call */
    double transform_ms;             /* HIP events around all launches of the call */
} msfm_transform_stats;
int msfm_estimate_alignment(msfm_ctx* ctx, const int32_t* image_ids, const double* positions, int n, const msfm_alignment_params* params,
                            msfm_alignment* out, msfm_alignment_residual* out_per_prior);
int msfm_transform_map(msfm_ctx* ctx, const msfm_similarity* similarity, msfm_transform_stats* stats);

/* ---- image registration: absolute pose from the triangulated tracks (opt-in) ---------------
 * The reference's MapBuilder::TryRegisterNextImage -> Registrant::Register (src/Reconstruction/Registrant.cpp) for every listed
 * image at once: the 2D-3D correspondences an image has with the points of the last msfm_triangulate_tracks, P3P RANSAC, a
 * Gauss-Newton refinement of the winner.  The arithmetic is csrc/msfm_register.h, shared with the host twin:
 *   correspondences of image I   every kept track whose record has POINT & ERROR_OK & ANGLE_OK and which has an element (I, k), by
 *               ascending track number; 2D: the keypoint pixel through the camera to normalised undistorted (u, v); 3D: the record's
 *               X.  n of them.  ATTEMPTED iff n >= 3 and n >= min_inliers.
 *   hypothesis  it = 0 .. : three distinct correspondences from the counter stream keyed by (image id, it), Grunert's P3P (up to 4
 *               poses), scored by  Y = R X + t,  inlier iff Y.z > eps and |(Y.x / Y.z, Y.y / Y.z) - (u, v)|^2 f^2 <= max_error^2,
 *               f = (fx + fy) / 2; the hypothesis counts the best of its poses.
 *   stopping    the sequential adaptive rule (w^3, confidence) over at most max_iters hypotheses, run in rounds of 64; the winner is
 *               the lowest iteration among the largest count; POSE iff it has >= 3 inliers.
 *   refinement  refine_iters Gauss-Newton steps on the winner's inliers (0: none); the refined pose stands (REFINED) iff it has at
 *               least the winner's number of inliers.  SUCCEEDED iff n_inliers >= min_inliers (the reference's is_succeed).
 *   record      hypotheses: the hypotheses scored for the image (whole rounds, at most max_iters); R, t: x_cam = R X + t (0 without
 *               POSE); mean_residual: mean pixel error of the inliers.  Per correspondence: the track number, the inlier flag and the
 *               pixel error under the final pose (all correspondences; 0 / -1.0 without POSE).
 * Images that already have a pose may be listed: they are localised again, from the points alone.  The tracks, the points and every
 * match list are untouched.  params NULL = {4.0 px, 0.9999, 1024, 15, 10} (Registrant.h:22-26; max_iters is this library's).
 * Errors: MSFM_E_STATE -- no track session, no points (msfm_triangulate_tracks has not run since the last msfm_tracks_finish), a
 * streaming series open; msfm_fetch_registrations without a successful msfm_register_images since then.  MSFM_E_NOIMAGE -- a listed
 * image that is not declared in the session or has no keypoints (msfm_upload_keypoints).  MSFM_E_INVALID -- NULL or bad camera, an id
 * given twice, n_images < 0, non-finite or negative max_error, confidence outside (0, 1), max_iters outside 1 .. 65536, min_inliers
 * < 0, refine_iters outside 0 .. 100.  The results live in the session (counted in msfm_register_stats::device_bytes); a later
 * msfm_tracks_finish or msfm_triangulate_tracks invalidates them, msfm_tracks_end frees them.
 * msfm_fetch_registrations: n_images records in the order of the list, n_images + 1 offsets, then offsets[n_images] track numbers,
 * flags and errors; any pointer may be NULL. */
enum { MSFM_REG_ATTEMPTED = 1, MSFM_REG_POSE = 2, MSFM_REG_SUCCEEDED = 4, MSFM_REG_REFINED = 8 };
typedef struct msfm_register_params {   /* 32 bytes, no implicit padding */
    double max_error;
    double confidence;
    int32_t max_iters;
    int32_t min_inliers;
    int32_t refine_iters;
    int32_t reserved;
} msfm_register_params;
typedef struct msfm_registration {   /* 128 bytes, no implicit padding */
    int32_t image_id;
    int32_t status;
    int32_t n_correspondences;
    int32_t n_inliers;
    int32_t hypotheses;
    int32_t reserved;
    double R[9];
    double t[3];
    double mean_residual;
} msfm_registration;
typedef struct msfm_register_stats {   /* 48 bytes, no implicit padding */
    int32_t images;
    int32_t attempted;
    int32_t succeeded;
    int32_t rounds;              /* rounds any image ran */
    int64_t correspondences;
    int64_t hypotheses;          /* hypotheses solved */
    int64_t device_bytes;        /* the results held by the session */
    double register_ms;          /* HIP events around the launches */
} msfm_register_stats;
int msfm_register_images(msfm_ctx* ctx, const msfm_camera* camera, const int32_t* image_ids, int n_images,
                         const msfm_register_params* params, msfm_register_stats* stats);
int msfm_fetch_registrations(msfm_ctx* ctx, msfm_registration* out, int64_t* out_offsets, int32_t* out_track_ids, uint8_t* out_inlier,
                             double* out_residuals);

/* ---- host-side helpers (no device work) ------------------------------------------------- */
/* FeatureUtils::ExtractTopScaleDescriptors' row selection (FeatureUtils.cpp:68-96):
 * kpts = n x 4 float (x, y, size, angle); writes min(k, n) indices, k > n => identity.
 * Tie rule (reference: unspecified, std::partial_sort): size descending, index ascending. */
int msfm_topscale_select(const float* kpts, int n, int k, int32_t* out_idx, int* out_count);
/* Database::ImagePairToPairId / PairIdToImagePair / SwapImagePair (Database.cpp:656-694) */
int msfm_pair_id(int id1, int id2, int32_t* out_pair_id);
int msfm_pair_from_id(int32_t pair_id, int* out_id1, int* out_id2);
int msfm_swap_image_pair(int id1, int id2);

const char* msfm_version(void);
/* gfx950 devices this process can open with msfm_create (ordinals 0 .. n-1); 0 without a GPU.  The reference is single-device;
 * the drop-in's node-level fan-out (MSFM_DEVICES=all in host/FeatureMatching.cpp) asks it how many contexts to create. */
int msfm_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
