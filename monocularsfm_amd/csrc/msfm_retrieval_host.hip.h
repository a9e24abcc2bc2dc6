// msfm_retrieval_host.hip.h -- host side of vocabulary retrieval (matching mode 2) behind the C ABI entry points of include/msfm_match.h
// "vocabulary retrieval" (defined in msfm_match.hip), around the kernels of msfm_retrieval.hip.h.  Included by msfm_match.hip.
#pragma once

namespace {

constexpr int kRetDefaultWords = 16384, kRetMaxWords = 65536, kRetDefaultIters = 8;
constexpr long long kRetMaxTrainRows = 1LL << 24;   // q sums of one word and dimension stay below 2^32

// Scratch of one retrieval call: freed when the call returns, whatever it returns
struct RetScratch {
    DevBuf segs, tiles, gsegs, prefix, sample, assign, sums, cnt, changed, hist, idf, norm, score, ids, tile_ij, keys, counts;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~RetScratch() {
        DevBuf* all[] = {&segs, &tiles, &gsegs, &prefix, &sample, &assign, &sums, &cnt, &changed, &hist, &idf, &norm, &score, &ids, &tile_ij, &keys, &counts};
        for (DevBuf* b : all) b->release();
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

inline int ret_vpad(int v) { return (v + kRetWordTile - 1) / kRetWordTile * kRetWordTile; }

// The call's images by ascending id, each as a segment of quantised rows (empty images have none); the row prefix of every image.
struct RetImages {
    std::vector<int> ids;               // ascending
    std::vector<RetSeg> segs;           // non-empty images
    std::vector<long long> seg_prefix;  // first row of every segment
    std::vector<long long> img_prefix;  // first row of every image (ids order)
    long long rows = 0;
};

int ret_segment(msfm_ctx* ctx, int id, long long out, RetSeg* seg) {
    const Image& im = ctx->images[(size_t)id];
    *seg = RetSeg{nullptr, 0, 0, im.n, out};
    if (im.n == 0) return MSFM_OK;
    if (im.ret_int && im.is_u8 && im.i8) {
        *seg = RetSeg{im.i8, kRetI8Rows, kI8RowBytes, im.n, out};
    } else if ((im.ret_int || im.ret_unit) && im.rawp) {
        *seg = RetSeg{im.rawp, im.ret_int ? kRetInt : kRetUnit, kDim * 4, im.n, out};
    } else {
        return fail(ctx, MSFM_E_INVALID, "vocabulary retrieval: image " + std::to_string(id) +
                                             " has values that are neither all integers in [0, 255] nor all in [0, 1]");
    }
    return MSFM_OK;
}

int ret_collect(msfm_ctx* ctx, const int32_t* ids, int n, RetImages& out) {
    if (n < 0 || n > MSFM_MAX_IMAGES || (n > 0 && !ids)) return fail(ctx, MSFM_E_INVALID, "vocabulary retrieval: bad image list");
    if (ctx->series_open) return fail(ctx, MSFM_E_STATE, "vocabulary retrieval while a streaming series (msfm_match_pairs_begin .. _next) is open");
    out.ids.assign(ids, ids + n);
    std::sort(out.ids.begin(), out.ids.end());
    for (int k = 0; k < n; ++k) {
        const int id = out.ids[(size_t)k];
        if (id < 0 || id >= (int)ctx->images.size() || ctx->images[(size_t)id].n < 0)
            return fail(ctx, MSFM_E_INVALID, "vocabulary retrieval: image not resident: " + std::to_string(id));
        if (k && out.ids[(size_t)k - 1] == id) return fail(ctx, MSFM_E_INVALID, "vocabulary retrieval: image listed twice: " + std::to_string(id));
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = settle_store(ctx);   // a pending store build first, as every matching call does
    if (rc != MSFM_OK) return rc;
    for (int id : out.ids) {
        RetSeg s;
        const int rc2 = ret_segment(ctx, id, out.rows, &s);
        if (rc2 != MSFM_OK) return rc2;
        out.img_prefix.push_back(out.rows);
        if (s.n > 0) {
            out.segs.push_back(s);
            out.seg_prefix.push_back(out.rows);
        }
        out.rows += ctx->images[(size_t)id].n;
    }
    return MSFM_OK;
}

template <class T>
int ret_upload(msfm_ctx* ctx, DevBuf& b, const std::vector<T>& v) {
    HIPCHK(ctx, b.ensure(std::max<size_t>(1, v.size()) * sizeof(T)));
    if (!v.empty()) HIPCHK(ctx, hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return MSFM_OK;
}

// the nearest resident word of every row of `segs` into out[seg.out + row]
int ret_assign(msfm_ctx* ctx, RetScratch& rs, const std::vector<RetSeg>& segs, int* out) {
    std::vector<RetTile> tiles;
    for (size_t k = 0; k < segs.size(); ++k)
        for (int r = 0; r < segs[k].n; r += kRetWgRows) tiles.push_back(RetTile{(int)k, r});
    if (tiles.empty()) return MSFM_OK;
    int rc = ret_upload(ctx, rs.segs, segs);
    if (rc == MSFM_OK) rc = ret_upload(ctx, rs.tiles, tiles);
    if (rc != MSFM_OK) return rc;
    hipLaunchKernelGGL(ret_assign_kernel, dim3((unsigned)tiles.size()), dim3(256), 0, store_stream(ctx), rs.segs.as<RetSeg>(),
                       rs.tiles.as<RetTile>(), ctx->ret_words.as<signed char>(), ctx->ret_cn.as<unsigned>(), ret_vpad(ctx->ret_v), out);
    HIPCHK(ctx, hipGetLastError());
    return MSFM_OK;
}

int ret_norms(msfm_ctx* ctx) {
    const int vpad = ret_vpad(ctx->ret_v);
    hipLaunchKernelGGL(ret_norms_kernel, dim3((unsigned)((vpad + 255) / 256)), dim3(256), 0, store_stream(ctx), ctx->ret_words.as<signed char>(),
                       ctx->ret_v, vpad, ctx->ret_cn.as<unsigned>());
    HIPCHK(ctx, hipGetLastError());
    return MSFM_OK;
}

// room for a vocabulary of v words: zero padding rows (they never win, ret_norms_kernel)
int ret_alloc_vocab(msfm_ctx* ctx, int v) {
    const int vpad = ret_vpad(v);
    ctx->ret_v = 0;
    HIPCHK(ctx, ctx->ret_words.ensure((size_t)vpad * kDim));
    HIPCHK(ctx, ctx->ret_cn.ensure((size_t)vpad * 4));
    HIPCHK(ctx, hipMemsetAsync(ctx->ret_words.p, 0, (size_t)vpad * kDim, store_stream(ctx)));
    return MSFM_OK;
}

float ret_elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

int train_impl(msfm_ctx* ctx, const int32_t* ids, int n, const msfm_retrieval_params* params, uint8_t* out_words, int* out_num_words) {
    msfm_retrieval_params p = {0, 0, 0};
    if (params) p = *params;
    if (p.num_words < 0 || p.num_words > kRetMaxWords || p.train_iters < 0 || p.train_rows < 0 || p.train_rows > kRetMaxTrainRows)
        return fail(ctx, MSFM_E_INVALID, "msfm_train_vocabulary: bad parameters");
    const int V = p.num_words ? p.num_words : kRetDefaultWords;
    const int T = p.train_iters ? p.train_iters : kRetDefaultIters;
    const long long M = p.train_rows ? p.train_rows : std::min<long long>(64LL * V, kRetMaxTrainRows);
    RetImages im;
    int rc = ret_collect(ctx, ids, n, im);
    if (rc != MSFM_OK) return rc;
    const MsfmRetSample smp = msfm_ret_sample(im.rows, M);
    if (smp.count == 0) return fail(ctx, MSFM_E_INVALID, "msfm_train_vocabulary: the images hold no rows");
    const int vp = msfm_ret_vocab_size(V, smp.count);
    RetScratch rs;
    hipStream_t st = store_stream(ctx);
    for (hipEvent_t& e : rs.ev) HIPCHK(ctx, hipEventCreate(&e));
    HIPCHK(ctx, hipEventRecord(rs.ev[0], st));
    // the sample, contiguous q' rows (its own segment table: ret_assign rewrites rs.segs while the gather may still run)
    rc = ret_upload(ctx, rs.gsegs, im.segs);
    if (rc == MSFM_OK) rc = ret_upload(ctx, rs.prefix, im.seg_prefix);
    if (rc != MSFM_OK) return rc;
    HIPCHK(ctx, rs.sample.ensure((size_t)smp.count * kDim));
    hipLaunchKernelGGL(ret_gather_kernel, dim3((unsigned)((smp.count * 8 + 255) / 256)), dim3(256), 0, st, rs.gsegs.as<RetSeg>(),
                       rs.prefix.as<long long>(), (int)im.segs.size(), smp.step, smp.count, rs.sample.as<signed char>());
    HIPCHK(ctx, hipGetLastError());
    rc = ret_alloc_vocab(ctx, vp);
    if (rc != MSFM_OK) return rc;
    // a training that fails from here on leaves no vocabulary behind
    struct Unset {
        msfm_ctx* c;
        bool keep = false;
        ~Unset() {
            if (!keep) c->ret_v = 0;
        }
    } unset{ctx};
    hipLaunchKernelGGL(ret_init_kernel, dim3((unsigned)((vp * 8 + 255) / 256)), dim3(256), 0, st, rs.sample.as<signed char>(), smp.count, vp,
                       ctx->ret_words.as<signed char>());
    HIPCHK(ctx, hipGetLastError());
    ctx->ret_v = vp;
    const std::vector<RetSeg> sseg = {RetSeg{rs.sample.p, kRetI8Rows, kDim, (int)smp.count, 0}};
    HIPCHK(ctx, rs.assign.ensure((size_t)smp.count * 4));
    HIPCHK(ctx, rs.sums.ensure((size_t)vp * kDim * 4));
    HIPCHK(ctx, rs.cnt.ensure((size_t)vp * 4));
    HIPCHK(ctx, rs.changed.ensure(4));
    int iters = 0;
    for (; iters < T;) {
        rc = ret_norms(ctx);
        if (rc == MSFM_OK) rc = ret_assign(ctx, rs, sseg, rs.assign.as<int>());
        if (rc != MSFM_OK) return rc;
        HIPCHK(ctx, hipMemsetAsync(rs.sums.p, 0, (size_t)vp * kDim * 4, st));
        HIPCHK(ctx, hipMemsetAsync(rs.cnt.p, 0, (size_t)vp * 4, st));
        HIPCHK(ctx, hipMemsetAsync(rs.changed.p, 0, 4, st));
        hipLaunchKernelGGL(ret_accum_kernel, dim3((unsigned)((smp.count * kDim + 255) / 256)), dim3(256), 0, st, rs.sample.as<signed char>(),
                           rs.assign.as<int>(), smp.count, rs.sums.as<unsigned>(), rs.cnt.as<unsigned>());
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(ret_update_kernel, dim3((unsigned)((vp * kDim + 255) / 256)), dim3(256), 0, st, rs.sums.as<unsigned>(),
                           rs.cnt.as<unsigned>(), vp, ctx->ret_words.as<signed char>(), rs.changed.as<int>());
        HIPCHK(ctx, hipGetLastError());
        ++iters;
        int changed = 0;
        HIPCHK(ctx, hipMemcpyAsync(&changed, rs.changed.p, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (!changed) break;   // a fixed point: further iterations change nothing
    }
    rc = ret_norms(ctx);
    if (rc != MSFM_OK) return rc;
    HIPCHK(ctx, hipEventRecord(rs.ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->ret_prof.train_ms = ret_elapsed(rs.ev[0], rs.ev[1]);
    ctx->ret_prof.train_iterations = iters;
    ctx->ret_prof.num_words = vp;
    if (out_words) {
        HIPCHK(ctx, hipMemcpy(out_words, ctx->ret_words.p, (size_t)vp * kDim, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < (size_t)vp * kDim; ++k) out_words[k] ^= 0x80;   // c = c' + 128
    }
    if (out_num_words) *out_num_words = vp;
    unset.keep = true;
    return MSFM_OK;
}

int retrieve_impl(msfm_ctx* ctx, const int32_t* ids, int n, int k, int32_t* out_pairs, float* out_scores, int* out_n_pairs,
                  float* out_matrix) {
    if (!out_n_pairs || (n > 0 && !out_pairs)) return fail(ctx, MSFM_E_INVALID, "msfm_retrieve_pairs: null output");
    if (k < 1 || k > kRetMaxK) return fail(ctx, MSFM_E_INVALID, "msfm_retrieve_pairs: num_nearest must lie in 1 .. 1024");
    if (!ctx->ret_v) return fail(ctx, MSFM_E_STATE, "msfm_retrieve_pairs without a vocabulary (msfm_train_vocabulary / msfm_set_vocabulary)");
    *out_n_pairs = 0;
    RetImages im;
    int rc = ret_collect(ctx, ids, n, im);
    if (rc != MSFM_OK) return rc;
    if (n == 0) return MSFM_OK;
    const int vpad = ret_vpad(ctx->ret_v);
    RetScratch rs;
    hipStream_t st = store_stream(ctx);
    for (hipEvent_t& e : rs.ev) HIPCHK(ctx, hipEventCreate(&e));
    HIPCHK(ctx, rs.assign.ensure((size_t)std::max<long long>(1, im.rows) * 4));
    HIPCHK(ctx, hipEventRecord(rs.ev[0], st));
    rc = ret_assign(ctx, rs, im.segs, rs.assign.as<int>());
    if (rc != MSFM_OK) return rc;
    HIPCHK(ctx, hipEventRecord(rs.ev[1], st));
    // tf-idf vectors: counts, idf, norms, a_iw in place of the counts
    const size_t cells = (size_t)n * vpad;
    HIPCHK(ctx, rs.hist.ensure(cells * 4));
    HIPCHK(ctx, hipMemsetAsync(rs.hist.p, 0, cells * 4, st));
    rc = ret_upload(ctx, rs.prefix, im.img_prefix);
    if (rc != MSFM_OK) return rc;
    if (im.rows > 0) {
        hipLaunchKernelGGL(ret_hist_kernel, dim3((unsigned)((im.rows + 255) / 256)), dim3(256), 0, st, rs.assign.as<int>(), rs.prefix.as<long long>(), n,
                           im.rows, vpad, rs.hist.as<unsigned>());
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, rs.idf.ensure((size_t)vpad * 8));
    HIPCHK(ctx, rs.norm.ensure((size_t)n * 8));
    hipLaunchKernelGGL(ret_idf_kernel, dim3((unsigned)((vpad + 255) / 256)), dim3(256), 0, st, rs.hist.as<unsigned>(), n, vpad, rs.idf.as<double>());
    hipLaunchKernelGGL(ret_rownorm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, rs.hist.as<unsigned>(), rs.idf.as<double>(), n, vpad,
                       rs.norm.as<double>());
    hipLaunchKernelGGL(ret_normalize_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, rs.hist.as<unsigned>(), rs.idf.as<double>(),
                       rs.norm.as<double>(), n, vpad);
    HIPCHK(ctx, hipGetLastError());
    // S = A A^T on the tiles on and above the diagonal
    const int nt = (n + kRetScoreTile - 1) / kRetScoreTile;
    std::vector<int2> tij;
    for (int a = 0; a < nt; ++a)
        for (int b = a; b < nt; ++b) tij.push_back(make_int2(a, b));
    rc = ret_upload(ctx, rs.tile_ij, tij);
    if (rc != MSFM_OK) return rc;
    HIPCHK(ctx, rs.score.ensure((size_t)n * n * 4));
    hipLaunchKernelGGL(ret_score_kernel, dim3((unsigned)tij.size()), dim3(256), 0, st, rs.hist.as<float>(), n, vpad, rs.tile_ij.as<int2>(),
                       rs.score.as<float>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(rs.ev[2], st));
    // top-K of every image
    rc = ret_upload(ctx, rs.ids, im.ids);
    if (rc != MSFM_OK) return rc;
    HIPCHK(ctx, rs.keys.ensure((size_t)n * k * 8));
    HIPCHK(ctx, rs.counts.ensure((size_t)n * 4));
    hipLaunchKernelGGL(ret_topk_kernel, dim3((unsigned)n), dim3(256), 0, st, rs.score.as<float>(), rs.ids.as<int>(), n, k,
                       rs.keys.as<unsigned long long>(), rs.counts.as<int>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(rs.ev[3], st));
    std::vector<unsigned long long> keys((size_t)n * k);
    std::vector<int> counts((size_t)n);
    HIPCHK(ctx, hipMemcpyAsync(keys.data(), rs.keys.p, keys.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(counts.data(), rs.counts.p, counts.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->ret_prof.assign_ms = ret_elapsed(rs.ev[0], rs.ev[1]);
    ctx->ret_prof.score_ms = ret_elapsed(rs.ev[1], rs.ev[2]);
    ctx->ret_prof.topk_ms = ret_elapsed(rs.ev[2], rs.ev[3]);
    ctx->ret_prof.rows = im.rows;
    ctx->ret_prof.num_words = ctx->ret_v;
    // the union, in brute mode's orientation and order
    std::vector<std::pair<int, int>> sel;
    std::map<std::pair<int, int>, float> score_of;
    for (int i = 0; i < n; ++i)
        for (int t = 0; t < counts[(size_t)i] && t < k; ++t) {
            const unsigned long long key = keys[(size_t)i * k + t];
            const int j = msfm_ret_key_id(key);
            const unsigned bits = (unsigned)(key >> 32);
            float s;
            std::memcpy(&s, &bits, 4);
            sel.emplace_back(im.ids[(size_t)i], j);
            score_of[std::make_pair(std::max(im.ids[(size_t)i], j), std::min(im.ids[(size_t)i], j))] = s;
        }
    const std::vector<std::pair<int, int>> pairs = msfm_ret_union(sel);
    for (size_t t = 0; t < pairs.size(); ++t) {
        out_pairs[2 * t] = pairs[t].first;
        out_pairs[2 * t + 1] = pairs[t].second;
        if (out_scores) out_scores[t] = score_of[pairs[t]];
    }
    *out_n_pairs = (int)pairs.size();
    if (out_matrix) {
        // rows and columns in the caller's order of ids
        std::vector<float> s((size_t)n * n);
        HIPCHK(ctx, hipMemcpy(s.data(), rs.score.p, s.size() * 4, hipMemcpyDeviceToHost));
        std::vector<int> pos((size_t)n);
        for (int a = 0; a < n; ++a) pos[(size_t)a] = (int)(std::lower_bound(im.ids.begin(), im.ids.end(), ids[a]) - im.ids.begin());
        for (int a = 0; a < n; ++a)
            for (int b = 0; b < n; ++b) out_matrix[(size_t)a * n + b] = a == b ? 0.f : s[(size_t)pos[(size_t)a] * n + pos[(size_t)b]];
    }
    return MSFM_OK;
}

int image_words_impl(msfm_ctx* ctx, int image_id, int32_t* out_word) {
    if (!ctx->ret_v) return fail(ctx, MSFM_E_STATE, "msfm_image_words without a vocabulary (msfm_train_vocabulary / msfm_set_vocabulary)");
    RetImages im;
    const int32_t one = image_id;
    int rc = ret_collect(ctx, &one, 1, im);
    if (rc != MSFM_OK) return rc;
    if (im.rows == 0) return MSFM_OK;
    if (!out_word) return fail(ctx, MSFM_E_INVALID, "msfm_image_words: null output");
    RetScratch rs;
    HIPCHK(ctx, rs.assign.ensure((size_t)im.rows * 4));
    rc = ret_assign(ctx, rs, im.segs, rs.assign.as<int>());
    if (rc != MSFM_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(out_word, rs.assign.p, (size_t)im.rows * 4, hipMemcpyDeviceToHost, store_stream(ctx)));
    HIPCHK(ctx, hipStreamSynchronize(store_stream(ctx)));
    return MSFM_OK;
}

// an error leaves nothing in flight on the store's stream: the caller may reuse its buffers, the next call starts idle
int ret_drained(msfm_ctx* ctx, int rc) {
    if (rc != MSFM_OK) (void)hipStreamSynchronize(store_stream(ctx));
    return rc;
}

}  // namespace
