// msfm_tracks.hip.h -- feature tracks on the device (include/msfm_match.h "feature tracks"): the fold kernel that
// unions a sub-batch's kept matches into the session's resident forest, the kernels of msfm_tracks_finish, and the host side of the
// msfm_tracks_* entry points (defined in msfm_match.hip).  The host twin with the same definitions is csrc/msfm_tracks.h.
// Included by msfm_match.hip behind msfm_batch.hip.h.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace msfm {

struct TkImage {
    int base;   // first node of the image; -1: not declared
    int rows;
};

#define MSFM_TK_RLX __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- lock-free union-find on one int32 forest ---------------------------------------------------------------------------------------
// VISIBILITY.  Folds of up to three sub-batches run concurrently on one forest, from workgroups on all eight XCDs.  The XCDs' L2s are
// not coherent with each other and a CU's L1 is never refreshed by another CU's stores, so EVERY access to `parent` inside a fold is a
// relaxed agent-scope atomic -- never a plain load or store.  In the ISA: the loads are `global_load_dword .. sc1` (they bypass the
// CU's L1 and are served by L2), the halving write is `global_atomic_smin` and the link `global_atomic_cmpswap .. sc0` (sc0 marks the
// returning form); read-modify-writes carry no sc1 because at agent scope they EXECUTE at L2, which is the point of coherence for a
// device allocation (sc1 on them would mean system scope).  That gives no ordering between different words, and none is needed: the algorithm stays correct when a
// load returns an OLDER value of a word, because
//   * parent[x] only ever decreases, and every value it ever held is an ancestor-or-self of x in every later state of the forest: a
//     stale parent is still an ancestor, the walk just takes more steps (and ends: values strictly decrease along it);
//   * the only write that LINKS is the compare-and-swap of a root's parent from ITSELF to a smaller root.  It succeeds only if the
//     word still points to itself at the point of coherence, i.e. the node is still a root, whatever this lane believed before;
//   * the halving write (fetch_min of an ancestor into a non-root's word) never touches a root: it is issued only after parent[x] != x
//     was read, and a linked node never becomes a root again.
// A plain load here would be served from L1 / a remote-stale L2 line now and then and would, e.g., keep seeing a node as its own
// root after another XCD linked it: wrong tracks only sometimes.
__device__ __forceinline__ int tk_find(int* parent, int x) {
    int p = __hip_atomic_load(parent + x, MSFM_TK_RLX);
    while (p != x) {
        const int g = __hip_atomic_load(parent + p, MSFM_TK_RLX);
        if (g != p) (void)__hip_atomic_fetch_min(parent + x, g, MSFM_TK_RLX);   // path halving: x skips to its grandparent
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void tk_unite(int* parent, int a, int b) {
    for (;;) {
        a = tk_find(parent, a);
        b = tk_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int expected = hi;   // the larger root goes under the smaller one: a finished component's root is its smallest node
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, MSFM_TK_RLX)) return;
        a = expected;        // hi was linked meanwhile: go on from what it points to now
        b = lo;
    }
}

// read-only walk of a forest nobody writes any more (finish)
__device__ __forceinline__ int tk_root(const int* __restrict__ parent, int x) {
    int p = parent[x];
    while (p != x) {
        x = p;
        p = parent[x];
    }
    return x;
}

// One lane per match of the CSR lists (offsets[P + 1], qt): the pair by binary search in the offsets, the tests of
// msfm_track_pair_class (msfm_tracks.h) in the same order, the range test of both indices, then the union.  No LDS, no fences.
__global__ __launch_bounds__(256) void tk_fold_kernel(const int2* __restrict__ pairs, const long long* __restrict__ offsets, int P,
                                                      const int2* __restrict__ qt, const TkImage* __restrict__ table, int max_id,
                                                      int min_pair_matches, int* __restrict__ parent) {
    MSFM_TAIL_PRIO();
    const long long first = offsets[0], total = offsets[P] - first;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x; m < total; m += stride) {
        const long long at = first + m;
        int lo = 0, hi = P - 1;   // the last pair with offsets[p] <= at: the one whose list holds match `at` (empty lists share an offset)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offsets[mid] <= at) lo = mid;
            else hi = mid - 1;
        }
        const int2 id = pairs[lo];
        if ((unsigned)id.x >= (unsigned)max_id || (unsigned)id.y >= (unsigned)max_id || id.x == id.y) continue;
        if (offsets[lo + 1] - offsets[lo] < (long long)min_pair_matches) continue;
        const TkImage ia = table[id.x], ib = table[id.y];
        if (ia.base < 0 || ib.base < 0) continue;
        const int2 e = qt[m];
        if ((unsigned)e.x >= (unsigned)ia.rows || (unsigned)e.y >= (unsigned)ib.rows) continue;
        tk_unite(parent, ia.base + e.x, ib.base + e.y);
    }
}

// every node v joins in[v] (msfm_tracks_import_forest; the host has checked the range)
__global__ __launch_bounds__(256) void tk_import_kernel(const int* __restrict__ in, int n, int* __restrict__ parent) {
    MSFM_TAIL_PRIO();
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long long)gridDim.x * blockDim.x)
        tk_unite(parent, (int)v, in[v]);
}

__global__ void tk_init_kernel(int* __restrict__ parent, int n) {
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long long)gridDim.x * blockDim.x) parent[v] = (int)v;
}

// ---- finish: flatten, sizes, one ordering by (root, node), flags, two scans, emit ------------------------------------------------------
// Atomics below only COUNT (component sizes, the stats) or set a bit; no order that reaches the output depends on them.
constexpr unsigned kTkInconsistentBit = 0x80000000u;   // in size[root]

__global__ void tk_flatten_kernel(const int* __restrict__ parent, int n, int* __restrict__ root, unsigned* __restrict__ size) {
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long long)gridDim.x * blockDim.x) {
        const int r = tk_root(parent, (int)v);
        root[v] = r;
        atomicAdd(size + r, 1u);
    }
}

// flag[v] = the node belongs to a component of at least 2 nodes (flag has n + 1 entries, the last one 0: its scan is the total)
__global__ void tk_flag_kernel(const int* __restrict__ root, const unsigned* __restrict__ size, int n, int* __restrict__ flag) {
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v <= n; v += (long long)gridDim.x * blockDim.x)
        flag[v] = (v < n && size[root[v]] >= 2u) ? 1 : 0;
}

__global__ void tk_compact_kernel(const int* __restrict__ root, const int* __restrict__ flag, const int* __restrict__ pos, int n,
                                  int* __restrict__ keys, int* __restrict__ vals) {
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (long long)gridDim.x * blockDim.x)
        if (flag[v]) {
            keys[pos[v]] = root[v];
            vals[pos[v]] = (int)v;
        }
}

// the rank of the image a node belongs to: the last p with base[p] <= v (base: n_img + 1 entries)
__device__ __forceinline__ int tk_rank_of_node(const int* __restrict__ base, int n_img, int v) {
    int lo = 0, hi = n_img - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (base[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// in (root, node) order the nodes of one image are neighbours: a track is inconsistent iff two neighbours of it share their image
__global__ void tk_mark_kernel(const int* __restrict__ keys, const int* __restrict__ vals, int m, const int* __restrict__ base, int n_img,
                               unsigned* __restrict__ size) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x + 1; i < m; i += (long long)gridDim.x * blockDim.x)
        if (keys[i] == keys[i - 1] && tk_rank_of_node(base, n_img, vals[i]) == tk_rank_of_node(base, n_img, vals[i - 1]))
            atomicOr(size + keys[i], kTkInconsistentBit);
}

struct TkCounters {
    unsigned long long tracks_total, tracks_inconsistent, tracks_over_max, longest_kept;
};

// keep[i] = the element's track passes the filter, head[i] = and it is the track's first element (both m + 1 entries, the last 0)
__global__ void tk_keep_kernel(const int* __restrict__ keys, int m, const unsigned* __restrict__ size, int min_length, int max_length,
                               int keep_inconsistent, int* __restrict__ keep, int* __restrict__ head, TkCounters* __restrict__ counters) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += (long long)gridDim.x * blockDim.x) {
        int k = 0, h = 0;
        if (i < m) {
            const unsigned s = size[keys[i]];
            const long long len = (long long)(s & ~kTkInconsistentBit);
            const bool inconsistent = (s & kTkInconsistentBit) != 0;
            const bool first = i == 0 || keys[i] != keys[i - 1];
            const bool over = max_length > 0 && len > (long long)max_length;
            k = len >= (long long)(min_length < 2 ? 2 : min_length) && !over && (!inconsistent || keep_inconsistent);
            h = k && first;
            if (first) {
                atomicAdd(&counters->tracks_total, 1ull);
                if (inconsistent) atomicAdd(&counters->tracks_inconsistent, 1ull);
                if (over) atomicAdd(&counters->tracks_over_max, 1ull);
                if (k) atomicMax(&counters->longest_kept, (unsigned long long)len);
            }
        }
        keep[i] = k;
        head[i] = h;
    }
}

__global__ void tk_emit_kernel(const int* __restrict__ keys, const int* __restrict__ vals, int m, const int* __restrict__ keep,
                               const int* __restrict__ head, const int* __restrict__ kpos, const int* __restrict__ hpos,
                               const unsigned* __restrict__ size, const int* __restrict__ base, const int* __restrict__ ids, int n_img,
                               long long* __restrict__ offsets, int* __restrict__ out_img, int* __restrict__ out_idx,
                               unsigned char* __restrict__ out_cons, int* __restrict__ track_of) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += (long long)gridDim.x * blockDim.x) {
        if (i == m) {
            offsets[hpos[m]] = kpos[m];   // offsets[T] = kept observations
            continue;
        }
        if (!keep[i]) continue;
        const int v = vals[i], p = kpos[i], t = hpos[i] - 1 + head[i];   // (heads up to and including i) - 1
        const int r = tk_rank_of_node(base, n_img, v);
        out_img[p] = ids[r];
        out_idx[p] = v - base[r];
        track_of[v] = t;
        if (head[i]) {
            offsets[t] = p;
            out_cons[t] = (size[keys[i]] & kTkInconsistentBit) ? 0 : 1;
        }
    }
}

}  // namespace msfm

namespace {

inline unsigned tk_grid(msfm_ctx* ctx, long long work) {
    const long long blocks = std::max<long long>(1, (work + 255) / 256);
    return (unsigned)std::min<long long>(blocks, 8LL * std::max(1, ctx->cu_count));
}

// every stream of the context idle: the folds in flight have landed
int tk_drain(msfm_ctx* ctx) {
    for (Scratch& s : ctx->sc)
        if (s.stream) HIPCHK(ctx, hipStreamSynchronize(s.stream));
    return MSFM_OK;
}

// HIP events around the fold launches: read and recycled at msfm_tracks_finish (all == true), or -- a long run makes thousands of
// folds -- the oldest ones once more than kTkEventsKept pairs wait (their kernels completed sub-batches ago: the wait is a formality)
constexpr size_t kTkEventsKept = 32;
int tk_collect_events(msfm_ctx* ctx, bool all) {
    TrackSession& ts = ctx->tracks;
    if (!all && ts.ev_pending.size() <= 2 * kTkEventsKept) return MSFM_OK;
    const size_t take = all ? ts.ev_pending.size() : ts.ev_pending.size() - kTkEventsKept;
    for (size_t k = 0; k < take; ++k) {
        const auto e = ts.ev_pending[k];
        HIPCHK(ctx, hipEventSynchronize(e.second));
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, e.first, e.second));
        ts.stats.fold_ms += ms;
        ts.ev_free.push_back(e.first);
        ts.ev_free.push_back(e.second);
    }
    ts.ev_pending.erase(ts.ev_pending.begin(), ts.ev_pending.begin() + (long)take);
    return MSFM_OK;
}

int tk_take_event(msfm_ctx* ctx, hipEvent_t* out) {
    TrackSession& ts = ctx->tracks;
    if (ts.ev_free.empty()) {
        hipEvent_t e;
        HIPCHK(ctx, hipEventCreate(&e));
        ts.ev_free.push_back(e);
    }
    *out = ts.ev_free.back();
    ts.ev_free.pop_back();
    return MSFM_OK;
}

// the fold of CSR lists in device memory, on `stream`, between two events
int tk_launch_fold(msfm_ctx* ctx, hipStream_t stream, const int2* d_pairs, const long long* d_offsets, int P, const int2* d_qt, long long total) {
    TrackSession& ts = ctx->tracks;
    if (P <= 0 || total <= 0 || ts.nd.nodes() == 0) return MSFM_OK;
    int rc = tk_collect_events(ctx, false);
    if (rc != MSFM_OK) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if ((rc = tk_take_event(ctx, &e0)) != MSFM_OK || (rc = tk_take_event(ctx, &e1)) != MSFM_OK) return rc;
    HIPCHK(ctx, hipEventRecord(e0, stream));
    hipLaunchKernelGGL(tk_fold_kernel, dim3(tk_grid(ctx, total)), dim3(256), 0, stream, d_pairs, d_offsets, P, d_qt,
                       (const TkImage*)ts.d_table.as<TkImage>(), (int)MSFM_MAX_IMAGES, ts.min_pair_matches, ts.d_parent.as<int>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(e1, stream));
    ts.ev_pending.emplace_back(e0, e1);
    return MSFM_OK;
}

// what the host knows about the lists of a fold: the pair classes and the edge count (device lists hold no index out of range)
void tk_count_pairs(TrackSession& ts, const int32_t* id1, const int32_t* id2, size_t stride, size_t P, const long long* offs) {
    for (size_t p = 0; p < P; ++p) {
        const int a = id1[p * stride], b = id2[p * stride];
        const int ra = (a >= 0 && a < (int)ts.rank_of.size()) ? ts.rank_of[(size_t)a] : -1;
        const int rb = (b >= 0 && b < (int)ts.rank_of.size()) ? ts.rank_of[(size_t)b] : -1;
        const long long len = offs[p + 1] - offs[p];
        switch (msfm_track_pair_class(ra, rb, a, b, len, ts.min_pair_matches)) {
            case MSFM_TRACK_PAIR_SKIPPED: ts.stats.pairs_skipped += 1; break;
            case MSFM_TRACK_PAIR_SELF: ts.stats.matches_ignored += len; break;
            case MSFM_TRACK_PAIR_BELOW_MIN: ts.stats.pairs_below_min += 1; break;
            default:
                ts.stats.pairs += 1;
                ts.stats.edges += len;
        }
    }
}

// A completed and accepted sub-batch (MatchJob::complete): its final lists -- d_sub_qt in CSR order, d_offsets -- join the forest, on
// the sub-batch's own stream, before that scratch set can be reused (its next sub-batch is launched on the same stream).
// The pairs' (id1, id2) travel through the set's page-locked staging: the caller has just waited for the set's stream, so the copy of
// the set's previous fold has completed and the staging may be rewritten.
int tk_fold_sub_batch(msfm_ctx* ctx, Scratch& sc, const int* id1, const int* id2, size_t P, const long long* h_offsets) {
    TrackSession& ts = ctx->tracks;
    if (!P) return MSFM_OK;
    tk_count_pairs(ts, id1, id2, 1, P, h_offsets);
    if (h_offsets[P] <= 0) return MSFM_OK;
    HIPCHK(ctx, sc.d_tk_pairs.ensure(P * sizeof(int2)));
    HIPCHK(ctx, sc.h_tk_pairs.ensure(P * sizeof(int2), 0));
    int2* h = sc.h_tk_pairs.as<int2>();
    for (size_t p = 0; p < P; ++p) h[p] = make_int2(id1[p], id2[p]);
    HIPCHK(ctx, hipMemcpyAsync(sc.d_tk_pairs.p, h, P * sizeof(int2), hipMemcpyHostToDevice, sc.stream));
    return tk_launch_fold(ctx, sc.stream, sc.d_tk_pairs.as<int2>(), sc.d_offsets.as<long long>(), (int)P, sc.d_sub_qt.as<int2>(), h_offsets[P]);
}

int tracks_begin_impl(msfm_ctx* ctx, const int32_t* ids, int n, const msfm_track_params* params) {
    TrackSession& ts = ctx->tracks;
    if (ts.open) return fail(ctx, MSFM_E_STATE, "msfm_tracks_begin: a track session is open (msfm_tracks_end)");
    if (ctx->series_open) return fail(ctx, MSFM_E_STATE, "msfm_tracks_begin while a streaming series (msfm_match_pairs_begin .. _next) is open");
    if (n < 0 || n > MSFM_MAX_IMAGES || (n > 0 && !ids)) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_begin: bad image list");
    if (params && params->min_pair_matches < 0) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_begin: min_pair_matches must not be negative");
    for (int k = 0; k < n; ++k)
        if (ids[k] < 0 || ids[k] >= MSFM_MAX_IMAGES) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_begin: image id outside [0, MSFM_MAX_IMAGES): " + std::to_string(ids[k]));
    for (int k = 0; k < n; ++k)
        if (ctx->images[(size_t)ids[k]].n < 0) return fail(ctx, MSFM_E_NOIMAGE, "msfm_tracks_begin: image not resident: " + std::to_string(ids[k]));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = settle_store(ctx);   // a pending store build first, as every matching call does
    if (rc != MSFM_OK) return rc;
    std::vector<int32_t> rows((size_t)n);
    for (int k = 0; k < n; ++k) rows[(size_t)k] = ctx->images[(size_t)ids[k]].n;
    MsfmTrackNodes nd;
    switch (msfm_track_number_nodes(ids, rows.data(), n, MSFM_MAX_IMAGES, &nd)) {
        case MSFM_TRACK_NODES_OK: break;
        case MSFM_TRACK_NODES_TWICE: return fail(ctx, MSFM_E_INVALID, "msfm_tracks_begin: an image is listed twice");
        case MSFM_TRACK_NODES_TOO_MANY: return fail(ctx, MSFM_E_INVALID, "msfm_tracks_begin: 2^31 keypoints or more");
        default: return fail(ctx, MSFM_E_INVALID, "msfm_tracks_begin: bad image list");
    }
    ts.release();
    struct Undo {   // a failure below leaves no half-built session
        TrackSession& t;
        bool keep = false;
        ~Undo() {
            if (!keep) t.release();
        }
    } undo{ts};
    const long long nodes = nd.nodes();
    std::vector<TkImage> table((size_t)MSFM_MAX_IMAGES, TkImage{-1, 0});
    std::vector<int> base((size_t)n + 1), idv((size_t)std::max(n, 1), 0);
    ts.rank_of.assign((size_t)MSFM_MAX_IMAGES, -1);
    for (int p = 0; p < n; ++p) {
        table[(size_t)nd.ids[(size_t)p]] = TkImage{(int)nd.base[(size_t)p], nd.rows[(size_t)p]};
        ts.rank_of[(size_t)nd.ids[(size_t)p]] = p;
        base[(size_t)p] = (int)nd.base[(size_t)p];
        idv[(size_t)p] = nd.ids[(size_t)p];
    }
    base[(size_t)n] = (int)nodes;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, ts.d_parent.ensure((size_t)std::max<long long>(1, nodes) * 4));
    HIPCHK(ctx, ts.d_table.ensure(table.size() * sizeof(TkImage)));
    HIPCHK(ctx, ts.d_base.ensure(base.size() * 4));
    HIPCHK(ctx, ts.d_ids.ensure(idv.size() * 4));
    HIPCHK(ctx, hipMemcpyAsync(ts.d_table.p, table.data(), table.size() * sizeof(TkImage), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ts.d_base.p, base.data(), base.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ts.d_ids.p, idv.data(), idv.size() * 4, hipMemcpyHostToDevice, st));
    if (nodes > 0) {
        hipLaunchKernelGGL(tk_init_kernel, dim3(tk_grid(ctx, nodes)), dim3(256), 0, st, ts.d_parent.as<int>(), (int)nodes);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));   // (the host tables above die with this function; folds on other streams follow)
    ts.nd = nd;
    ts.min_pair_matches = params ? params->min_pair_matches : 0;
    ts.add_only = params && params->add_only != 0;
    ts.stats = msfm_track_stats{};
    ts.stats.nodes = nodes;
    ts.open = true;
    ts.closed = ts.finished = false;
    undo.keep = true;
    return MSFM_OK;
}

int tracks_need_open(msfm_ctx* ctx, const char* who, bool accumulating) {
    if (!ctx->tracks.open) return fail(ctx, MSFM_E_STATE, std::string(who) + " without a track session (msfm_tracks_begin)");
    if (accumulating && ctx->tracks.closed) return fail(ctx, MSFM_E_STATE, std::string(who) + " after msfm_tracks_finish");
    return MSFM_OK;
}

int tracks_add_impl(msfm_ctx* ctx, const int32_t* pairs, int n_pairs, const int64_t* offsets, const int32_t* qt) {
    int rc = tracks_need_open(ctx, "msfm_tracks_add", true);
    if (rc != MSFM_OK) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && (!pairs || !offsets))) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_add: bad pair list");
    if (n_pairs == 0) return MSFM_OK;
    if (offsets[0] < 0) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_add: negative offset");
    for (int p = 0; p < n_pairs; ++p)
        if (offsets[p + 1] < offsets[p]) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_add: offsets must not decrease");
    const long long first = offsets[0], total = offsets[n_pairs] - first;
    if (total > 0 && !qt) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_add: null match list");
    TrackSession& ts = ctx->tracks;
    const size_t P = (size_t)n_pairs;
    std::vector<long long> offs(P + 1);
    for (size_t p = 0; p <= P; ++p) offs[p] = (long long)offsets[p] - first;
    tk_count_pairs(ts, pairs, pairs + 1, 2, P, offs.data());
    // matches the device will ignore, counted here: an index outside its image's rows in a pair that is folded
    long long ignored = 0;
    for (size_t p = 0; p < P; ++p) {
        const int a = pairs[2 * p], b = pairs[2 * p + 1];
        const int ra = (a >= 0 && a < MSFM_MAX_IMAGES) ? ts.rank_of[(size_t)a] : -1, rb = (b >= 0 && b < MSFM_MAX_IMAGES) ? ts.rank_of[(size_t)b] : -1;
        if (msfm_track_pair_class(ra, rb, a, b, offs[p + 1] - offs[p], ts.min_pair_matches) != MSFM_TRACK_PAIR_FOLD) continue;
        const int na = ts.nd.rows[(size_t)ra], nb = ts.nd.rows[(size_t)rb];
        for (long long m = first + offs[p]; m < first + offs[p + 1]; ++m)
            if (qt[2 * m] < 0 || qt[2 * m] >= na || qt[2 * m + 1] < 0 || qt[2 * m + 1] >= nb) ++ignored;
    }
    ts.stats.matches_ignored += ignored;
    ts.stats.edges -= ignored;   // (tk_count_pairs counted every match of a folded pair)
    if (total <= 0) return MSFM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    struct Tmp {
        DevBuf pairs, offs, qt;
        ~Tmp() {
            pairs.release();
            offs.release();
            qt.release();
        }
    } tmp;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, tmp.pairs.ensure(P * 8));
    HIPCHK(ctx, tmp.offs.ensure((P + 1) * 8));
    HIPCHK(ctx, tmp.qt.ensure((size_t)total * 8));
    HIPCHK(ctx, hipMemcpyAsync(tmp.pairs.p, pairs, P * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(tmp.offs.p, offs.data(), (P + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(tmp.qt.p, qt + 2 * first, (size_t)total * 8, hipMemcpyHostToDevice, st));
    rc = tk_launch_fold(ctx, st, tmp.pairs.as<int2>(), tmp.offs.as<long long>(), n_pairs, tmp.qt.as<int2>(), total);
    const hipError_t e = hipStreamSynchronize(st);   // (before the temporaries go, whatever the launch returned)
    if (rc != MSFM_OK) return rc;
    HIPCHK(ctx, e);
    return MSFM_OK;
}

int tracks_export_impl(msfm_ctx* ctx, int32_t* parent) {
    int rc = tracks_need_open(ctx, "msfm_tracks_export_forest", false);
    if (rc != MSFM_OK) return rc;
    TrackSession& ts = ctx->tracks;
    if (ts.nd.nodes() == 0) return MSFM_OK;
    if (!parent) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_export_forest: null output");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = tk_drain(ctx);   // every fold in flight has landed
    if (rc != MSFM_OK) return rc;
    HIPCHK(ctx, hipMemcpy(parent, ts.d_parent.p, (size_t)ts.nd.nodes() * 4, hipMemcpyDeviceToHost));
    return MSFM_OK;
}

int tracks_import_impl(msfm_ctx* ctx, const int32_t* parent) {
    int rc = tracks_need_open(ctx, "msfm_tracks_import_forest", true);
    if (rc != MSFM_OK) return rc;
    TrackSession& ts = ctx->tracks;
    const long long n = ts.nd.nodes();
    if (n == 0) return MSFM_OK;
    if (!parent) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_import_forest: null forest");
    for (long long v = 0; v < n; ++v)
        if (parent[v] < 0 || parent[v] >= n) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_import_forest: entry outside [0, nodes) at node " + std::to_string(v));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    struct Tmp {
        DevBuf in;
        ~Tmp() { in.release(); }
    } tmp;
    hipStream_t st = store_stream(ctx);
    HIPCHK(ctx, tmp.in.ensure((size_t)n * 4));
    HIPCHK(ctx, hipMemcpyAsync(tmp.in.p, parent, (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(tk_import_kernel, dim3(tk_grid(ctx, n)), dim3(256), 0, st, (const int*)tmp.in.as<int>(), (int)n, ts.d_parent.as<int>());
    const hipError_t e0 = hipGetLastError(), e1 = hipStreamSynchronize(st);
    HIPCHK(ctx, e0);
    HIPCHK(ctx, e1);
    return MSFM_OK;
}

int tracks_finish_impl(msfm_ctx* ctx, const msfm_track_filter* filter, msfm_track_stats* stats) {
    int rc = tracks_need_open(ctx, "msfm_tracks_finish", false);
    if (rc != MSFM_OK) return rc;
    if (ctx->series_open) return fail(ctx, MSFM_E_STATE, "msfm_tracks_finish while a streaming series (msfm_match_pairs_begin .. _next) is open");
    msfm_track_filter f = {2, 0, 0, 0};
    if (filter) f = *filter;
    if (f.max_length < 0) return fail(ctx, MSFM_E_INVALID, "msfm_tracks_finish: max_length must not be negative");
    TrackSession& ts = ctx->tracks;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    rc = tk_drain(ctx);   // every fold has landed: the forest is final and read with plain loads from here on
    if (rc != MSFM_OK) return rc;
    rc = tk_collect_events(ctx, true);
    if (rc != MSFM_OK) return rc;
    ts.closed = true;      // the accumulation is closed whatever happens below ...
    ts.finished = false;   // ... and there is no result until this finish has succeeded
    ts.tri_valid = false;  // the points of an earlier result (msfm_triangulate_tracks) do not belong to the new one
    ts.mask_valid = false; // ... nor do the inlier bytes of a robust one
    ts.reg_valid = false;  // ... nor do the registrations made from them (msfm_register_images)
    const int n = (int)ts.nd.nodes(), n_img = (int)ts.nd.ids.size();
    hipStream_t st = store_stream(ctx);
    struct Tmp {   // freed when finish returns, whatever it returns
        DevBuf root, size, flag, pos, keys, vals, keys2, vals2, hflag, hpos, counters, sort_tmp;
        hipEvent_t ev[2] = {nullptr, nullptr};
        ~Tmp() {
            for (DevBuf* b : {&root, &size, &flag, &pos, &keys, &vals, &keys2, &vals2, &hflag, &hpos, &counters, &sort_tmp}) b->release();
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    } t;
    for (hipEvent_t& e : t.ev) HIPCHK(ctx, hipEventCreate(&e));
    HIPCHK(ctx, hipEventRecord(t.ev[0], st));
    long long T = 0, O = 0;
    TkCounters hc = {};
    HIPCHK(ctx, ts.r_tid.ensure((size_t)std::max(n, 1) * 4));
    HIPCHK(ctx, hipMemsetAsync(ts.r_tid.p, 0xff, (size_t)std::max(n, 1) * 4, st));   // -1: no kept track
    int m = 0;
    if (n > 0) {
        const size_t nb = (size_t)n * 4;
        HIPCHK(ctx, t.root.ensure(nb));
        HIPCHK(ctx, t.size.ensure(nb));
        HIPCHK(ctx, t.flag.ensure(nb + 4));
        HIPCHK(ctx, t.pos.ensure(nb + 4));
        HIPCHK(ctx, hipMemsetAsync(t.size.p, 0, nb, st));
        const unsigned g = tk_grid(ctx, n);
        hipLaunchKernelGGL(tk_flatten_kernel, dim3(g), dim3(256), 0, st, (const int*)ts.d_parent.as<int>(), n, t.root.as<int>(), t.size.as<unsigned>());
        hipLaunchKernelGGL(tk_flag_kernel, dim3(g), dim3(256), 0, st, (const int*)t.root.as<int>(), (const unsigned*)t.size.as<unsigned>(), n, t.flag.as<int>());
        HIPCHK(ctx, hipGetLastError());
        size_t tmp_bytes = 0;
        HIPCHK(ctx, rocprim::exclusive_scan(nullptr, tmp_bytes, t.flag.as<int>(), t.pos.as<int>(), 0, (size_t)n + 1, rocprim::plus<int>(), st));
        HIPCHK(ctx, t.sort_tmp.ensure(std::max<size_t>(tmp_bytes, 256)));
        HIPCHK(ctx, rocprim::exclusive_scan(t.sort_tmp.p, tmp_bytes, t.flag.as<int>(), t.pos.as<int>(), 0, (size_t)n + 1, rocprim::plus<int>(), st));
        HIPCHK(ctx, hipMemcpyAsync(&m, t.pos.as<int>() + n, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    if (m > 0) {
        const size_t mb = (size_t)m * 4;
        for (DevBuf* b : {&t.keys, &t.vals, &t.keys2, &t.vals2}) HIPCHK(ctx, b->ensure(mb));
        HIPCHK(ctx, t.hflag.ensure(mb + 4));
        HIPCHK(ctx, t.hpos.ensure(mb + 4));
        HIPCHK(ctx, t.counters.ensure(sizeof(TkCounters)));
        HIPCHK(ctx, hipMemsetAsync(t.counters.p, 0, sizeof(TkCounters), st));
        hipLaunchKernelGGL(tk_compact_kernel, dim3(tk_grid(ctx, n)), dim3(256), 0, st, (const int*)t.root.as<int>(), (const int*)t.flag.as<int>(),
                           (const int*)t.pos.as<int>(), n, t.keys.as<int>(), t.vals.as<int>());
        HIPCHK(ctx, hipGetLastError());
        // the one ordering: stable LSD radix sort by root of a list that is already ascending in node => (root, node) order
        unsigned bits = 1;
        while (bits < 31 && ((long long)1 << bits) < (long long)n) ++bits;
        size_t tmp_bytes = 0;
        HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, t.keys.as<int>(), t.keys2.as<int>(), t.vals.as<int>(), t.vals2.as<int>(), (size_t)m, 0u, bits, st));
        HIPCHK(ctx, t.sort_tmp.ensure(std::max<size_t>(tmp_bytes, 256)));
        HIPCHK(ctx, rocprim::radix_sort_pairs(t.sort_tmp.p, tmp_bytes, t.keys.as<int>(), t.keys2.as<int>(), t.vals.as<int>(), t.vals2.as<int>(), (size_t)m, 0u, bits, st));
        const unsigned g = tk_grid(ctx, m);
        const int *keys = t.keys2.as<int>(), *vals = t.vals2.as<int>();
        hipLaunchKernelGGL(tk_mark_kernel, dim3(g), dim3(256), 0, st, keys, vals, m, (const int*)ts.d_base.as<int>(), n_img, t.size.as<unsigned>());
        // (flag / pos are free again: they become keep / its scan)
        int *keep = t.flag.as<int>(), *kpos = t.pos.as<int>(), *head = t.hflag.as<int>(), *hpos = t.hpos.as<int>();
        hipLaunchKernelGGL(tk_keep_kernel, dim3(g), dim3(256), 0, st, keys, m, (const unsigned*)t.size.as<unsigned>(), f.min_length, f.max_length,
                           f.keep_inconsistent, keep, head, t.counters.as<TkCounters>());
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, rocprim::exclusive_scan(nullptr, tmp_bytes, keep, kpos, 0, (size_t)m + 1, rocprim::plus<int>(), st));
        HIPCHK(ctx, t.sort_tmp.ensure(std::max<size_t>(tmp_bytes, 256)));
        HIPCHK(ctx, rocprim::exclusive_scan(t.sort_tmp.p, tmp_bytes, keep, kpos, 0, (size_t)m + 1, rocprim::plus<int>(), st));
        HIPCHK(ctx, rocprim::exclusive_scan(t.sort_tmp.p, tmp_bytes, head, hpos, 0, (size_t)m + 1, rocprim::plus<int>(), st));
        int totals[2] = {0, 0};
        HIPCHK(ctx, hipMemcpyAsync(&totals[0], kpos + m, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(&totals[1], hpos + m, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(&hc, t.counters.p, sizeof(hc), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        O = totals[0];
        T = totals[1];
        HIPCHK(ctx, ts.r_offsets.ensure((size_t)(T + 1) * 8));
        HIPCHK(ctx, ts.r_img.ensure((size_t)std::max<long long>(1, O) * 4));
        HIPCHK(ctx, ts.r_idx.ensure((size_t)std::max<long long>(1, O) * 4));
        HIPCHK(ctx, ts.r_cons.ensure((size_t)std::max<long long>(1, T)));
        hipLaunchKernelGGL(tk_emit_kernel, dim3(g), dim3(256), 0, st, keys, vals, m, (const int*)keep, (const int*)head, (const int*)kpos, (const int*)hpos,
                           (const unsigned*)t.size.as<unsigned>(), (const int*)ts.d_base.as<int>(), (const int*)ts.d_ids.as<int>(), n_img,
                           ts.r_offsets.as<long long>(), ts.r_img.as<int>(), ts.r_idx.as<int>(), ts.r_cons.as<unsigned char>(), ts.r_tid.as<int>());
        HIPCHK(ctx, hipGetLastError());
    } else {
        HIPCHK(ctx, ts.r_offsets.ensure(8));
        HIPCHK(ctx, hipMemsetAsync(ts.r_offsets.p, 0, 8, st));
    }
    HIPCHK(ctx, hipEventRecord(t.ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, t.ev[0], t.ev[1]));
    ts.stats.tracks_total = (int64_t)hc.tracks_total;
    ts.stats.tracks_inconsistent = (int64_t)hc.tracks_inconsistent;
    ts.stats.tracks_over_max_length = (int64_t)hc.tracks_over_max;
    ts.stats.longest_track = (int64_t)hc.longest_kept;
    ts.stats.tracks_kept = T;
    ts.stats.observations_kept = O;
    ts.stats.finish_ms = ms;
    ts.stats.device_bytes = ts.device_bytes();
    ts.finished = true;
    if (stats) *stats = ts.stats;
    return MSFM_OK;
}

int tracks_fetch_impl(msfm_ctx* ctx, int64_t* offsets, int32_t* image_ids, int32_t* point_idx, uint8_t* consistent) {
    int rc = tracks_need_open(ctx, "msfm_fetch_tracks", false);
    if (rc != MSFM_OK) return rc;
    TrackSession& ts = ctx->tracks;
    if (!ts.finished) return fail(ctx, MSFM_E_STATE, "msfm_fetch_tracks before msfm_tracks_finish");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t T = (size_t)ts.stats.tracks_kept, O = (size_t)ts.stats.observations_kept;
    if (offsets) HIPCHK(ctx, hipMemcpy(offsets, ts.r_offsets.p, (T + 1) * 8, hipMemcpyDeviceToHost));
    if (image_ids && O) HIPCHK(ctx, hipMemcpy(image_ids, ts.r_img.p, O * 4, hipMemcpyDeviceToHost));
    if (point_idx && O) HIPCHK(ctx, hipMemcpy(point_idx, ts.r_idx.p, O * 4, hipMemcpyDeviceToHost));
    if (consistent && T) HIPCHK(ctx, hipMemcpy(consistent, ts.r_cons.p, T, hipMemcpyDeviceToHost));
    return MSFM_OK;
}

int tracks_fetch_ids_impl(msfm_ctx* ctx, int image_id, int32_t* out) {
    int rc = tracks_need_open(ctx, "msfm_fetch_track_ids", false);
    if (rc != MSFM_OK) return rc;
    TrackSession& ts = ctx->tracks;
    if (!ts.finished) return fail(ctx, MSFM_E_STATE, "msfm_fetch_track_ids before msfm_tracks_finish");
    if (!ts.declares(image_id)) return fail(ctx, MSFM_E_INVALID, "msfm_fetch_track_ids: image not declared in the session: " + std::to_string(image_id));
    const int p = ts.rank_of[(size_t)image_id], rows = ts.nd.rows[(size_t)p];
    if (rows == 0) return MSFM_OK;
    if (!out) return fail(ctx, MSFM_E_INVALID, "msfm_fetch_track_ids: null output");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemcpy(out, ts.r_tid.as<int>() + ts.nd.base[(size_t)p], (size_t)rows * 4, hipMemcpyDeviceToHost));
    return MSFM_OK;
}

int tracks_end_impl(msfm_ctx* ctx) {
    if (!ctx->tracks.open) return MSFM_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = tk_drain(ctx);   // folds in flight still write the forest
    ctx->tracks.release();
    return rc;
}

}  // namespace
