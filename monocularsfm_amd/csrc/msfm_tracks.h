// msfm_tracks.h -- the pure host parts of the feature tracks (include/msfm_match.h "feature tracks"): node
// numbering, the filter predicate, and a serial union-find with the device's definitions -- the HOST TWIN of csrc/msfm_tracks.hip.h.
// No HIP, no library state: compiled by g++ in tests/test_tracks_host.py, by host/HostTestApi.cpp, and usable by a caller without a
// session.  Included by msfm_match.hip for the numbering and the predicate.
//
// What the reference does with a `matches` table before anything else: SceneGraph::Load -> AddCorrespondences joins the pairwise
// matches of every pair with at least min_num_matches matches into per-keypoint correspondence lists
// (src/Reconstruction/SceneGraph.cpp:11-85, 170-251) and MapBuilder walks them transitively while it grows Tracks
// (src/Reconstruction/MapBuilder.cpp:333-340, 469-488).  The closure of that walk is a connected component of the graph whose nodes
// are (image, keypoint) and whose edges are the matches: that is what is computed here, once, for the whole run.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

// ---- node numbering: images ranked by ascending id, node v = base[rank] + keypoint index -------------------------------------------
struct MsfmTrackNodes {
    std::vector<int32_t> ids;    // ascending, distinct
    std::vector<int32_t> rows;   // rows of ids[p]
    std::vector<int64_t> base;   // exclusive prefix sum of rows, n + 1 entries: base[n] = number of nodes
    int64_t nodes() const { return base.empty() ? 0 : base.back(); }
    int rank_of(int id) const {   // -1: not declared
        const auto it = std::lower_bound(ids.begin(), ids.end(), (int32_t)id);
        return (it != ids.end() && *it == id) ? (int)(it - ids.begin()) : -1;
    }
    // the rank of the image a node belongs to: the last p with base[p] <= v (images without rows own no node)
    int rank_of_node(int64_t v) const { return (int)(std::upper_bound(base.begin(), base.end() - 1, v) - base.begin()) - 1; }
};

enum { MSFM_TRACK_NODES_OK = 0, MSFM_TRACK_NODES_BAD_ID = 1, MSFM_TRACK_NODES_TWICE = 2, MSFM_TRACK_NODES_TOO_MANY = 3 };

// ids in any order (rows[k] belongs to ids[k]); max_id: ids must lie in [0, max_id).  2^31 nodes or more do not fit an int32 forest.
inline int msfm_track_number_nodes(const int32_t* ids, const int32_t* rows, int n, int max_id, MsfmTrackNodes* out) {
    std::vector<std::pair<int32_t, int32_t>> v((size_t)std::max(n, 0));
    for (int k = 0; k < n; ++k) {
        if (ids[k] < 0 || ids[k] >= max_id || rows[k] < 0) return MSFM_TRACK_NODES_BAD_ID;
        v[(size_t)k] = {ids[k], rows[k]};
    }
    std::sort(v.begin(), v.end());
    out->ids.clear();
    out->rows.clear();
    out->base.assign(1, 0);
    for (size_t k = 0; k < v.size(); ++k) {
        if (k && v[k].first == v[k - 1].first) return MSFM_TRACK_NODES_TWICE;
        out->ids.push_back(v[k].first);
        out->rows.push_back(v[k].second);
        out->base.push_back(out->base.back() + v[k].second);
        if (out->base.back() >= ((int64_t)1 << 31)) return MSFM_TRACK_NODES_TOO_MANY;
    }
    return MSFM_TRACK_NODES_OK;
}

// ---- the filter ---------------------------------------------------------------------------------------------------------------------
struct MsfmTrackFilter {
    int32_t min_length = 2;       // values below 2 mean 2
    int32_t max_length = 0;       // 0: no bound
    int32_t keep_inconsistent = 0;
};
inline bool msfm_track_kept(int64_t length, bool consistent, const MsfmTrackFilter& f) {
    if (length < std::max<int64_t>(2, f.min_length)) return false;
    if (f.max_length > 0 && length > f.max_length) return false;
    return consistent || f.keep_inconsistent != 0;
}

// what one pair does in a fold (the same order of tests on the device and in the twin)
enum { MSFM_TRACK_PAIR_FOLD = 0, MSFM_TRACK_PAIR_SKIPPED = 1, MSFM_TRACK_PAIR_SELF = 2, MSFM_TRACK_PAIR_BELOW_MIN = 3 };
inline int msfm_track_pair_class(int rank1, int rank2, int id1, int id2, int64_t length, int min_pair_matches) {
    if (rank1 < 0 || rank2 < 0) return MSFM_TRACK_PAIR_SKIPPED;      // an image outside the declared set
    if (id1 == id2) return MSFM_TRACK_PAIR_SELF;                     // every match of it is ignored
    if (length < min_pair_matches) return MSFM_TRACK_PAIR_BELOW_MIN;   // SceneGraph::Load's rule
    return MSFM_TRACK_PAIR_FOLD;
}

// ---- the twin -----------------------------------------------------------------------------------------------------------------------
struct MsfmTrackCounts {   // the integer part of msfm_track_stats, field for field
    int64_t nodes = 0, edges = 0, pairs = 0, pairs_skipped = 0, pairs_below_min = 0, matches_ignored = 0;
    int64_t tracks_total = 0, tracks_inconsistent = 0, tracks_over_max_length = 0, tracks_kept = 0, observations_kept = 0, longest_track = 0;
};
struct MsfmTrackResult {
    MsfmTrackCounts counts;
    std::vector<int64_t> offsets;      // T + 1
    std::vector<int32_t> image_ids;    // per kept observation
    std::vector<int32_t> point_idx;
    std::vector<uint8_t> consistent;   // T
    std::vector<int32_t> track_of;     // per node: its kept track's number or -1
};

struct MsfmTrackTwin {
    MsfmTrackNodes nd;
    int min_pair_matches = 0;
    std::vector<int32_t> parent;
    MsfmTrackCounts counts;

    void begin(const MsfmTrackNodes& nodes, int min_pair) {
        nd = nodes;
        min_pair_matches = min_pair;
        parent.resize((size_t)nd.nodes());
        for (size_t v = 0; v < parent.size(); ++v) parent[v] = (int32_t)v;
        counts = MsfmTrackCounts{};
        counts.nodes = nd.nodes();
    }
    int32_t find(int32_t x) {
        while (parent[(size_t)x] != x) {   // path halving
            parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
            x = parent[(size_t)x];
        }
        return x;
    }
    // the larger root goes under the smaller one: the root of a component is its smallest node whatever the order of the unions
    void unite(int32_t a, int32_t b) {
        a = find(a);
        b = find(b);
        if (a == b) return;
        parent[(size_t)std::max(a, b)] = std::min(a, b);
    }
    // CSR lists as msfm_match_pairs returns them: pairs = n_pairs x (id1, id2), qt = (q, t) rows
    void add(const int32_t* pairs, int n_pairs, const int64_t* offsets, const int32_t* qt) {
        for (int p = 0; p < n_pairs; ++p) {
            const int id1 = pairs[2 * p], id2 = pairs[2 * p + 1];
            const int r1 = nd.rank_of(id1), r2 = nd.rank_of(id2);
            const int64_t len = offsets[p + 1] - offsets[p];
            switch (msfm_track_pair_class(r1, r2, id1, id2, len, min_pair_matches)) {
                case MSFM_TRACK_PAIR_SKIPPED: counts.pairs_skipped += 1; continue;
                case MSFM_TRACK_PAIR_SELF: counts.matches_ignored += len; continue;
                case MSFM_TRACK_PAIR_BELOW_MIN: counts.pairs_below_min += 1; continue;
                default: break;
            }
            counts.pairs += 1;
            for (int64_t m = offsets[p]; m < offsets[p + 1]; ++m) {
                const int32_t q = qt[2 * m], t = qt[2 * m + 1];
                if (q < 0 || q >= nd.rows[(size_t)r1] || t < 0 || t >= nd.rows[(size_t)r2]) {
                    counts.matches_ignored += 1;   // AddCorrespondences ignores it (SceneGraph.cpp:172-176, 198-248)
                    continue;
                }
                counts.edges += 1;
                unite((int32_t)(nd.base[(size_t)r1] + q), (int32_t)(nd.base[(size_t)r2] + t));
            }
        }
    }
    // another forest over the same nodes: every v joins in[v]; false: an entry outside [0, nodes)
    bool import_forest(const int32_t* in) {
        for (size_t v = 0; v < parent.size(); ++v)
            if (in[v] < 0 || (size_t)in[v] >= parent.size()) return false;
        for (size_t v = 0; v < parent.size(); ++v) unite((int32_t)v, in[v]);
        return true;
    }
    void export_forest(int32_t* out) {
        for (size_t v = 0; v < parent.size(); ++v) out[v] = find((int32_t)v);
    }
    MsfmTrackResult finish(const MsfmTrackFilter& f) {
        MsfmTrackResult r;
        r.counts = counts;
        const size_t n = parent.size();
        std::vector<int32_t> root(n), size(n, 0);
        for (size_t v = 0; v < n; ++v) size[(size_t)(root[v] = find((int32_t)v))] += 1;
        // the nodes of the components of size >= 2 by (root, node): the root is the smallest node, so the tracks come by ascending
        // smallest node and the elements of each by ascending node
        std::vector<int32_t> order;
        for (size_t v = 0; v < n; ++v)
            if (size[(size_t)root[v]] >= 2) order.push_back((int32_t)v);
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return root[(size_t)a] < root[(size_t)b]; });
        r.track_of.assign(n, -1);
        r.offsets.assign(1, 0);
        for (size_t i = 0; i < order.size();) {
            size_t j = i;
            bool consistent = true;
            while (j < order.size() && root[(size_t)order[j]] == root[(size_t)order[i]]) {
                if (j > i && nd.rank_of_node(order[j]) == nd.rank_of_node(order[j - 1])) consistent = false;
                ++j;
            }
            const int64_t len = (int64_t)(j - i);
            r.counts.tracks_total += 1;
            if (!consistent) r.counts.tracks_inconsistent += 1;
            if (f.max_length > 0 && len > f.max_length) r.counts.tracks_over_max_length += 1;
            if (msfm_track_kept(len, consistent, f)) {
                const int32_t t = (int32_t)r.consistent.size();
                for (size_t k = i; k < j; ++k) {
                    const int p = nd.rank_of_node(order[k]);
                    r.image_ids.push_back(nd.ids[(size_t)p]);
                    r.point_idx.push_back((int32_t)(order[k] - nd.base[(size_t)p]));
                    r.track_of[(size_t)order[k]] = t;
                }
                r.consistent.push_back(consistent ? 1 : 0);
                r.offsets.push_back((int64_t)r.image_ids.size());
                r.counts.longest_track = std::max(r.counts.longest_track, len);
            }
            i = j;
        }
        r.counts.tracks_kept = (int64_t)r.consistent.size();
        r.counts.observations_kept = (int64_t)r.image_ids.size();
        return r;
    }
};
