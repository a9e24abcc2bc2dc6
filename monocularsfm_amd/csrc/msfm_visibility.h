// msfm_visibility.h -- map visibility counting shared by the device kernels (msfm_visibility.hip.h, hipcc) and the host twin
// (host/HostTestApi.cpp, MapVisibility, g++): the one quantity the reference's MapBuilder derives its decisions from -- how many
// tracks or points two images share (FindFirstInitialImage / FindSecondInitialImage, Map::GetNextImageIds, Map::GetLocalBAData;
// DESIGN.md section 24).  Integer counting only: every output is a sum of ones, so no order reaches an output and the device, the
// twin and an independent numpy reference agree exactly.
//
//   standing track   basis TRACKS: every kept consistent track.  basis MAP: a kept consistent track whose record has POINT | ERROR_OK
//                    | ANGLE_OK (msfm_ext::continues).  An inconsistent track never counts anything.
//   counting element of a standing track.  TRACKS: every element.  MAP, image without a valid pose: every element (a correspondence a
//                    registration would use).  MAP, image with a valid pose: iff its observation is fitting -- inlier byte 1 where the
//                    session has bytes, else every element (the image is posed, so the observation is used).
//   per image        three counters, planar: word [k * n + rank] -- k = 0: n_elements (elements of kept consistent tracks, both bases
//                    alike), k = 1: n_visible (elements of standing tracks, counting or not), k = 2: n_points (counting elements of a
//                    POSED image; 0 under TRACKS, where no image is posed).
//   matrix           C[row][rank]: standing tracks in which the query image of that row and the image of that rank both have a
//                    counting element.  A consistent track has at most one element per image, so one add per (query element,
//                    counting element) pair is exact; the entry at the query image's own rank is its number of counting elements.
//   walk             one track in two walks (walk_track): the elements for the per-image counters, then per counting element of a
//                    query image one add per counting element.  `first` / `step` share a track's elements among the lanes of a wave
//                    (0 / 1: one lane, the host); the tally of a track is the sum of its lanes' tallies.
#pragma once

#include "msfm_extend.h"

namespace msfm_vis {

enum { BASIS_TRACKS = 0, BASIS_MAP = 1 };
enum { ROUTE_AUTO = 0, ROUTE_GLOBAL = 1, ROUTE_LDS = 2 };
enum { IMG_ELEMENTS = 0, IMG_VISIBLE = 1, IMG_POINTS = 2, kImageCounters = 3 };

// A track at most this long is walked by one lane; a longer one by a whole wave (msfm_visibility.hip.h, vis_wave_kernel), so that one
// lane never holds its wave behind more than kLaneMax^2 adds.
constexpr int kLaneMax = 64;

// one element of a track as the walk sees it
struct Elem {
    int rank;             // of its image
    int row;              // of its image in the query list, -1: not a query image
    bool posed;           // its image has a valid pose (always false under TRACKS)
    unsigned char byte;   // its inlier byte; 1 where the session has none
};

// what one lane's share of one track adds to the call's statistics
struct Tally {
    long long tracks, elements, increments;
};

MSFM_FHD bool standing(int basis, bool consistent, int status) {
    if (!consistent) return false;
    if (basis == BASIS_TRACKS) return true;
    msfm_point3d r = {};
    r.status = status;
    return msfm_ext::continues(r);
}

MSFM_FHD bool counting(int basis, const Elem& e) { return basis == BASIS_TRACKS || !e.posed || e.byte != 0; }

// One kept track of n elements: elem(k) -> Elem; status: its record's (not read under TRACKS).  add_image(k, rank): 1 to counter k of
// the image; add_cell(row, rank): 1 to the matrix (never called without rows).  The lane takes elements first, first + step, ...
template <class E, class AddImage, class AddCell>
MSFM_FHD void walk_track(const E& elem, int n, int first, int step, int basis, bool consistent, int status, bool rows, AddImage add_image,
                         AddCell add_cell, Tally* tally) {
    if (!consistent) return;
    const bool stands = standing(basis, consistent, status);
    long long counted = 0, cells = 0;
    for (int k = first; k < n; k += step) {
        const Elem e = elem(k);
        add_image((int)IMG_ELEMENTS, e.rank);
        if (!stands) continue;
        add_image((int)IMG_VISIBLE, e.rank);
        if (!counting(basis, e)) continue;
        counted += 1;
        if (e.posed) add_image((int)IMG_POINTS, e.rank);
    }
    if (stands && rows) {
        for (int q = 0; q < n; ++q) {   // (every lane of a wave reads the same element: the loop is uniform)
            const Elem a = elem(q);
            if (a.row < 0 || !counting(basis, a)) continue;
            for (int j = first; j < n; j += step) {
                const Elem b = elem(j);
                if (!counting(basis, b)) continue;
                add_cell(a.row, b.rank);
                cells += 1;
            }
        }
    }
    tally->tracks += (stands && first == 0) ? 1 : 0;
    tally->elements += counted;
    tally->increments += cells;
}

// ---- the route of a call: the ONE statement of the policy (both routes give the same counts) --------------------
// ROUTE_GLOBAL: every add is an agent-scope add in global memory.  ROUTE_LDS: the per-image counters (3 n words), and the matrix rows
// (n_query x n words) where both fit kLdsMatrixBytes, are privatised per workgroup in LDS and flushed once.
constexpr long long kLdsMaxBytes = 64 * 1024;      // what one workgroup gets without asking for more than the default limit
constexpr long long kLdsMatrixBytes = 32 * 1024;   // counters + matrix at most this: five workgroups a CU (160 KiB of LDS)
constexpr long long kLdsCuBytes = 160 * 1024;

struct Route {
    int route;           // ROUTE_GLOBAL or ROUTE_LDS: the one to run; 0: ROUTE_LDS was asked for and does not fit
    int lds_bytes;       // of one workgroup under ROUTE_LDS (0 under ROUTE_GLOBAL)
    int matrix_in_lds;   // the matrix rows are privatised as well
    int wgs_per_cu;      // workgroups of 256 threads a CU's LDS holds (0 under ROUTE_GLOBAL)
};

// n declared images, n_query rows, T kept tracks, O kept observations; want: ROUTE_*.  AUTO: ROUTE_LDS wherever it fits -- measured
// from 3 190 to 612 112 observations over 300 images it was the faster one or within 0.6 us: T and O decide nothing.
inline Route vis_route(int want, long long n, long long n_query, long long T, long long O) {
    const long long image_bytes = 4 * (long long)kImageCounters * (n > 0 ? n : 1);
    const long long matrix_bytes = 4 * (n_query > 0 ? n_query : 0) * (n > 0 ? n : 1);
    const bool fits = image_bytes <= kLdsMaxBytes;
    const bool with_matrix = fits && n_query > 0 && image_bytes + matrix_bytes <= kLdsMatrixBytes;
    const long long bytes = image_bytes + (with_matrix ? matrix_bytes : 0);
    const long long per_cu = kLdsCuBytes / bytes;   // (8: what 2048 threads a CU admit)
    const Route lds = {ROUTE_LDS, (int)bytes, with_matrix ? 1 : 0, (int)(per_cu > 8 ? 8 : per_cu)};
    const Route global = {ROUTE_GLOBAL, 0, 0, 0};
    if (want == ROUTE_GLOBAL) return global;
    if (want == ROUTE_LDS) return fits ? lds : Route{0, 0, 0, 0};
    (void)T;
    (void)O;
    return fits ? lds : global;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the host twin: MapVisibility over the outputs of the other twins -----------------------------------------------------------------
// tracks and rank_of_id as TriangulateTracks takes them; n ranks; posed: one byte per rank (all zero under TRACKS); row_of: per rank the
// row in the query list or -1; status: per track (nullptr under TRACKS); mask: the session's inlier bytes or nullptr.  image_counters
// (3 n words, planar) and matrix (n_query x n, may be nullptr without rows) are ADDED to, as is tally.
inline void MapVisibility(const int64_t* offsets, const int32_t* image_ids, const uint8_t* consistent, int64_t n_tracks, const int* rank_of_id,
                          int n, const uint8_t* posed, const int* row_of, int n_query, int basis, const msfm_point3d* points,
                          const uint8_t* mask, uint32_t* image_counters, uint32_t* matrix, Tally* tally) {
    for (int64_t t = 0; t < n_tracks; ++t) {
        const int64_t b = offsets[t];
        const int len = (int)(offsets[t + 1] - b);
        const auto elem = [&](int k) {
            const int r = rank_of_id[image_ids[b + k]];
            return Elem{r, row_of[r], basis == BASIS_MAP && posed[r] != 0, mask ? mask[b + k] : (unsigned char)1};
        };
        walk_track(elem, len, 0, 1, basis, consistent[t] != 0, points ? points[t].status : 0, n_query > 0,
                   [&](int k, int rank) { image_counters[(size_t)k * (size_t)n + (size_t)rank] += 1u; },
                   [&](int row, int rank) { matrix[(size_t)row * (size_t)n + (size_t)rank] += 1u; }, tally);
    }
}
#endif

}  // namespace msfm_vis
