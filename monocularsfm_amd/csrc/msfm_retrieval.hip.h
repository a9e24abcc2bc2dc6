// msfm_retrieval.hip.h -- device code of vocabulary retrieval (matching mode 2; semantics in include/msfm_match.h).
// Included by msfm_match.hip after msfm_prefilter.hip.h (kDim, i4v / i16v).
//
//   ret_assign_kernel    the hot path: the nearest word of every row, exhaustively, on v_mfma_i32_32x32x32_i8
//   ret_gather_kernel    the training sample, as contiguous quantised rows q' = q - 128
//   ret_init_kernel / ret_accum_kernel / ret_update_kernel / ret_norms_kernel   integer Lloyd iterations
//   ret_hist_kernel / ret_idf_kernel / ret_rownorm_kernel / ret_normalize_kernel   tf-idf image vectors
//   ret_score_kernel     S = A A^T in one fixed fp32 order
//   ret_topk_kernel      one workgroup per image: radix select of the K-th key, then a bitonic sort of the K
#pragma once
#include "msfm_retrieval.h"

namespace msfm {

// where the quantised rows of an image come from
enum { kRetI8Rows = 0, kRetUnit = 1, kRetInt = 2 };
struct RetSeg {
    const void* src;   // kRetI8Rows: signed rows q' (stride bytes apart); kRetUnit / kRetInt: the store's permuted fp32 rows (rawp)
    int kind;
    int stride;
    int n;
    long long out;     // index of the segment's first row in the output
};
struct RetTile {
    int seg, row0;
};
constexpr int kRetWgRows = 256;              // rows per workgroup of the assignment: four waves of 2 x 32 rows
constexpr int kRetWordTile = 64;             // words per LDS tile
constexpr int kRetLdsStride = 144;           // bytes per word row in LDS (128 + 16: the 32 rows of a fragment read hit distinct banks)
constexpr int kRetPassWords = 8192;          // words per packed pass: 256 blocks of 32 (8 bits of the packed key)
constexpr unsigned kRetKeyBias = 1u << 21;   // |c'|^2 - 2 q'.c' >= -|q'|^2 >= -2^21, and < 2^23 + 2^21 - 2^21: 24 bits once biased

// bytes 16 c .. 16 c + 15 of quantised row `row` of a segment, as q - 128
__device__ __forceinline__ i4v ret_load16(const RetSeg& S, int row, int c) {
    if (S.kind == kRetI8Rows)
        return *reinterpret_cast<const i4v*>(static_cast<const char*>(S.src) + (size_t)row * (size_t)S.stride + 16 * c);
    // element k = 16 c + j of the row sits at rawp_pos(k) = 64 (c >> 2) + 4 j + (c & 3)
    const float* p = static_cast<const float*>(S.src) + (size_t)row * kDim + 64 * (c >> 2) + (c & 3);
    unsigned w[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        unsigned v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float x = p[4 * (4 * g + b)];
            const int q = S.kind == kRetUnit ? (int)rintf(x * 255.0f) : (int)x;   // round half to even
            v |= (unsigned)((q - 128) & 255) << (8 * b);
        }
        w[g] = v;
    }
    i4v r;
    r.x = (int)w[0], r.y = (int)w[1], r.z = (int)w[2], r.w = (int)w[3];
    return r;
}

// grid = tiles, 256 threads.  Each workgroup owns 256 rows (wave w: rows 64 w .. 64 w + 63, two 32-row MFMA blocks) across ALL words:
// the A fragments stay in registers, the words stream through a double-buffered LDS tile of 64.  Per 32 x 32 block the epilogue is two
// VALU instructions per accumulator: v = cn[w] - 512 acc = ((|c'|^2 - 2 q'.c' + 2^21) << 8 | (w >> 5) mod 256) and an unsigned min --
// the lower word wins a tie inside a lane (blocks ascend); every 8192 words the packed minima are folded into a 64-bit (distance, word)
// key, and at the end the 32 lanes of a row take the minimum key (lower word on a tie).  No reduction across workgroups.
__global__ __launch_bounds__(256) void ret_assign_kernel(const RetSeg* __restrict__ segs, const RetTile* __restrict__ tiles,
                                                         const signed char* __restrict__ words, const unsigned* __restrict__ cn,
                                                         int vpad, int* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) char sB[2][kRetWordTile * kRetLdsStride];
    __shared__ unsigned sCn[2][kRetWordTile];
    const RetTile T = tiles[blockIdx.x];
    const RetSeg S = segs[T.seg];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lcol = lane & 31, lhalf = lane >> 5;
    const int wrow0 = T.row0 + 64 * wave;   // first row of the wave

    i4v af[2][4];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int row = wrow0 + 32 * b + lcol;
#pragma unroll
        for (int s = 0; s < 4; ++s) af[b][s] = row < S.n ? ret_load16(S, row, 2 * s + lhalf) : i4v(0);   // padding rows: zeros, never written
    }
    // one word tile: 64 rows x 128 B = 512 pieces of 16 B, two per thread; the 64 constants
    auto fetch = [&](int t, i4v (&g)[2], unsigned& c) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int piece = tid + 256 * u;
            g[u] = *reinterpret_cast<const i4v*>(words + ((size_t)t * kRetWordTile + (piece >> 3)) * kDim + 16 * (piece & 7));
        }
        if (tid < kRetWordTile) c = cn[(size_t)t * kRetWordTile + tid];
    };
    auto stash = [&](int buf, const i4v (&g)[2], unsigned c) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int piece = tid + 256 * u;
            *reinterpret_cast<i4v*>(&sB[buf][(piece >> 3) * kRetLdsStride + 16 * (piece & 7)]) = g[u];
        }
        if (tid < kRetWordTile) sCn[buf][tid] = c;
    };

    unsigned best[2][16];
    unsigned long long run[2][16];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            best[b][r] = 0xffffffffu;
            run[b][r] = ~0ull;
        }
    auto fold_pass = [&](int pass) {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned v = best[b][r];
                const unsigned w = (unsigned)(pass * kRetPassWords) + (v & 255u) * 32u + (unsigned)lcol;
                const unsigned long long key = ((unsigned long long)(v >> 8) << 32) | w;
                if (v != 0xffffffffu && key < run[b][r]) run[b][r] = key;
                best[b][r] = 0xffffffffu;
            }
    };

    const int n_tiles = vpad / kRetWordTile;
    {
        i4v g[2];
        unsigned c = 0;
        fetch(0, g, c);
        stash(0, g, c);
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < n_tiles; ++t) {
        i4v g[2];
        unsigned c = 0;
        const bool more = t + 1 < n_tiles;
        if (more) fetch(t + 1, g, c);
        const char* base = sB[t & 1];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            i4v bf[4];
            const char* wrow = base + (blk * 32 + lcol) * kRetLdsStride + 16 * lhalf;
#pragma unroll
            for (int s = 0; s < 4; ++s) bf[s] = *reinterpret_cast<const i4v*>(wrow + 32 * s);
            const unsigned cw = sCn[t & 1][blk * 32 + lcol];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                i16v acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[b][0], bf[0], i16v(0), 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[b][1], bf[1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[b][2], bf[2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[b][3], bf[3], acc, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) best[b][r] = min(best[b][r], cw - ((unsigned)acc[r] << 9));
            }
        }
        if ((((t + 1) * kRetWordTile) % kRetPassWords) == 0 || !more) fold_pass((t * kRetWordTile) / kRetPassWords);
        if (more) stash((t + 1) & 1, g, c);
        __syncthreads();
    }
    // the 32 lanes of a half hold the 32 columns of the same 16 rows: minimum key across them
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            unsigned long long k = run[b][r];
#pragma unroll
            for (int m = 1; m < 32; m <<= 1) {
                const unsigned lo = __shfl_xor((unsigned)k, m), hi = __shfl_xor((unsigned)(k >> 32), m);
                const unsigned long long o = ((unsigned long long)hi << 32) | lo;
                k = o < k ? o : k;
            }
            const int row = wrow0 + 32 * b + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
            if (lcol == 0 && row < S.n) out[S.out + row] = (int)(unsigned)(k & 0xffffffffu);
        }
}

// the constant of every word: ((|c'|^2 + 2^21) << 8) | ((w >> 5) & 255); padding words (zero rows) get all ones and never win
__global__ void ret_norms_kernel(const signed char* __restrict__ words, int v, int vpad, unsigned* __restrict__ cn) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= vpad) return;
    if (w >= v) {
        cn[w] = 0xffffffffu;
        return;
    }
    const signed char* p = words + (size_t)w * kDim;
    unsigned s = 0;
    for (int k = 0; k < kDim; ++k) s += (unsigned)((int)p[k] * (int)p[k]);
    cn[w] = ((s + kRetKeyBias) << 8) | ((unsigned)(w >> 5) & 255u);
}

// sample row t = row t * step of the concatenation (prefix[i] = first row of segment i), as q' bytes; 8 threads per row
__global__ void ret_gather_kernel(const RetSeg* __restrict__ segs, const long long* __restrict__ prefix, int nseg, long long step,
                                  long long count, signed char* __restrict__ out) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= count * 8) return;
    const long long t = g >> 3;
    const int c = (int)(g & 7);
    const long long p = t * step;
    int lo = 0, hi = nseg - 1;   // the last segment with prefix <= p
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    const RetSeg S = segs[lo];
    *reinterpret_cast<i4v*>(out + t * kDim + 16 * c) = ret_load16(S, (int)(p - prefix[lo]), c);
}

// word k starts as sample row msfm_ret_initial_row(k)
__global__ void ret_init_kernel(const signed char* __restrict__ sample, long long ms, int v, signed char* __restrict__ words) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= v * 8) return;
    const int k = g >> 3, c = g & 7;
    const long long row = msfm_ret_initial_row(k, ms, v);
    *reinterpret_cast<i4v*>(words + (size_t)k * kDim + 16 * c) = *reinterpret_cast<const i4v*>(sample + row * kDim + 16 * c);
}

// integer sums of q (not q') per word and dimension, and the counts: the order of the atomics cannot change a bit
__global__ void ret_accum_kernel(const signed char* __restrict__ sample, const int* __restrict__ assign, long long ms,
                                 unsigned* __restrict__ sums, unsigned* __restrict__ cnt) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ms * kDim) return;
    const long long row = g >> 7;
    const int k = (int)(g & 127);
    const int w = assign[row];
    atomicAdd(&sums[(size_t)w * kDim + k], (unsigned)((int)sample[g] + 128));
    if (k == 0) atomicAdd(&cnt[w], 1u);
}

// c = floor((2 sum + cnt) / (2 cnt)) for every word with rows; *changed != 0 when any byte moved
__global__ void ret_update_kernel(const unsigned* __restrict__ sums, const unsigned* __restrict__ cnt, int v,
                                  signed char* __restrict__ words, int* __restrict__ changed) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= v * kDim) return;
    const unsigned n = cnt[g >> 7];
    if (n == 0) return;   // an empty word keeps its centroid
    const int c = (int)msfm_ret_centroid(sums[g], n);
    const signed char q = (signed char)(c - 128);
    if (words[g] != q) {
        words[g] = q;
        *changed = 1;
    }
}

// c_iw: rows of image i (row r belongs to the last image with prefix <= r) whose word is w
__global__ void ret_hist_kernel(const int* __restrict__ assign, const long long* __restrict__ prefix, int n_img, long long rows,
                                int vpad, unsigned* __restrict__ hist) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int lo = 0, hi = n_img - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= r) lo = mid;
        else hi = mid - 1;
    }
    atomicAdd(&hist[(size_t)lo * vpad + assign[r]], 1u);
}

// idf_w = ln(N / n_w) in fp64; 0 for a word no image contains (its c_iw are all 0)
__global__ void ret_idf_kernel(const unsigned* __restrict__ hist, int n_img, int vpad, double* __restrict__ idf) {
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= vpad) return;
    int nw = 0;
    for (int i = 0; i < n_img; ++i) nw += hist[(size_t)i * vpad + w] != 0u;
    idf[w] = nw ? log((double)n_img / (double)nw) : 0.0;
}

// |v_i| in fp64, one wave per image, a fixed order (strided lane sums, then a fixed butterfly): the same bits on every call
__global__ void ret_rownorm_kernel(const unsigned* __restrict__ hist, const double* __restrict__ idf, int n_img, int vpad,
                                   double* __restrict__ norm) {
    const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n_img) return;
    double s = 0.0;
    for (int w = lane; w < vpad; w += 64) {
        const double x = (double)hist[(size_t)i * vpad + w] * idf[w];
        s = fma(x, x, s);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o = __shfl_xor(s, m);
        s = lane & m ? o + s : s + o;   // both lanes of a pair form the same sum (fp addition is commutative)
    }
    if (lane == 0) norm[i] = sqrt(s);
}

// a_iw = fl32(c_iw idf_w / |v_i|), in place over the counts; 0 where |v_i| = 0
__global__ void ret_normalize_kernel(unsigned* __restrict__ hist, const double* __restrict__ idf, const double* __restrict__ norm,
                                     int n_img, int vpad) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (long long)n_img * vpad) return;
    const int i = (int)(g / vpad), w = (int)(g % vpad);
    const double nv = norm[i];
    const float a = nv > 0.0 ? (float)((double)hist[g] * idf[w] / nv) : 0.f;
    reinterpret_cast<float*>(hist)[g] = a;
}

// S = A A^T, one 64 x 64 tile per workgroup (256 threads, 4 x 4 outputs each), tiles on and above the diagonal only, mirrored.  Every
// output is ONE fmaf chain over w = 0 .. vpad-1 in ascending order: a fixed order, the same bits whatever the tile or the call;
// fmaf(a, b, s) == fmaf(b, a, s), so s_ij and s_ji are the same bits.  Terms with a zero factor add an exact zero.
constexpr int kRetScoreTile = 64, kRetScoreK = 16;
__global__ __launch_bounds__(256) void ret_score_kernel(const float* __restrict__ a, int n_img, int vpad, const int2* __restrict__ tile_ij,
                                                        float* __restrict__ s) {
    __shared__ float sI[kRetScoreK][kRetScoreTile + 4], sJ[kRetScoreK][kRetScoreTile + 4];
    const int2 tij = tile_ij[blockIdx.x];
    const int i0 = tij.x * kRetScoreTile, j0 = tij.y * kRetScoreTile;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    float acc[4][4] = {};
    for (int k0 = 0; k0 < vpad; k0 += kRetScoreK) {
        // 64 rows x 16 words per side: 1024 values, four per thread
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = threadIdx.x + 256 * u;
            const int rr = e >> 4, kk = e & 15;
            const int ri = i0 + rr, rj = j0 + rr;
            sI[kk][rr] = ri < n_img ? a[(size_t)ri * vpad + k0 + kk] : 0.f;
            sJ[kk][rr] = rj < n_img ? a[(size_t)rj * vpad + k0 + kk] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kRetScoreK; ++kk) {
            float x[4], y[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                x[q] = sI[kk][ty + 16 * q];
                y[q] = sJ[kk][tx + 16 * q];
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = fmaf(x[p], y[q], acc[p][q]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + ty + 16 * p, j = j0 + tx + 16 * q;
            if (i < n_img && j < n_img) {
                s[(size_t)i * n_img + j] = acc[p][q];
                s[(size_t)j * n_img + i] = acc[p][q];
            }
        }
}

// One workgroup per image i: the K largest selection keys (msfm_ret_key) of row i, j != i, s > 0, highest first.  Keys are distinct
// (ids are), so an MSB-first radix select over the eight key bytes finds the K-th key exactly; the keys at or above it are collected and
// sorted (bitonic, in LDS).  out: n x k keys (0 past the image's count), counts: n.
constexpr int kRetMaxK = 1024;
__global__ __launch_bounds__(256) void ret_topk_kernel(const float* __restrict__ s, const int* __restrict__ ids, int n_img, int k,
                                                       unsigned long long* __restrict__ out, int* __restrict__ counts) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sel[kRetMaxK];
    __shared__ unsigned long long s_prefix, s_mask;
    __shared__ int s_need, s_count;
    const int i = blockIdx.x, tid = threadIdx.x;
    const float* row = s + (size_t)i * n_img;
    auto key_of = [&](int j) -> unsigned long long { return j == i ? 0ull : msfm_ret_key(row[j], ids[j]); };
    // candidates
    if (tid == 0) s_count = 0;
    __syncthreads();
    int mine = 0;
    for (int j = tid; j < n_img; j += 256) mine += key_of(j) != 0ull;
    atomicAdd(&s_count, mine);
    __syncthreads();
    const int want = min(k, s_count);
    if (tid == 0) {
        s_prefix = 0ull;
        s_mask = 0ull;
        s_need = want;
    }
    __syncthreads();
    if (want > 0) {
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0u;
            __syncthreads();
            const unsigned long long prefix = s_prefix, mask = s_mask;
            for (int j = tid; j < n_img; j += 256) {
                const unsigned long long key = key_of(j);
                if (key && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255ull], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0;
                int b = 255;
                for (; b > 0; --b) {
                    if (cum + hist[b] >= (unsigned)s_need) break;
                    cum += hist[b];
                }
                s_need -= (int)cum;
                s_prefix = prefix | ((unsigned long long)b << shift);
                s_mask = mask | (255ull << shift);
            }
            __syncthreads();
        }
    }
    // collect the keys >= the K-th one (exactly `want` of them), then sort them in descending order
    const unsigned long long kth = s_prefix;
    for (int t = tid; t < kRetMaxK; t += 256) sel[t] = 0ull;
    if (tid == 0) s_count = 0;
    __syncthreads();
    if (want > 0)
        for (int j = tid; j < n_img; j += 256) {
            const unsigned long long key = key_of(j);
            if (key && key >= kth) {
                const int slot = atomicAdd(&s_count, 1);
                if (slot < kRetMaxK) sel[slot] = key;
            }
        }
    __syncthreads();
    int len = 1;
    while (len < want) len <<= 1;
    for (int size = 2; size <= len; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < len; t += 256) {
                const int o = t ^ stride;
                if (o > t) {
                    const bool desc = (t & size) == 0;
                    const unsigned long long x = sel[t], y = sel[o];
                    if (desc ? x < y : x > y) {
                        sel[t] = y;
                        sel[o] = x;
                    }
                }
            }
            __syncthreads();
        }
    for (int t = tid; t < k; t += 256) out[(size_t)i * k + t] = t < want ? sel[t] : 0ull;
    if (tid == 0) counts[i] = want;
}

}  // namespace msfm
