// lgr_index.h -- every index the RANSAC-free rigid estimators (lgr.hip: dr_weighted_procrustes_f32, dr_lgr_f32, dr_spatial_consistency_f32,
// dr_sc_row_sums_f32, dr_sc_leading_eigenvector_f32) compute, stated once for the device and for the host check (tools/lgr_index_check.cpp):
// the assignment of a group's elements to the four VIRTUAL waves of the fixed summation order, the mapping of a flat workgroup to the groups
// and hypotheses it serves, the chunk scan of a problem's patch ids, the LDS tiles of the row sums and the carve of the two workspaces.
// Outside hipcc the file compiles as plain C++.
#pragma once
#include "knn_index.h"           // knn_blocks, knn_grid_bound, knn_block_to_pair, knn_row, knn_coord, knn_local_coord; nr_slice_ok, align256

namespace dr {

constexpr int LGR_WAVE = 64;
constexpr int LGR_VWAVES = 4;          // virtual waves of the summation order: element i belongs to virtual wave (i / 64) % 4, lane i % 64
constexpr int LGR_THREADS = LGR_WAVE * LGR_VWAVES;
constexpr int LGR_STRIDE = LGR_THREADS;            // a (virtual wave, lane) slot meets elements slot, slot + 256, ... in ascending order
constexpr int LGR_WAVE_LIMIT = 256;    // a group of at most this many rows is fitted by ONE wave, a longer one by the four waves of a workgroup
constexpr int LGR_GROUPS_PER_BLOCK = LGR_VWAVES;   // a workgroup of the fit serves this many consecutive groups
constexpr int LGR_MAX_STEPS = 64;      // num_refinement_steps of one call

constexpr int LGR_ST_OFFSETS = 4;      // bad offsets, or patch ids that descend: the problem is skipped
constexpr int LGR_ST_NONFINITE = 8;    // a NaN / Inf coordinate, weight or score: the problem (group) is skipped
constexpr int LGR_ST_DEGENERATE = 16;  // no positive weight, or an all-zero H: identity rotation
constexpr int LGR_ST_EMPTY = 32;       // a problem without correspondences: identity

constexpr int SC_BLOCK = 64;           // queries of a workgroup of the row sums: one wave, lane l owns query l of the block
constexpr int SC_TILE = 512;           // supports per LDS tile: six arrays (src x y z, tgt x y z) and the multiplier, SC_TILE floats each (14 KiB)
constexpr int SC_PLANES = 7;
constexpr int SC_LDS_WORDS = SC_PLANES * SC_TILE;
constexpr int SC_DENSE_THREADS = 256;

__host__ __device__ inline int lgr_wave_limit() { return LGR_WAVE_LIMIT; }
__host__ __device__ inline int sc_block() { return SC_BLOCK; }
__host__ __device__ inline int sc_tile() { return SC_TILE; }

// ---- the summation order: the first element of slot (virtual wave v, lane l), and how many elements of a group of n rows the slot meets
__host__ __device__ inline int lgr_slot_first(int v, int lane) { return v * LGR_WAVE + lane; }
__host__ __device__ inline int lgr_slot_count(int n, int v, int lane) {
    const int first = lgr_slot_first(v, lane);
    return n <= first ? 0 : (n - first + LGR_STRIDE - 1) / LGR_STRIDE;
}
// a team of `nw` physical waves (1 or 4): physical wave w serves virtual waves w, w + nw, ...
__host__ __device__ inline bool lgr_team_serves(int w, int nw, int v) { return v % nw == w; }
// LDS word of term k of virtual wave v in the workgroup's exchange of N terms
__host__ __device__ inline int lgr_exchange_word(int N, int v, int k) { return v * N + k; }
constexpr int LGR_MAX_TERMS = 9;
constexpr int LGR_EXCHANGE_WORDS = LGR_VWAVES * LGR_MAX_TERMS;

// ---- the fit's grid: workgroup b serves groups [b * 4, b * 4 + 4); wave w fits group b * 4 + w when it is short, all four waves the long ones
__host__ __device__ inline long long lgr_fit_blocks(long long groups) { return (groups + LGR_GROUPS_PER_BLOCK - 1) / LGR_GROUPS_PER_BLOCK; }
__host__ __device__ inline long long lgr_fit_group(long long b, int w) { return b * LGR_GROUPS_PER_BLOCK + w; }
__host__ __device__ inline bool lgr_uses_wave(int len, int wave_limit) { return len <= wave_limit; }
__host__ __device__ inline size_t lgr_transform_word(long long g, int k) { return (size_t)g * 16 + (size_t)k; }

// ---- chunks: problem p's correspondences are rows [lo, hi) of the stacked arrays; a run of equal patch ids of length >= min_local is a chunk.
// The scan writes the problem's run starts (problem-local) to slots lo + r of `starts`, then the chunks (start, end, GLOBAL rows) to slots
// lo + j of chunk_lo / chunk_hi: a problem of n rows has at most n runs and at most n chunks, so both lists fit the problem's own slice.
__host__ __device__ inline size_t lgr_list_slot(int lo, int j) { return (size_t)lo + (size_t)j; }
__host__ __device__ inline bool lgr_is_run_start(const int32_t* ids, int i) { return i == 0 || ids[i] != ids[i - 1]; }
// the most hypotheses a call can have, known without reading the offsets (min_local >= 1)
__host__ __device__ inline long long lgr_chunk_bound(int n_corr, int min_local) { return (long long)(n_corr < 0 ? 0 : n_corr) / (min_local < 1 ? 1 : min_local); }
// problem p's slice is usable when the offsets ascend from entry 0 up to entry p + 1 inside [0, total]: the usable problems of a call are then
// a chain of disjoint slices (their lists and outputs cannot overlap, and their chunks together are at most n_corr).  O(P) reads: a batch size
__host__ __device__ inline bool lgr_prefix_ok(const int32_t* off, int p, int total) {
    if (off[0] < 0 || off[p + 1] > total) return false;
    for (int q = 0; q <= p; ++q)
        if (off[q + 1] < off[q]) return false;
    return true;
}

// ---- workspace of dr_lgr_f32: starts, chunk_lo, chunk_hi [n_corr] int32 (per problem, in its slice); n_chunks [P], chunk_off [P + 1] int32;
// the hypotheses of the call in one dense list dense_lo, dense_hi, dense_p [n_corr] int32 (hypothesis g = chunk_off[p] + j); counts [n_corr]
// int32 and transforms [n_corr, 16] float32 (used when the caller does not take the hypotheses)
struct LgrCarve {
    size_t starts, chunk_lo, chunk_hi, n_chunks, chunk_off, dense_lo, dense_hi, dense_p, counts, transforms, total;
};
__host__ __device__ inline LgrCarve lgr_carve(int P, int n_corr) {
    LgrCarve c;
    const size_t n = (size_t)(n_corr < 0 ? 0 : n_corr), p = (size_t)(P < 0 ? 0 : P);
    size_t at = 0;
    c.starts = at;      at += align256(n * sizeof(int32_t));
    c.chunk_lo = at;    at += align256(n * sizeof(int32_t));
    c.chunk_hi = at;    at += align256(n * sizeof(int32_t));
    c.n_chunks = at;    at += align256(p * sizeof(int32_t));
    c.chunk_off = at;   at += align256((p + 1) * sizeof(int32_t));
    c.dense_lo = at;    at += align256(n * sizeof(int32_t));
    c.dense_hi = at;    at += align256(n * sizeof(int32_t));
    c.dense_p = at;     at += align256(n * sizeof(int32_t));
    c.counts = at;      at += align256(n * sizeof(int32_t));
    c.transforms = at;  at += align256(n * 16 * sizeof(float));
    c.total = P <= 0 ? 0 : at;
    return c;
}

// ---- spatial consistency: support tiles (as knn_index.h's, with SC_TILE), LDS word of plane c of entry e, the dense output
__host__ __device__ inline int sc_tiles(int S) { return knn_blocks(S, SC_TILE); }
__host__ __device__ inline int sc_tile_count(int S, int t) {
    const int left = S - t * SC_TILE;
    return left <= 0 ? 0 : (left < SC_TILE ? left : SC_TILE);
}
__host__ __device__ inline int sc_support_of(int t, int e) { return t * SC_TILE + e; }
__host__ __device__ inline int sc_lds_word(int plane, int e) { return plane * SC_TILE + e; }
__host__ __device__ inline int sc_query_of(int block, int lane) { return block * SC_BLOCK + lane; }
// element (i, j) of a problem's dense [Nq, Ns] matrix that starts at element `base` of the output
__host__ __device__ inline size_t sc_dense_at(long long base, int Ns, int i, int j) { return (size_t)base + (size_t)i * (size_t)Ns + (size_t)j; }
// the dense kernel: a workgroup owns SC_BLOCK rows of a problem; thread t writes elements t, t + 256, ... of the rows' [rows, Ns] block
__host__ __device__ inline int sc_block_rows(int Nq, int block) {
    const int left = Nq - block * SC_BLOCK;
    return left <= 0 ? 0 : (left < SC_BLOCK ? left : SC_BLOCK);
}

// ---- workspace of dr_sc_leading_eigenvector_f32: y [n] float32 (SC v before the normalisation), done [P] int32
struct EigCarve {
    size_t y, done, total;
};
__host__ __device__ inline EigCarve eig_carve(int P, int n) {
    EigCarve c;
    size_t at = 0;
    c.y = at;       at += align256((size_t)(n < 0 ? 0 : n) * sizeof(float));
    c.done = at;    at += align256((size_t)(P < 0 ? 0 : P) * sizeof(int32_t));
    c.total = P <= 0 ? 0 : at;
    return c;
}
// the dense-matrix product: a wave owns a row; workgroup b of a problem serves rows [b * 4, b * 4 + 4)
constexpr int EIG_ROWS_PER_BLOCK = LGR_VWAVES;
__host__ __device__ inline int eig_row_of(int block, int w) { return block * EIG_ROWS_PER_BLOCK + w; }

}  // namespace dr
