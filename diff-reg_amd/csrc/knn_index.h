// knn_index.h -- every index the non-rigid evaluation kernels (knn_points.hip: dr_knn_points_f32, dr_nn_stats_f32, dr_flow_metrics_f32) compute,
// stated once for the device and for the host check (tools/knn_index_check.cpp): the ragged offsets, the mapping of a flat workgroup to
// (pair, query block), the staging of a support tile into LDS and the quarter of it each wave walks, the merge rows the four waves exchange,
// the [rows, k] outputs, and the partials of the two-stage reductions that the size queries and the entries share.  Outside hipcc the file
// compiles as plain C++.
#pragma once
#include "nonrigid_index.h"      // nr_slice_ok, align256

namespace dr {

constexpr int KNN_MAX_K = 16;          // slots of a query's sorted list; the kernel is instantiated for 1, 4, 8 and 16
constexpr int KNN_WAVE = 64;
constexpr int KNN_WAVES = 4;           // the waves of a workgroup share ONE block of queries and split every tile between them
constexpr int KNN_BLOCK = 64;          // queries of a workgroup: lane l of every wave owns query l of the block
constexpr int KNN_THREADS = KNN_WAVE * KNN_WAVES;
constexpr int KNN_TILE = 1024;         // supports per LDS tile: x[], y[], z[] of KNN_TILE floats each (12 KiB)
constexpr int KNN_QUARTER = KNN_TILE / KNN_WAVES;   // wave w walks entries [w KNN_QUARTER, (w + 1) KNN_QUARTER) of every tile
constexpr int KNN_VEC = 4;             // a wave reads four consecutive supports of a coordinate at once (one 16-byte broadcast read)

constexpr int KNN_ST_OFFSETS = 4;      // status bit: the pair's offsets do not describe slices of the stacked arrays: the pair is skipped
constexpr int KNN_ST_NONFINITE = 8;    // status bit: a query with a NaN or Inf coordinate was met: its row is +inf / -1

constexpr int FLOW_BLOCK = 256;        // points of a workgroup of the flow metrics, one per thread
constexpr int FLOW_SLOTS = 6;          // n, sum |e|, n_strict, n_relaxed, n_outlier, n_within
constexpr int NN_SLOTS = 4;            // Q, sum dist, sum dist^2, count(dist < limit)

__host__ __device__ inline int knn_max_k() { return KNN_MAX_K; }
__host__ __device__ inline int knn_tile() { return KNN_TILE; }
__host__ __device__ inline int knn_block() { return KNN_BLOCK; }

// the instantiation that serves k: the smallest of 1, 4, 8, 16 that holds it (0: k is out of range)
__host__ __device__ inline int knn_width(int k) { return k < 1 ? 0 : k == 1 ? 1 : k <= 4 ? 4 : k <= 8 ? 8 : k <= KNN_MAX_K ? 16 : 0; }

// ---- blocks of `per` rows a pair of n rows occupies, the grid's upper bound known without reading the offsets, and flat block -> (pair, block)
__host__ __device__ inline int knn_blocks(int n, int per) { return n <= 0 ? 0 : (n + per - 1) / per; }
__host__ __device__ inline long long knn_grid_bound(int total, int P, int per) { return (long long)(total < 0 ? 0 : total) / per + P; }
// a pair whose slice is not usable counts as empty.  O(P) reads of the offset array: P is a batch size
__host__ __device__ inline bool knn_block_to_pair(int P, const int32_t* offsets, int total, int per, long long b, int& pair, int& block) {
    long long first = 0;
    for (int p = 0; p < P; ++p) {
        const int lo = offsets[p], hi = offsets[p + 1];
        const int t = knn_blocks(nr_slice_ok(lo, hi, total) ? hi - lo : 0, per);
        if (b < first + t) {
            pair = p;
            block = (int)(b - first);
            return true;
        }
        first += t;
    }
    return false;
}
// the first flat block of pair p (the final pass of a reduction adds blocks [first, first + knn_blocks(n_p)) in ascending order)
__host__ __device__ inline long long knn_first_block(int p, const int32_t* offsets, int total, int per) {
    long long first = 0;
    for (int q = 0; q < p; ++q) {
        const int lo = offsets[q], hi = offsets[q + 1];
        first += knn_blocks(nr_slice_ok(lo, hi, total) ? hi - lo : 0, per);
    }
    return first;
}

// ---- a pair's rows: the row of the stacked array, and the 32-bit offset of a coordinate inside the pair (3 n < 2^31 is checked by the entries)
__host__ __device__ inline size_t knn_row(int lo, int i) { return (size_t)lo + (size_t)i; }
__host__ __device__ inline size_t knn_coord(int lo, int i, int c) { return knn_row(lo, i) * 3 + (size_t)c; }
__host__ __device__ inline int knn_local_coord(int i, int c) { return 3 * i + c; }
// query of lane `lane` in block `block` of a pair (pair-local; may lie behind the pair: the lane then owns no query)
__host__ __device__ inline int knn_query_of(int block, int lane) { return block * KNN_BLOCK + lane; }

// ---- support tiles: tile t of a pair of S supports holds supports [t KNN_TILE, t KNN_TILE + knn_tile_count(S, t))
__host__ __device__ inline int knn_tiles(int S) { return knn_blocks(S, KNN_TILE); }
__host__ __device__ inline int knn_tile_count(int S, int t) {
    const int left = S - t * KNN_TILE;
    return left <= 0 ? 0 : (left < KNN_TILE ? left : KNN_TILE);
}
// staging: thread `tid` fills entries tid, tid + KNN_THREADS, ... of ALL KNN_TILE entries (an entry behind the tile's count gets NaN, which no
// comparison selects); LDS word of coordinate c of entry e
__host__ __device__ inline int knn_lds_coord(int c, int e) { return c * KNN_TILE + e; }
// the entries of a tile with `count` supports that wave w walks: [w KNN_QUARTER, w KNN_QUARTER + knn_quarter_walk(count, w)), the count of its
// quarter rounded up to KNN_VEC (never past the quarter: KNN_QUARTER is a multiple of KNN_VEC)
__host__ __device__ inline int knn_quarter_first(int w) { return w * KNN_QUARTER; }
__host__ __device__ inline int knn_quarter_walk(int count, int w) {
    int c = count - w * KNN_QUARTER;
    c = c <= 0 ? 0 : (c < KNN_QUARTER ? c : KNN_QUARTER);
    return (c + KNN_VEC - 1) / KNN_VEC * KNN_VEC;
}
// pair-local support index of entry e of tile t
__host__ __device__ inline int knn_support_of(int t, int e) { return t * KNN_TILE + e; }

// ---- merge: waves 1 .. 3 hand their K-slot lists to wave 0 through LDS (the tile's words are reused after a barrier): word of slot j of
// lane `lane` of wave w, in the distance plane (plane 0) or the index plane (plane 1)
__host__ __device__ inline int knn_merge_word(int K, int plane, int w, int j, int lane) {
    return ((plane * (KNN_WAVES - 1) + (w - 1)) * K + j) * KNN_WAVE + lane;
}
constexpr int KNN_MERGE_WORDS = 2 * (KNN_WAVES - 1) * KNN_MAX_K * KNN_WAVE;
constexpr int KNN_TILE_WORDS = 3 * KNN_TILE;
constexpr int KNN_LDS_WORDS = KNN_MERGE_WORDS > KNN_TILE_WORDS ? KNN_MERGE_WORDS : KNN_TILE_WORDS;     // 6 144 words, 24 KiB

// ---- outputs [rows, k]
__host__ __device__ inline size_t knn_out(size_t row, int k, int j) { return row * (size_t)k + (size_t)j; }

// ---- reductions: one row of `slots` doubles per flat block, then the final pass; the workspace is the partials alone
__host__ __device__ inline size_t knn_partial(long long block, int slots, int s) { return (size_t)block * (size_t)slots + (size_t)s; }
__host__ __device__ inline size_t nn_stats_workspace_bytes(int P, int n_q) {
    if (P <= 0) return 0;
    return align256((size_t)knn_grid_bound(n_q, P, KNN_BLOCK) * NN_SLOTS * sizeof(double));
}
__host__ __device__ inline size_t flow_metrics_workspace_bytes(int P, int n) {
    if (P <= 0) return 0;
    return align256((size_t)knn_grid_bound(n, P, FLOW_BLOCK) * FLOW_SLOTS * sizeof(double));
}
// the flow kernel's cross-wave exchange: slot s of wave w
__host__ __device__ inline int flow_lds_word(int w, int s) { return w * FLOW_SLOTS + s; }
constexpr int FLOW_LDS_WORDS = (FLOW_BLOCK / KNN_WAVE) * FLOW_SLOTS;

}  // namespace dr
