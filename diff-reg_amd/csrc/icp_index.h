// icp_index.h -- every index the point-to-point ICP kernels (icp.hip: dr_icp_p2p_f32) compute, stated once for the device and for the host
// check (tools/icp_index_check.cpp): the mapping of a flat workgroup to (pair, block of source rows), the rows a wave of the block walks, the
// slots of a workgroup's partial moments and the blocks the finish adds for a pair, the exchange words of the sweep, the grid the entry
// launches, and the carve of the workspace that the size query and the entry point share.  The target grid (cell, key, nine runs, binary
// search) is item3d_index.h's.  Outside hipcc the file compiles as plain C++.
#pragma once
#include "lgr_index.h"           // lgr_prefix_ok, lgr_transform_word; knn_blocks, knn_grid_bound, knn_block_to_pair, knn_first_block,
                                 // knn_partial, knn_row, knn_coord; nr_slice_ok, align256
#include "item3d_index.h"        // it3_cell, it3_key, it3_run_keys, it3_lower_bound, it3_blocks, IT3_BLOCK; next_pow2

namespace dr {

constexpr int ICP_WAVE = 64;
constexpr int ICP_WAVES = 4;               // waves of a workgroup of the sweep: one source row per wave at a time
constexpr int ICP_THREADS = ICP_WAVE * ICP_WAVES;
constexpr int ICP_ROWS_PER_WAVE = 16;      // rows a wave walks one after the other
constexpr int ICP_BLOCK_ROWS = ICP_WAVES * ICP_ROWS_PER_WAVE;   // source rows of a workgroup: all of ONE pair
constexpr int ICP_SLOTS = 17;              // count, sum d2, sum p (3), sum q (3), sum p q^T (9, row-major): doubles
constexpr int ICP_FINISH_THREADS = 64;     // the finish: ONE wave per pair (the kernel relies on the wave's lockstep: icp.hip)
constexpr int ICP_MAX_ITERATIONS = 4096;   // max_iteration of one call (two launches each)
constexpr int ICP_MAX_PAIRS = 65535;       // what the pair bits of it3_key hold; P is a batch size: pairs are found by O(P) walks of the offsets
constexpr int ICP_LDS_WORDS = ICP_WAVES * ICP_SLOTS;            // doubles of the sweep's exchange: 544 bytes

constexpr int ICP_ST_OFFSETS = 4;          // the pair's offsets do not describe slices: the pair is skipped
constexpr int ICP_ST_NONFINITE = 8;        // a NaN / Inf coordinate or initial transform: the pair is skipped
constexpr int ICP_ST_DEGENERATE = 16;      // a fit met an H of rank <= 1 (Jacobi completion), or an all-zero H (identity update)
constexpr int ICP_ST_EMPTY = 32;           // an evaluation found no correspondence: the pair stopped and kept its transform
constexpr int ICP_ST_SKIP = ICP_ST_OFFSETS | ICP_ST_NONFINITE;

constexpr double ICP_RANK_TOL = 1e-12;     // H has rank <= 1 when its second singular value is <= this times its first

// pair-local source row that wave w of block `block` meets in its round j (ascending in j; may lie behind the pair: the wave then stops)
__host__ __device__ inline int icp_row_of(int block, int w, int j) { return block * ICP_BLOCK_ROWS + j * ICP_WAVES + w; }
// exchange word of slot k of wave w
__host__ __device__ inline int icp_exchange_word(int w, int k) { return w * ICP_SLOTS + k; }
// the sweep's grid: known without reading the offsets
__host__ __device__ inline long long icp_grid(int ns, int P) { return knn_grid_bound(ns, P, ICP_BLOCK_ROWS); }

// the workspace: the grid origin of every pair, the (key, target) list padded to a power of two for the sort, the targets in key order, the
// partial moments of every workgroup of the sweep, the done flag of every pair
struct IcpCarve {
    size_t origin, keys, vals, sorted, partial, done, bytes;
};
__host__ __device__ inline IcpCarve icp_carve(int P, int ns, int nt) {
    IcpCarve c;
    const size_t p = P > 0 ? (size_t)P : 0, t = nt > 0 ? (size_t)nt : 0;
    const size_t pad = nt > 0 ? (size_t)next_pow2(nt) : 0;
    size_t at = 0;
    c.origin = at;   at += align256(p * 4 * sizeof(float));
    c.keys = at;     at += align256(pad * sizeof(unsigned long long));
    c.vals = at;     at += align256(pad * sizeof(uint32_t));
    c.sorted = at;   at += align256(t * 4 * sizeof(float));
    c.partial = at;  at += align256((size_t)icp_grid(ns, P > 0 ? P : 0) * ICP_SLOTS * sizeof(double));
    c.done = at;     at += align256(p * sizeof(int32_t));
    c.bytes = P <= 0 ? 0 : at;
    return c;
}

}  // namespace dr
