// nonrigid_index.h -- every index the non-rigid ICP kernels (nonrigid.hip: dr_ed_graph_f32, dr_ed_warp_f32, dr_nicp_cost_grad_f32,
// dr_nicp_adam_f32) compute, stated once for the device and for the host check (tools/nonrigid_index_check.cpp): the ragged offset arrays,
// the mapping of a flat workgroup index to (pair, tile), the adjacency bit map and its ordered edge scan, the node-major CSR lists the solver
// gathers its gradient through, the LDS carve that fixes the node capacity, and the carve of the workspaces that the size queries and the
// entry points share.  Outside hipcc the file compiles as plain C++.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
#include <stddef.h>
#include <stdint.h>
#include "carve.h"               // align256

namespace dr {

constexpr int NR_MAX_ANCHORS = 8;      // K of a point's anchor list (the reference's 4DMatch setting is 6)
constexpr int NR_TILE = 128;           // points per workgroup of the anchor search and of the warp (one per thread)
constexpr int NR_STAGE = 1024;         // nodes per LDS stage of the anchor search (a float4 each: 16 KiB)
constexpr int NR_EDGE_BLOCK = 256;     // threads of the edge scan, one adjacency row each
constexpr int NR_SOLVER_BLOCK = 1024;  // threads of the solver's one workgroup per pair
constexpr int NR_COMP = 12;            // parameters per node: rotation row-major (9), translation (3)
constexpr int NR_LDS_BYTES = 160 * 1024;   // LDS of one gfx950 compute unit, all of it usable by one workgroup

// a pair's slice [lo, hi) of a stacked array of `total` rows, read from an offset array of P + 1 entries
__host__ __device__ inline bool nr_slice_ok(int lo, int hi, int total) { return lo >= 0 && hi >= lo && hi <= total; }

// tiles of NR_TILE points a pair of n points occupies (none for an empty pair)
__host__ __device__ inline int nr_tiles(int n) { return n <= 0 ? 0 : (n + NR_TILE - 1) / NR_TILE; }

// the grid: an upper bound of sum_p nr_tiles(n_p) over P pairs whose n_p >= 0 add up to at most `total`, known without reading the offsets
__host__ __device__ inline long long nr_grid_bound(int total, int P) { return (long long)(total < 0 ? 0 : total) / NR_TILE + P; }

// flat workgroup b -> (pair, tile): pairs in order, nr_tiles(n_p) tiles each; false when b lies behind the last tile.  A pair whose slice is not
// usable counts as empty.  O(P) reads of the offset array: P is a batch size.
__host__ __device__ inline bool nr_tile_to_pair(int P, const int32_t* offsets, int total, long long b, int& pair, int& tile) {
    long long first = 0;
    for (int p = 0; p < P; ++p) {
        const int lo = offsets[p], hi = offsets[p + 1];
        const int t = nr_tiles(nr_slice_ok(lo, hi, total) ? hi - lo : 0);
        if (b < first + t) {
            pair = p;
            tile = (int)(b - first);
            return true;
        }
        first += t;
    }
    return false;
}

// nodes of the stage that starts at node k0 of a pair of n: min(NR_STAGE, n - k0), never negative
__host__ __device__ inline int nr_stage_count(int n, int k0) {
    const int left = n - k0;
    return left <= 0 ? 0 : (left < NR_STAGE ? left : NR_STAGE);
}

// the reference's effective K: knn() asks KeOps for min(K, M) neighbours (vision3d/ops/knn.py:76)
__host__ __device__ inline int nr_effective_k(int K, int M) { return K < M ? K : M; }

// ---- adjacency bit map: row i of pair p (nodes [m0, m0 + M)) is the `words` 32-bit words from word (m0 + i) * words, with words fixed by
// max_nodes, the largest node count of one pair as the HOST states it, so that the host can size the map without reading the offsets (a pair
// with more nodes is not computed); bit j of a row: word j / 32, bit j % 32
__host__ __device__ inline int nr_bitmap_words(int n_nodes) { return n_nodes <= 0 ? 0 : (n_nodes + 31) / 32; }
__host__ __device__ inline size_t nr_bitmap_word(int m0, int i, int words, int j) { return ((size_t)m0 + (size_t)i) * (size_t)words + (size_t)(j >> 5); }
__host__ __device__ inline uint32_t nr_bitmap_bit(int j) { return 1u << (j & 31); }

// the workspace of dr_ed_graph_f32: the bit map, then per node the number of set bits of its row and the sum of its row's skinning weights
struct NrGraphCarve {
    size_t bitmap, row_count, row_sum, bytes;
};
__host__ __device__ inline NrGraphCarve nr_graph_carve(int n_nodes, int max_nodes) {
    NrGraphCarve c;
    const size_t m = n_nodes > 0 ? (size_t)n_nodes : 0;
    c.bitmap = 0;
    c.row_count = c.bitmap + align256(m * (size_t)nr_bitmap_words(max_nodes) * sizeof(uint32_t));
    c.row_sum = c.row_count + align256(m * sizeof(int32_t));
    c.bytes = c.row_sum + align256(m * sizeof(double));
    return c;
}

// ---- the solver's LDS carve, in floats, for a pair of at most `cap` nodes.  Per node: two copies of rotation | translation (an iteration reads
// one and writes the other, which saves the barrier between the gradient gather and the update), exp_avg, exp_avg_sq (NR_COMP each) and the
// node's position (3).  Behind them the per-wave partial sums of a cost reduction (3 doubles per wave).
constexpr int NR_NODE_FLOATS = 4 * NR_COMP + 3;
constexpr int NR_REDUCE_BYTES = (NR_SOLVER_BLOCK / 64) * 3 * 8;
struct NrLdsCarve {
    int param0, param1, exp_avg, exp_avg_sq, node;      // float offsets
    int reduce_byte, status_byte, bytes;                // byte offsets: the reduction's doubles, the pair's status word, the end
};
__host__ __device__ inline NrLdsCarve nr_lds_carve(int cap) {
    NrLdsCarve c;
    const int m = cap > 0 ? cap : 0;
    c.param0 = 0;
    c.param1 = c.param0 + m * NR_COMP;
    c.exp_avg = c.param1 + m * NR_COMP;
    c.exp_avg_sq = c.exp_avg + m * NR_COMP;
    c.node = c.exp_avg_sq + m * NR_COMP;
    c.reduce_byte = ((c.node + m * 3) * 4 + 7) & ~7;
    c.status_byte = c.reduce_byte + NR_REDUCE_BYTES;
    c.bytes = c.status_byte + 8;
    return c;
}
// the node capacity: the largest cap whose carve fits the compute unit's LDS (8 bytes of alignment slack, 8 of status)
__host__ __device__ inline int nr_node_capacity() { return (NR_LDS_BYTES - NR_REDUCE_BYTES - 16) / (NR_NODE_FLOATS * 4); }

// ---- the solver's workspace.  Pair p owns rows [c0, c1) of the correspondences, [m0, m1) of the nodes and [e0, e1) of the edges; its slices of the
// arrays below start at c0 * 3 (resid), c0 * K (anchor, weight, lm_*), m0 + p (the three row-pointer arrays: M + 1 entries per pair) and e0.
struct NrSolveCarve {
    size_t resid;        // double [n_corr, 3]  residual of the warped correspondence, written once per iteration
    size_t anchor;       // int32 [n_corr, K]   pair-local anchor, -1 where absent or out of range
    size_t weight;       // float [n_corr, K]   w / (sum_k w + eps)
    size_t lm_ptr;       // int32 [n_nodes + P] node-major CSR of (correspondence, column) entries
    size_t lm_corr;      // int32 [n_corr, K]   correspondence of a CSR entry (pair-local)
    size_t lm_pw;        // float4 [n_corr, K]  (point, weight) of a CSR entry
    size_t out_ptr;      // int32 [n_nodes + P] CSR of the edges that leave a node
    size_t out_adj;      // (int32 other, float weight) [n_edges]
    size_t in_ptr;       // int32 [n_nodes + P] CSR of the edges that enter a node
    size_t in_adj;       // (int32 other, float weight) [n_edges]
    size_t bytes;
};
__host__ __device__ inline NrSolveCarve nr_solve_carve(int P, int n_corr, int n_nodes, int n_edges, int K) {
    NrSolveCarve c;
    const size_t p = P > 0 ? (size_t)P : 0, n = n_corr > 0 ? (size_t)n_corr : 0, m = n_nodes > 0 ? (size_t)n_nodes : 0;
    const size_t e = n_edges > 0 ? (size_t)n_edges : 0, k = K > 0 ? (size_t)K : 0;
    c.resid = 0;
    c.anchor = c.resid + align256(n * 3 * 8);
    c.weight = c.anchor + align256(n * k * 4);
    c.lm_ptr = c.weight + align256(n * k * 4);
    c.lm_corr = c.lm_ptr + align256((m + p) * 4);
    c.lm_pw = c.lm_corr + align256(n * k * 4);
    c.out_ptr = c.lm_pw + align256(n * k * 16);
    c.out_adj = c.out_ptr + align256((m + p) * 4);
    c.in_ptr = c.out_adj + align256(e * 8);
    c.in_adj = c.in_ptr + align256((m + p) * 4);
    c.bytes = c.in_adj + align256(e * 8);
    return c;
}

// ---- node-major CSR construction, as one node's thread performs it: a count pass, an exclusive prefix over the nodes, a fill pass; both passes walk
// the entries in ascending order, so a node's list is in ascending entry order whatever the thread schedule.
// entries of node `node` among `count` keys (anchor columns or edge endpoints); keys outside [0, M) belong to no node
__host__ __device__ inline int nr_csr_count(const int32_t* keys, int count, int stride, int node) {
    int c = 0;
    for (int i = 0; i < count; ++i) c += keys[(size_t)i * stride] == node ? 1 : 0;
    return c;
}
// exclusive prefix in place over ptr[0 .. M]: ptr[i] holds node i's count on entry, ptr[M] is ignored; returns the total
__host__ __device__ inline int nr_csr_prefix(int32_t* ptr, int M) {
    int run = 0;
    for (int i = 0; i < M; ++i) {
        const int c = ptr[i];
        ptr[i] = run;
        run += c;
    }
    ptr[M] = run;
    return run;
}

// beta^n in double by squaring (n >= 0): the bias corrections of Adam from the step count
__host__ __device__ inline double nr_pow_int(double b, int n) {
    double r = 1.0;
    while (n > 0) {
        if (n & 1) r *= b;
        b *= b;
        n >>= 1;
    }
    return r;
}

}  // namespace dr
