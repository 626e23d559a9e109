// nonrigid_gn_index.h -- every index the Gauss-Newton non-rigid ICP kernels (nonrigid_gn.hip: dr_nicp_gn_f32, dr_nicp_gn_normal_f32,
// dr_spd_solve_f64) compute, stated once for the device and for the host check (tools/nonrigid_gn_index_check.cpp): the order of the 6 M
// unknowns, the dense normal matrix and its blocks, the tiles of the blocked Cholesky factorisation, and the carve of the workspace that the size
// query and the entries share.  Outside hipcc the file compiles as plain C++.
#pragma once
#include "nonrigid_index.h"

namespace dr {

constexpr int NRG_B = 64;              // block width of the factorisation: a 64 x 64 float64 tile is 32 KiB
constexpr int NRG_MAX_NODES = 1024;    // nodes of one pair: what a call needs grows with the workspace ((6 M)^2 doubles per pair: 302 MB at the
                                       // cap), not with LDS.  The cap itself sizes the set-up pass's static LDS scratch of 3 (M + 1) ints
                                       // (12 KiB) and is the assembly's grid width; it lies above the Adam solver's 801.
constexpr int NRG_MAX_N = 6 * NRG_MAX_NODES;   // unknowns of one system
constexpr int NRG_TILE_PAD = 66;       // doubles per LDS row of a transposed tile: 16-byte aligned rows, no 64-stride bank pattern
constexpr int NRG_UPDATE_T = 256;      // threads of the trailing update: 16 x 16, a 4 x 4 patch of the 64 x 64 tile each
constexpr int NRG_SUBST_T = 1024;      // threads of the substitution's one workgroup per system
constexpr int NRG_ST_PIVOT = 32;       // status bit: a pivot was not finite or not > 0; the pair stopped before that iteration's update

// ---- the unknowns of a pair of M nodes, in the order of the reference's permute(1, 3, 0, 2, 4): all axis-angle increments (3 n + d), then all
// translation increments (3 M + 3 n + d).  i in [0, 6): component of node n's 6-vector (rotation 0..2, translation 3..5).
__host__ __device__ inline int nrg_unknown(int M, int n, int i) { return i < 3 ? 3 * n + i : 3 * M + 3 * n + (i - 3); }

// element (row, col) of system p: systems are stacked with a fixed slot of ld * ld doubles, ld = the HOST's bound of every system's size
__host__ __device__ inline size_t nrg_elem(int p, int ld, int row, int col) {
    return (size_t)p * (size_t)ld * (size_t)ld + (size_t)row * (size_t)ld + (size_t)col;
}
__host__ __device__ inline size_t nrg_rhs(int p, int ld, int row) { return (size_t)p * (size_t)ld + (size_t)row; }

// ---- blocks of a system of n unknowns
__host__ __device__ inline int nrg_blocks(int n) { return n <= 0 ? 0 : (n + NRG_B - 1) / NRG_B; }
// rows (= columns) of block k: NRG_B, fewer in the ragged last one, 0 behind it
__host__ __device__ inline int nrg_block_rows(int n, int k) {
    const int left = n - k * NRG_B;
    return left <= 0 ? 0 : (left < NRG_B ? left : NRG_B);
}
// the trailing update of step k launches a square of (nb - k - 1)^2 workgroups per system; workgroup (x, y) owns tile (bi, bj) = (k + 1 + x,
// k + 1 + y) and works only on and below the diagonal
__host__ __device__ inline bool nrg_update_tile(int n, int k, int x, int y, int& bi, int& bj) {
    bi = k + 1 + x;
    bj = k + 1 + y;
    return bj <= bi && nrg_block_rows(n, bi) > 0;
}

// ---- the workspace of dr_nicp_gn_f32 / dr_nicp_gn_normal_f32: the Adam solver's lists (nr_solve_carve, built by the same code), then
struct NrGnCarve {
    NrSolveCarve lists;  // at offset 0
    size_t n6;           // int32 [P]            6 M of the pair, 0 for a pair that is not computed
    size_t rot;          // float [n_nodes, 9]   working rotations (used when the caller's state has none)
    size_t trn;          // float [n_nodes, 3]   working translations
    size_t jac;          // double [n_corr, K, 4] per anchor column: R_a (p - g_a) and the column's Jacobian weight (0: the column has no block)
    size_t b;            // double [P, ld]       right-hand side, then the solution
    size_t A;            // double [P, ld, ld]   normal matrix, then its Cholesky factor in the lower triangle
    size_t bytes;
    int ld;              // 6 * max_nodes
};
__host__ __device__ inline NrGnCarve nrg_carve(int P, int n_corr, int n_nodes, int n_edges, int K, int max_nodes) {
    NrGnCarve c;
    c.lists = nr_solve_carve(P, n_corr, n_nodes, n_edges, K);
    const size_t p = P > 0 ? (size_t)P : 0, n = n_corr > 0 ? (size_t)n_corr : 0, m = n_nodes > 0 ? (size_t)n_nodes : 0;
    const size_t k = K > 0 ? (size_t)K : 0;
    c.ld = 6 * (max_nodes > 0 ? max_nodes : 0);
    c.n6 = c.lists.bytes;
    c.rot = c.n6 + align256(p * 4);
    c.trn = c.rot + align256(m * 9 * 4);
    c.jac = c.trn + align256(m * 3 * 4);
    c.b = c.jac + align256(n * k * 4 * 8);
    c.A = c.b + align256(p * (size_t)c.ld * 8);
    c.bytes = c.A + align256(p * (size_t)c.ld * (size_t)c.ld * 8);
    return c;
}

}  // namespace dr
