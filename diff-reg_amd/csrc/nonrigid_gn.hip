// nonrigid_gn.hip -- Gauss-Newton non-rigid ICP on an embedded deformation graph (sixteenth set after ABI 0.7.0):
//   dr_nicp_gn_f32          non_rigid_icp_gauss_newton              2D-3D vision3d/layers/nonrigid_icp.py:18-154
//   dr_nicp_gn_normal_f32   its normal equations at a given state   2D-3D vision3d/layers/nonrigid_icp.py:94-143
//   dr_spd_solve_f64        torch.linalg.solve on an SPD matrix     2D-3D vision3d/layers/nonrigid_icp.py:144
// All are ragged over P pairs, asynchronous on the given stream, read nothing back to the host and use no floating-point atomic (the status words
// take integer ORs): two runs are bit-equal.  The launch sequence depends only on sizes the host states (max_nodes, n_max), so a call can be
// captured on one stream; a kernel finds out on the device whether its pair, block or tile exists.
//
// Every index below comes from nonrigid_gn_index.h / nonrigid_index.h (walked on the host by tools/nonrigid_gn_index_check.cpp).
//
// One iteration: zero A | b; one thread per correspondence writes its scaled residual and, per anchor column, R_a (p - g_a) and the column's
// Jacobian weight; one wave per node walks the node's lists (the Adam solver's, built by the same set-up pass) and accumulates its 6 x 6 blocks --
// lane (i, j) owns one element, the diagonal block in a register, a partner's block by read-modify-write of a row only this wave writes; the
// blocked right-looking Cholesky factorisation (diagonal block in LDS by one workgroup, panel by one workgroup per row block, trailing update
// by one workgroup per 64 x 64 tile); forward and back substitution by one workgroup per pair; one thread per node applies Rodrigues' formula.
// The Jacobian never exists.
#include "nonrigid_lists.h"
#include "nonrigid_gn_index.h"

namespace dr {

struct GnArgs {
    dr_nicp_problem pb;
    NrLists L;
    double* resid;                    // [n_corr, 3] corr_lambda (warp(p) - q)
    int32_t* n6;                      // [P]
    float* rot;                       // [n_nodes, 9] the state the iterations work on (the caller's, or the workspace's)
    float* trn;                       // [n_nodes, 3]
    double* jac;                      // [n_corr, K, 4]
    double* A;                        // [P, ld, ld]
    double* b;                        // [P, ld]
    int ld;
    double lc, la, lm;
    const float* corr_w;              // [n_corr] or NULL
    int32_t* status;
    int resume;
    float* transforms;
};

// a pair that takes part: computed by the set-up pass and not stopped by a failed pivot
__device__ __forceinline__ bool gn_live(const int32_t* n6, const int32_t* status, int pair, int& M) {
    const int n = n6[pair];
    M = n / 6;
    return n > 0 && !(status[pair] & NRG_ST_PIVOT);
}

// ------------------------------------------------------------------------------------------------ set-up
__global__ __launch_bounds__(NR_SOLVER_BLOCK) void gn_setup_kernel(GnArgs G) {
    __shared__ int s_cnt[3 * (NRG_MAX_NODES + 1)];
    __shared__ int s_status;
    const int pair = blockIdx.x, t = threadIdx.x;
    NrPair S;
    const int st = nr_pair_slices(G.pb, pair, S);
    if (st) {                                               // uniform over the workgroup: nothing of the pair is read or written
        if (t == 0) { G.status[pair] = st; G.n6[pair] = 0; }
        return;
    }
    if (t == 0) s_status = 0;
    __syncthreads();
    nr_setup_lists(G.pb, G.L, S, pair, s_cnt, &s_status);
    if (!G.resume) {
        for (int it = t; it < S.M * NR_COMP; it += NR_SOLVER_BLOCK) {
            const int i = it / NR_COMP, comp = it - i * NR_COMP;
            const size_t g = (size_t)(S.m0 + i);
            if (comp < 9) G.rot[g * 9 + comp] = (comp == 0 || comp == 4 || comp == 8) ? 1.f : 0.f;
            else G.trn[g * 3 + comp - 9] = 0.f;
        }
    }
    if (t == 0) { G.status[pair] = s_status; G.n6[pair] = 6 * S.M; }
}

// ------------------------------------------------------------------------------------------------ residuals and Jacobian columns
// one correspondence per thread: :98-112.  The warp is apply_deformation's (all columns != -1, weights over sum + eps), the Jacobian weight is the
// RAW anchor weight (times sqrt(corr_weight)) of the columns with weight > 0; of two such columns that name one node the later one is kept.
__global__ __launch_bounds__(NR_TILE) void gn_prep_kernel(GnArgs G) {
    int pair, tile, M;
    if (!nr_tile_to_pair(G.pb.P, G.pb.c_offsets, G.pb.n_corr, blockIdx.x, pair, tile)) return;
    if (!gn_live(G.n6, G.status, pair, M)) return;
    const int c0 = G.pb.c_offsets[pair], N = G.pb.c_offsets[pair + 1] - c0, m0 = G.pb.m_offsets[pair], K = G.pb.K;
    const int q = tile * NR_TILE + threadIdx.x;
    if (q >= N) return;
    const size_t r = (size_t)(c0 + q);
    const double px = G.pb.src_corr[r * 3], py = G.pb.src_corr[r * 3 + 1], pz = G.pb.src_corr[r * 3 + 2];
    const double cw = G.corr_w ? sqrt((double)G.corr_w[r]) : 1.0;
    double ox = 0.0, oy = 0.0, oz = 0.0;
    for (int k = 0; k < K; ++k) {
        const int a = G.L.anchor[r * K + k];
        double* J = G.jac + (r * K + k) * 4;
        if (a < 0) {
            J[0] = 0.0; J[1] = 0.0; J[2] = 0.0; J[3] = 0.0;
            continue;
        }
        const double w = G.L.weight[r * K + k];
        const float* g = G.pb.nodes + (size_t)(m0 + a) * 3;
        const float* R = G.rot + (size_t)(m0 + a) * 9;
        const float* T = G.trn + (size_t)(m0 + a) * 3;
        const double gx = g[0], gy = g[1], gz = g[2];
        const double dx = px - gx, dy = py - gy, dz = pz - gz;
        const double rx = ((double)R[0] * dx + (double)R[1] * dy) + (double)R[2] * dz;
        const double ry = ((double)R[3] * dx + (double)R[4] * dy) + (double)R[5] * dz;
        const double rz = ((double)R[6] * dx + (double)R[7] * dy) + (double)R[8] * dz;
        ox = ox + ((rx + (double)T[0]) + gx) * w;
        oy = oy + ((ry + (double)T[1]) + gy) * w;
        oz = oz + ((rz + (double)T[2]) + gz) * w;
        const double raw = G.pb.anchor_weights[r * K + k];
        bool keep = raw > 0.0;
        for (int k2 = k + 1; k2 < K; ++k2) keep = keep && !(G.L.anchor[r * K + k2] == a && G.pb.anchor_weights[r * K + k2] > 0.f);
        J[0] = rx; J[1] = ry; J[2] = rz;
        J[3] = keep ? G.lc * (cw * raw) : 0.0;
    }
    G.resid[r * 3] = G.lc * (ox - (double)G.pb.tgt_corr[r * 3]);
    G.resid[r * 3 + 1] = G.lc * (oy - (double)G.pb.tgt_corr[r * 3 + 1]);
    G.resid[r * 3 + 2] = G.lc * (oz - (double)G.pb.tgt_corr[r * 3 + 2]);
}

// ------------------------------------------------------------------------------------------------ assembly
// [d]x element (r, c): 0 -z y | z 0 -x | -y x 0
__device__ __forceinline__ double gn_skew(double d0, double d1, double d2, int r, int c) {
    if (r == c) return 0.0;
    const int k = 3 - r - c;
    const double dk = k == 0 ? d0 : (k == 1 ? d1 : d2);
    return (c == r + 1 || c == r - 2) ? -dk : dk;
}
// element (r, i) of the 3 x 6 block (-w [d]x | w I)
__device__ __forceinline__ double gn_jel(double d0, double d1, double d2, double w, int r, int i) {
    return i < 3 ? -(w * gn_skew(d0, d1, d2, r, i)) : (r == i - 3 ? w : 0.0);
}

// one wave per node n: lane l < 36 owns element (i, j) = (l / 6, l % 6) of n's 6 x 6 blocks, lanes 36 .. 41 component l - 36 of n's right-hand
// side.  The wave walks n's lists in their (ascending) order; the row block n of A is written by this wave alone.
__global__ __launch_bounds__(WAVE) void gn_assemble_kernel(GnArgs G) {
    const int pair = blockIdx.y, n = blockIdx.x, lane = threadIdx.x;
    int M;
    if (!gn_live(G.n6, G.status, pair, M) || n >= M) return;
    const int m0 = G.pb.m_offsets[pair], c0 = G.pb.c_offsets[pair], e0 = G.pb.e_offsets[pair], K = G.pb.K;
    const bool mat = lane < 36, rhs = lane >= 36 && lane < 42;
    const int i = mat ? lane / 6 : (rhs ? lane - 36 : 0), j = mat ? lane - i * 6 : 0;
    double* Arow = G.A + nrg_elem(pair, G.ld, nrg_unknown(M, n, i), 0);
    const size_t rowp = (size_t)m0 + pair + n;
    double acc = 0.0;
    // ---- correspondence rows
    {
        const size_t base = (size_t)c0 * K;
        const int lo = G.L.lm_ptr[rowp], hi = G.L.lm_ptr[rowp + 1];
        int prev = -1;
        for (int e = lo; e < hi; ++e) {
            const int c = G.L.lm_corr[base + e];
            if (c == prev) continue;                        // the row names n twice: its kept column was handled with the first entry
            prev = c;
            const size_t r = (size_t)(c0 + c);
            int kn = -1;
            for (int k = 0; k < K; ++k) kn = (G.L.anchor[r * K + k] == n && G.jac[(r * K + k) * 4 + 3] != 0.0) ? k : kn;
            if (kn < 0) continue;
            const double* Jn = G.jac + (r * K + kn) * 4;
            const double n0 = Jn[0], n1 = Jn[1], n2 = Jn[2], wn = Jn[3];
            if (rhs) {
                acc = acc - ((gn_jel(n0, n1, n2, wn, 0, i) * G.resid[r * 3] + gn_jel(n0, n1, n2, wn, 1, i) * G.resid[r * 3 + 1]) +
                             gn_jel(n0, n1, n2, wn, 2, i) * G.resid[r * 3 + 2]);
            }
            for (int km = 0; km < K; ++km) {
                const int am = G.L.anchor[r * K + km];
                const double* Jm = G.jac + (r * K + km) * 4;
                const double wm = Jm[3];
                if (am < 0 || wm == 0.0) continue;
                if (!mat) continue;
                const double q0 = Jm[0], q1 = Jm[1], q2 = Jm[2];
                const double v = (gn_jel(n0, n1, n2, wn, 0, i) * gn_jel(q0, q1, q2, wm, 0, j) +
                                  gn_jel(n0, n1, n2, wn, 1, i) * gn_jel(q0, q1, q2, wm, 1, j)) +
                                 gn_jel(n0, n1, n2, wn, 2, i) * gn_jel(q0, q1, q2, wm, 2, j);
                if (am == n) acc = acc + v;
                else Arow[nrg_unknown(M, am, j)] += v;
            }
        }
    }
    // ---- ARAP rows: :117-137
    if (G.la > 0.0) {
        const float* gn = G.pb.nodes + (size_t)(m0 + n) * 3;
        const double g0 = gn[0], g1 = gn[1], g2 = gn[2];
        {   // edges n -> v: blocks (-s [R_n (g_v - g_n)]x | s I) at n and (0 | -s I) at v
            const float* R = G.rot + (size_t)(m0 + n) * 9;
            const float* T = G.trn + (size_t)(m0 + n) * 3;
            const int lo = G.L.out_ptr[rowp], hi = G.L.out_ptr[rowp + 1];
            for (int e = lo; e < hi; ++e) {
                const NrAdj ad = G.L.out_adj[e0 + e];
                const int v = ad.other;
                if (v == n) continue;
                const double s = G.la * sqrt((double)ad.weight);
                const float* gv = G.pb.nodes + (size_t)(m0 + v) * 3;
                const float* Tv = G.trn + (size_t)(m0 + v) * 3;
                const double dx = (double)gv[0] - g0, dy = (double)gv[1] - g1, dz = (double)gv[2] - g2;
                const double d0 = ((double)R[0] * dx + (double)R[1] * dy) + (double)R[2] * dz;
                const double d1 = ((double)R[3] * dx + (double)R[4] * dy) + (double)R[5] * dz;
                const double d2 = ((double)R[6] * dx + (double)R[7] * dy) + (double)R[8] * dz;
                if (rhs) {
                    const double r0 = s * ((((d0 + (double)T[0]) + g0) - (double)gv[0]) - (double)Tv[0]);
                    const double r1 = s * ((((d1 + (double)T[1]) + g1) - (double)gv[1]) - (double)Tv[1]);
                    const double r2 = s * ((((d2 + (double)T[2]) + g2) - (double)gv[2]) - (double)Tv[2]);
                    acc = acc - ((gn_jel(d0, d1, d2, s, 0, i) * r0 + gn_jel(d0, d1, d2, s, 1, i) * r1) + gn_jel(d0, d1, d2, s, 2, i) * r2);
                }
                if (mat) {
                    acc = acc + ((gn_jel(d0, d1, d2, s, 0, i) * gn_jel(d0, d1, d2, s, 0, j) +
                                  gn_jel(d0, d1, d2, s, 1, i) * gn_jel(d0, d1, d2, s, 1, j)) +
                                 gn_jel(d0, d1, d2, s, 2, i) * gn_jel(d0, d1, d2, s, 2, j));
                    if (j >= 3) Arow[nrg_unknown(M, v, j)] += -(s * gn_jel(d0, d1, d2, s, j - 3, i));
                }
            }
        }
        {   // edges u -> n: block (0 | -s I) at n against (-s [R_u (g_n - g_u)]x | s I) at u
            const int lo = G.L.in_ptr[rowp], hi = G.L.in_ptr[rowp + 1];
            for (int e = lo; e < hi; ++e) {
                const NrAdj ad = G.L.in_adj[e0 + e];
                const int u = ad.other;
                if (u == n) continue;
                const double s = G.la * sqrt((double)ad.weight);
                const float* gu = G.pb.nodes + (size_t)(m0 + u) * 3;
                const float* R = G.rot + (size_t)(m0 + u) * 9;
                const float* Tu = G.trn + (size_t)(m0 + u) * 3;
                const float* T = G.trn + (size_t)(m0 + n) * 3;
                const double u0 = gu[0], u1 = gu[1], u2 = gu[2];
                const double dx = g0 - u0, dy = g1 - u1, dz = g2 - u2;
                const double d0 = ((double)R[0] * dx + (double)R[1] * dy) + (double)R[2] * dz;
                const double d1 = ((double)R[3] * dx + (double)R[4] * dy) + (double)R[5] * dz;
                const double d2 = ((double)R[6] * dx + (double)R[7] * dy) + (double)R[8] * dz;
                if (rhs && i >= 3) {
                    const double dd = i == 3 ? d0 : (i == 4 ? d1 : d2), tu = Tu[i - 3], uu = i == 3 ? u0 : (i == 4 ? u1 : u2);
                    const double gg = i == 3 ? g0 : (i == 4 ? g1 : g2);
                    const double re = s * ((((dd + tu) + uu) - gg) - (double)T[i - 3]);
                    acc = acc + s * re;
                }
                if (mat && i >= 3) {
                    if (i == j) acc = acc + s * s;
                    Arow[nrg_unknown(M, u, j)] += -(s * gn_jel(d0, d1, d2, s, i - 3, j));
                }
            }
        }
    }
    if (mat) Arow[nrg_unknown(M, n, j)] = i == j ? acc + G.lm : acc;
    if (rhs) G.b[nrg_rhs(pair, G.ld, nrg_unknown(M, n, i))] = acc;
}

// ------------------------------------------------------------------------------------------------ blocked Cholesky
struct SpdArgs {
    double* A;                        // [P, ld, ld]: lower triangle in, factor out
    double* bx;                       // [P, ld]: right-hand side in, solution out
    const int32_t* n;                 // [P] size of each system
    int32_t* status;
    int ld, k;
};

// the size of system p (0: nothing to do -- out of range, or stopped by a failed pivot)
__device__ __forceinline__ int spd_size(const SpdArgs& S, int p) {
    const int n = S.n[p];
    return (n < 0 || n > S.ld || (S.status[p] & NRG_ST_PIVOT)) ? 0 : n;
}

// block k's diagonal tile, one workgroup per system: unblocked Cholesky in LDS.  A pivot that is not finite or not > 0 sets the status bit and
// leaves; every later kernel of the system sees the bit and does nothing.
__global__ __launch_bounds__(256) void spd_diag_kernel(SpdArgs S) {
    __shared__ double s[NRG_B][NRG_B + 1];
    const int p = blockIdx.x, t = threadIdx.x;
    if (S.k == 0 && t == 0 && (S.n[p] < 0 || S.n[p] > S.ld)) atomicOr(&S.status[p], NR_ST_OFFSETS);
    const int np = spd_size(S, p), bw = nrg_block_rows(np, S.k), k0 = S.k * NRG_B;
    if (bw <= 0) return;
    for (int idx = t; idx < NRG_B * NRG_B; idx += 256) {
        const int r = idx / NRG_B, c = idx - r * NRG_B;
        s[r][c] = (r < bw && c <= r) ? S.A[nrg_elem(p, S.ld, k0 + r, k0 + c)] : 0.0;
    }
    __syncthreads();
    const int r = t & (NRG_B - 1), cg = t / NRG_B;
    for (int j = 0; j < bw; ++j) {
        const double piv = s[j][j];
        if (!(piv > 0.0) || !(piv < INFINITY)) {            // uniform: every thread reads the same word
            if (t == 0) atomicOr(&S.status[p], NRG_ST_PIVOT);
            return;
        }
        const double d = sqrt(piv);
        if (cg == 0 && r > j && r < bw) s[r][j] = s[r][j] / d;
        __syncthreads();
        for (int c = j + 1 + cg; c <= r && r < bw; c += 256 / NRG_B) s[r][c] -= s[r][j] * s[c][j];
        __syncthreads();
    }
    for (int idx = t; idx < NRG_B * NRG_B; idx += 256) {
        const int rr = idx / NRG_B, c = idx - rr * NRG_B;
        if (rr < bw && c <= rr) S.A[nrg_elem(p, S.ld, k0 + rr, k0 + c)] = rr == c ? sqrt(s[rr][rr]) : s[rr][c];
    }
}

// the panel below block k: workgroup x of system p solves X L_kk^T = A_ik for row block i = k + 1 + x, one row per thread
__global__ __launch_bounds__(NRG_B) void spd_panel_kernel(SpdArgs S) {
    __shared__ double sL[NRG_B * (NRG_B + 1) / 2];          // L_kk packed by rows: (j, t <= j) at j (j + 1) / 2 + t
    __shared__ double sX[NRG_B][NRG_B];                     // [column][row]
    const int p = blockIdx.y, r = threadIdx.x, bi = S.k + 1 + blockIdx.x, k0 = S.k * NRG_B;
    const int np = spd_size(S, p), rows = nrg_block_rows(np, bi);
    if (rows <= 0) return;
    for (int j = 0; j < NRG_B; ++j)
        if (r <= j) sL[j * (j + 1) / 2 + r] = S.A[nrg_elem(p, S.ld, k0 + j, k0 + r)];
    const bool has = r < rows;
    double* row = S.A + nrg_elem(p, S.ld, bi * NRG_B + (has ? r : 0), k0);
    for (int j = 0; j < NRG_B; ++j) sX[j][r] = has ? row[j] : 0.0;
    __syncthreads();
    for (int j = 0; j < NRG_B; ++j) {
        const double* Lj = sL + j * (j + 1) / 2;
        double acc = sX[j][r];
        for (int t = 0; t < j; ++t) acc -= sX[t][r] * Lj[t];
        sX[j][r] = acc / Lj[j];
    }
    if (has)
        for (int j = 0; j < NRG_B; ++j) row[j] = sX[j][r];
}

// the trailing update of step k: tile (bi, bj), bj <= bi, loses L_ik L_jk^T; 16 x 16 threads, a 4 x 4 patch each, the 64-deep product in two
// halves of 32 through LDS (transposed: [depth][row])
__global__ __launch_bounds__(NRG_UPDATE_T) void spd_update_kernel(SpdArgs S) {
    __shared__ __align__(16) double sI[NRG_B / 2][NRG_TILE_PAD];
    __shared__ __align__(16) double sJ[NRG_B / 2][NRG_TILE_PAD];
    const int p = blockIdx.z, t = threadIdx.x, k0 = S.k * NRG_B;
    const int np = spd_size(S, p);
    int bi, bj;
    if (!nrg_update_tile(np, S.k, blockIdx.x, blockIdx.y, bi, bj)) return;
    const int ri = nrg_block_rows(np, bi), rj = nrg_block_rows(np, bj);
    const int ty = t / 16, tx = t - ty * 16;
    double acc[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = 0.0;
    for (int half = 0; half < 2; ++half) {
        if (half) __syncthreads();
        for (int idx = t; idx < NRG_B * (NRG_B / 2); idx += NRG_UPDATE_T) {
            const int r = idx / (NRG_B / 2), cc = idx - r * (NRG_B / 2);
            const int col = k0 + half * (NRG_B / 2) + cc;
            sI[cc][r] = r < ri ? S.A[nrg_elem(p, S.ld, bi * NRG_B + r, col)] : 0.0;
            sJ[cc][r] = r < rj ? S.A[nrg_elem(p, S.ld, bj * NRG_B + r, col)] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int tt = 0; tt < NRG_B / 2; ++tt) {
            double a[4], b[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) { a[x] = sI[tt][ty * 4 + x]; b[x] = sJ[tt][tx * 4 + x]; }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] += a[x] * b[y];
        }
    }
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int r = ty * 4 + x, c = tx * 4 + y, R = bi * NRG_B + r, C = bj * NRG_B + c;
            if (r < ri && c < rj && C <= R) S.A[nrg_elem(p, S.ld, R, C)] -= acc[x][y];
        }
}

// L y = b, then L^T x = y, one workgroup per system, block by block: the diagonal triangle by wave 0 from LDS, the rows below (forward) or above
// (backward) by all threads.  bx is read and written by this workgroup alone; the barriers order its accesses.
__global__ __launch_bounds__(NRG_SUBST_T) void spd_subst_kernel(SpdArgs S) {
    __shared__ double s[NRG_B][NRG_B + 1];
    __shared__ double sy[NRG_B];
    const int p = blockIdx.x, t = threadIdx.x;
    const int np = spd_size(S, p), nb = nrg_blocks(np);
    if (np <= 0) return;
    double* bx = S.bx + nrg_rhs(p, S.ld, 0);
    for (int pass = 0; pass < 2; ++pass) {
        for (int step = 0; step < nb; ++step) {
            const int kb = pass == 0 ? step : nb - 1 - step, k0 = kb * NRG_B, bw = nrg_block_rows(np, kb);
            for (int idx = t; idx < NRG_B * NRG_B; idx += NRG_SUBST_T) {
                const int r = idx / NRG_B, c = idx - r * NRG_B;
                s[r][c] = (r < bw && c <= r) ? S.A[nrg_elem(p, S.ld, k0 + r, k0 + c)] : 0.0;
            }
            __syncthreads();
            if (t < WAVE) {
                double v = t < bw ? bx[k0 + t] : 0.0;
                if (pass == 0) {
                    for (int j = 0; j < bw; ++j) {
                        const double yj = __shfl(v, j) / s[j][j];
                        if (t == j) v = yj;
                        else if (t > j && t < bw) v -= s[t][j] * yj;
                    }
                } else {
                    for (int j = bw - 1; j >= 0; --j) {
                        const double xj = __shfl(v, j) / s[j][j];
                        if (t == j) v = xj;
                        else if (t < j) v -= s[j][t] * xj;
                    }
                }
                if (t < bw) { bx[k0 + t] = v; sy[t] = v; }
            }
            __syncthreads();
            if (pass == 0) {
                for (int i = k0 + bw + t; i < np; i += NRG_SUBST_T) {
                    const double* row = S.A + nrg_elem(p, S.ld, i, k0);
                    double acc = bx[i];
                    for (int j = 0; j < bw; ++j) acc -= row[j] * sy[j];
                    bx[i] = acc;
                }
            } else {
                for (int i = t; i < k0; i += NRG_SUBST_T) {
                    double acc = bx[i];
                    for (int j = 0; j < bw; ++j) acc -= S.A[nrg_elem(p, S.ld, k0 + j, i)] * sy[j];
                    bx[i] = acc;
                }
            }
            __syncthreads();
        }
    }
}

static int spd_launch(int P, int n_max, const int32_t* n, double* A, double* bx, int32_t* status, hipStream_t st) {
    SpdArgs S = {A, bx, n, status, n_max, 0};
    const int nb = nrg_blocks(n_max);
    for (int k = 0; k < nb; ++k) {
        S.k = k;
        hipLaunchKernelGGL(spd_diag_kernel, dim3((unsigned)P), dim3(256), 0, st, S);
        DR_LAUNCH_CHECK();
        const int rest = nb - k - 1;
        if (rest <= 0) continue;
        hipLaunchKernelGGL(spd_panel_kernel, dim3((unsigned)rest, (unsigned)P), dim3(NRG_B), 0, st, S);
        DR_LAUNCH_CHECK();
        hipLaunchKernelGGL(spd_update_kernel, dim3((unsigned)rest, (unsigned)rest, (unsigned)P), dim3(NRG_UPDATE_T), 0, st, S);
        DR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(spd_subst_kernel, dim3((unsigned)P), dim3(NRG_SUBST_T), 0, st, S);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// ------------------------------------------------------------------------------------------------ update and read-out
// R_n <- exp(phi_n) R_n, t_n <- t_n + dt_n: axis_angle_to_rotation_matrix (so3.py:389-406) with safe_divide's clamp of the angle at 1e-6
// (numeric.py:7-9) and Rodrigues' formula I + sin K + (1 - cos) K^2 (so3.py:107-133), float64 on the float32 state, rounded once
__global__ __launch_bounds__(WAVE) void gn_update_kernel(GnArgs G) {
    const int pair = blockIdx.y, n = blockIdx.x * WAVE + threadIdx.x;
    int M;
    if (!gn_live(G.n6, G.status, pair, M) || n >= M) return;
    const double* x = G.b + nrg_rhs(pair, G.ld, 0);
    const double p0 = x[nrg_unknown(M, n, 0)], p1 = x[nrg_unknown(M, n, 1)], p2 = x[nrg_unknown(M, n, 2)];
    const double theta = sqrt((p0 * p0 + p1 * p1) + p2 * p2), den = theta < 1e-6 ? 1e-6 : theta;
    const double w[3] = {p0 / den, p1 / den, p2 / den};
    const double sn = sin(theta), cs = 1.0 - cos(theta);
    double Kx[3][3], E[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Kx[r][c] = gn_skew(w[0], w[1], w[2], r, c);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double k2 = (Kx[r][0] * Kx[0][c] + Kx[r][1] * Kx[1][c]) + Kx[r][2] * Kx[2][c];
            E[r][c] = ((r == c ? 1.0 : 0.0) + sn * Kx[r][c]) + cs * k2;
        }
    const int m0 = G.pb.m_offsets[pair];
    float* R = G.rot + (size_t)(m0 + n) * 9;
    float* T = G.trn + (size_t)(m0 + n) * 3;
    double old[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) old[e] = R[e];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r * 3 + c] = (float)((E[r][0] * old[c] + E[r][1] * old[3 + c]) + E[r][2] * old[6 + c]);
#pragma unroll
    for (int d = 0; d < 3; ++d) T[d] = (float)((double)T[d] + x[nrg_unknown(M, n, 3 + d)]);
}

// transforms from the state, for every pair the set-up pass computed (a stopped pair included: its state is the one before the failed iteration)
__global__ __launch_bounds__(WAVE) void gn_transform_kernel(GnArgs G) {
    const int pair = blockIdx.y, n = blockIdx.x * WAVE + threadIdx.x;
    const int M = G.n6[pair] / 6;
    if (n >= M) return;
    const int m0 = G.pb.m_offsets[pair];
    const float* R = G.rot + (size_t)(m0 + n) * 9;
    const float* T = G.trn + (size_t)(m0 + n) * 3;
    float* out = G.transforms + (size_t)(m0 + n) * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        out[r * 4] = R[r * 3]; out[r * 4 + 1] = R[r * 3 + 1]; out[r * 4 + 2] = R[r * 3 + 2]; out[r * 4 + 3] = T[r];
    }
    out[12] = 0.f; out[13] = 0.f; out[14] = 0.f; out[15] = 1.f;
}

static bool gn_sizes_ok(long long a) { return a <= 0x7fffffffLL; }

// validation and carve shared by dr_nicp_gn_f32 and dr_nicp_gn_normal_f32; everything is reported before the first launch
static int gn_prepare(const dr_nicp_problem* pb, const dr_nicp_gn_options* op, const float* corr_weights, int32_t* status, void* workspace,
                      size_t workspace_bytes, GnArgs& G, NrGnCarve& c) {
    if (!pb || !op || pb->P < 0 || pb->n_corr < 0 || pb->n_nodes < 0 || pb->n_edges < 0) return DR_EINVAL;
    if (pb->K < 1 || pb->K > NR_MAX_ANCHORS || pb->max_nodes < 0 || pb->max_nodes > NRG_MAX_NODES) return DR_EINVAL;
    if (op->num_iterations < 0) return DR_EINVAL;
    if (!status && pb->P > 0) return DR_EINVAL;
    if (pb->P == 0) return DR_OK;
    if (!pb->m_offsets || !pb->c_offsets || !pb->e_offsets) return DR_EINVAL;
    if (pb->n_nodes > 0 && !pb->nodes) return DR_EINVAL;
    if (pb->n_corr > 0 && (!pb->src_corr || !pb->tgt_corr || !pb->anchor_indices || !pb->anchor_weights)) return DR_EINVAL;
    if (pb->n_edges > 0 && !pb->edges) return DR_EINVAL;     // edge_weights may be NULL: weight 1 (:60-61)
    if (!gn_sizes_ok((long long)pb->n_corr * pb->K * 4) || !gn_sizes_ok((long long)pb->n_nodes * 16 + pb->P) ||
        !gn_sizes_ok((long long)pb->n_edges * 2) || !gn_sizes_ok(nr_grid_bound(pb->n_corr, pb->P)) || pb->P > 65535)
        return DR_ENOSUP;
    c = nrg_carve(pb->P, pb->n_corr, pb->n_nodes, pb->n_edges, pb->K, pb->max_nodes);
    if (!workspace || workspace_bytes < c.bytes) return DR_EWORKSPACE;
    if (!aligned_to(workspace, 16)) return DR_EINVAL;
    char* w = (char*)workspace;
    G.pb = *pb;
    G.L = {(int32_t*)(w + c.lists.anchor), (float*)(w + c.lists.weight), (int32_t*)(w + c.lists.lm_ptr), (int32_t*)(w + c.lists.lm_corr),
           (float4*)(w + c.lists.lm_pw), (int32_t*)(w + c.lists.out_ptr), (NrAdj*)(w + c.lists.out_adj), (int32_t*)(w + c.lists.in_ptr),
           (NrAdj*)(w + c.lists.in_adj)};
    G.resid = (double*)(w + c.lists.resid);
    G.n6 = (int32_t*)(w + c.n6);
    G.rot = (float*)(w + c.rot); G.trn = (float*)(w + c.trn);
    G.jac = (double*)(w + c.jac);
    G.A = (double*)(w + c.A); G.b = (double*)(w + c.b);
    G.ld = c.ld;
    G.lc = op->corr_lambda; G.la = op->arap_lambda; G.lm = op->lm_lambda;
    G.corr_w = corr_weights;
    G.status = status;
    return DR_OK;
}

// zero A | b, residuals and Jacobian columns, assembly: one iteration's normal equations at the state G.rot / G.trn
static int gn_normal_equations(const GnArgs& G, hipStream_t st) {
    const int P = G.pb.P;
    DR_HIP_CHECK(hipMemsetAsync(G.A, 0, (size_t)P * G.ld * G.ld * sizeof(double), st));
    DR_HIP_CHECK(hipMemsetAsync(G.b, 0, (size_t)P * G.ld * sizeof(double), st));
    if (G.pb.n_corr > 0) {
        hipLaunchKernelGGL(gn_prep_kernel, dim3((unsigned)nr_grid_bound(G.pb.n_corr, P)), dim3(NR_TILE), 0, st, G);
        DR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gn_assemble_kernel, dim3((unsigned)G.pb.max_nodes, (unsigned)P), dim3(WAVE), 0, st, G);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // namespace dr

using namespace dr;

extern "C" {

size_t dr_nicp_gn_workspace_bytes(int P, int n_corr, int n_nodes, int n_edges, int K, int max_nodes) {
    return nrg_carve(P, n_corr, n_nodes, n_edges, K, max_nodes).bytes;
}

int dr_nicp_gn_f32(const dr_nicp_problem* problem, const dr_nicp_gn_options* options, const float* corr_weights, const dr_nicp_state* state,
                   int resume, float* transforms, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    GnArgs G = {};
    NrGnCarve c;
    if (problem && problem->n_nodes > 0 && !transforms) return DR_EINVAL;
    if (problem && resume && problem->n_nodes > 0 && (!state || !state->rotations || !state->translations)) return DR_EINVAL;
    const int rc = gn_prepare(problem, options, corr_weights, status, workspace, workspace_bytes, G, c);
    if (rc != DR_OK || problem->P == 0) return rc;
    if (state && state->rotations) G.rot = state->rotations;
    if (state && state->translations) G.trn = state->translations;
    G.resume = resume ? 1 : 0;
    G.transforms = transforms;
    hipStream_t st = (hipStream_t)stream;
    const int P = problem->P;
    hipLaunchKernelGGL(gn_setup_kernel, dim3((unsigned)P), dim3(NR_SOLVER_BLOCK), 0, st, G);
    DR_LAUNCH_CHECK();
    if (problem->max_nodes == 0) return DR_OK;
    const dim3 node_grid((unsigned)((problem->max_nodes + WAVE - 1) / WAVE), (unsigned)P);
    for (int it = 0; it < options->num_iterations; ++it) {
        int r2 = gn_normal_equations(G, st);
        if (r2 != DR_OK) return r2;
        r2 = spd_launch(P, G.ld, G.n6, G.A, G.b, status, st);
        if (r2 != DR_OK) return r2;
        hipLaunchKernelGGL(gn_update_kernel, node_grid, dim3(WAVE), 0, st, G);
        DR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(gn_transform_kernel, node_grid, dim3(WAVE), 0, st, G);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_nicp_gn_normal_f32(const dr_nicp_problem* problem, const dr_nicp_gn_options* options, const float* corr_weights, const float* rotations,
                          const float* translations, double* A, double* b, int32_t* status, void* workspace, size_t workspace_bytes,
                          void* stream) {
    GnArgs G = {};
    NrGnCarve c;
    if (problem && problem->n_nodes > 0 && (!rotations || !translations)) return DR_EINVAL;
    if (problem && problem->P > 0 && problem->max_nodes > 0 && (!A || !b)) return DR_EINVAL;
    const int rc = gn_prepare(problem, options, corr_weights, status, workspace, workspace_bytes, G, c);
    if (rc != DR_OK || problem->P == 0) return rc;
    G.rot = const_cast<float*>(rotations);                  // read only: resume keeps the set-up pass from writing a state
    G.trn = const_cast<float*>(translations);
    G.resume = 1;
    G.A = A; G.b = b;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_setup_kernel, dim3((unsigned)problem->P), dim3(NR_SOLVER_BLOCK), 0, st, G);
    DR_LAUNCH_CHECK();
    if (problem->max_nodes == 0) return DR_OK;
    return gn_normal_equations(G, st);
}

int dr_spd_solve_f64(int P, int n_max, const int32_t* n, double* A, double* bx, int32_t* status, void* stream) {
    if (P < 0 || n_max < 0 || n_max > NRG_MAX_N) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (P > 65535) return DR_ENOSUP;
    if (!n || !status || (n_max > 0 && (!A || !bx))) return DR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    DR_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)P * sizeof(int32_t), st));
    if (n_max == 0) return DR_OK;
    return spd_launch(P, n_max, n, A, bx, status, st);
}

}  // extern "C"
