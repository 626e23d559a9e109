// nonrigid.hip -- non-rigid ICP on an embedded deformation graph (fourteenth set after ABI 0.7.0):
//   dr_ed_graph_f32         build_euclidean_deformation_graph      2D-3D vision3d/ops/deformation_graph.py:26-103
//   dr_ed_warp_f32          apply_deformation                      2D-3D vision3d/ops/embedded_deformation.py:31-66
//   dr_nicp_cost_grad_f32   compute_cost_function + backward       2D-3D vision3d/ops/nonrigid_icp_adam.py:9-73
//   dr_nicp_adam_f32        non_rigid_icp_adam                     2D-3D vision3d/ops/nonrigid_icp_adam.py:76-131
// All are ragged over P pairs (offset arrays of P + 1 int32 entries on the device), asynchronous on the given stream, and read nothing back to
// the host.  The only atomics are integer ORs (adjacency bit map, status words) and one integer add (edge count): two runs are bit-equal.
//
// Every index below comes from nonrigid_index.h (walked on the host by tools/nonrigid_index_check.cpp).
//
// The solver runs all iterations of a pair in one workgroup of NR_SOLVER_BLOCK threads.  Rotation | translation (two copies), exp_avg and
// exp_avg_sq of every node stay in LDS for the whole run.  Thread (node, component) owns one of the node's 12 parameters: it gathers that
// parameter's gradient through the node-major lists of the set-up pass (correspondences anchored at the node, edges that leave it, edges that
// enter it), in float64 and in list order, rounds it once, and applies Adam to its own parameter -- reading the state of this iteration from one
// copy and writing the next into the other.  An iteration therefore has TWO barriers: after the per-correspondence residuals are written (they
// live in the workspace), and after the update.
#include "nonrigid_lists.h"      // status bits, NrPair, NrAdj and the set-up pass shared with nonrigid_gn.hip

// the float64 sums below are written operation by operation; nothing becomes an FMA behind the statement
#pragma clang fp contract(off)

namespace dr {

// exp(-d^2 / (2 c^2)), compute_skinning_weights (deformation_graph.py:22)
__device__ __forceinline__ double nr_skin(double d, double c) { return exp(-(d * d) / (2.0 * (c * c))); }

// pairwise_distance(nodes, nodes, squared=False) of pairwise_distance.py:51-58: sqrt(max(|a|^2 - 2 a.b + |b|^2, 0) + 1e-8)
__device__ __forceinline__ double nr_node_distance(const float* __restrict__ a, const float* __restrict__ b) {
    const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
    const double a2 = (ax * ax + ay * ay) + az * az, b2 = (bx * bx + by * by) + bz * bz, ab = (ax * bx + ay * by) + az * bz;
    double d2 = (a2 - 2.0 * ab) + b2;
    d2 = d2 < 0.0 ? 0.0 : d2;
    return sqrt(d2 + 1e-8);
}

// ------------------------------------------------------------------------------------------------ graph
struct GraphArgs {
    int P, n_points, n_nodes, K;
    const float* points;
    const int32_t* p_off;
    const float* nodes;
    const int32_t* m_off;
    double coverage, eps;
    long long* anchor_idx;
    float* anchor_w;
    float* anchor_d;
    int32_t* edge_counts;
    const int32_t* e_off;
    long long edge_cap;
    long long* edge_idx;
    float* edge_w;
    float* edge_d;
    int32_t* status;
    uint32_t* bitmap;
    int32_t* row_count;
    double* row_sum;
    int words, max_nodes;
};

// per pair: 0, or the status bits that keep it from being computed
__device__ __forceinline__ int nr_graph_status(const GraphArgs& A, int pair, int& p0, int& N, int& m0, int& M) {
    const int pl = A.p_off[pair], ph = A.p_off[pair + 1], ml = A.m_off[pair], mh = A.m_off[pair + 1];
    if (!nr_slice_ok(pl, ph, A.n_points) || !nr_slice_ok(ml, mh, A.n_nodes)) return NR_ST_OFFSETS;
    p0 = pl; N = ph - pl; m0 = ml; M = mh - ml;
    return ((N > 0 && M == 0) || M > A.max_nodes) ? NR_ST_NODES : 0;
}

// one point per thread; the pair's nodes stream through LDS in stages; the K nearest are kept sorted by insertion (a candidate of equal d^2
// goes behind the ones already there, which have lower indices)
__global__ __launch_bounds__(NR_TILE) void ed_anchor_kernel(GraphArgs A) {
    __shared__ float4 s_node[NR_STAGE];
    int pair, tile;
    if (!nr_tile_to_pair(A.P, A.p_off, A.n_points, blockIdx.x, pair, tile)) return;
    int p0 = 0, N = 0, m0 = 0, M = 0;
    if (nr_graph_status(A, pair, p0, N, m0, M)) return;
    const int t = threadIdx.x, q = tile * NR_TILE + t;
    const bool active = q < N;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (active) {
        const float* p = A.points + (size_t)(p0 + q) * 3;
        px = p[0]; py = p[1]; pz = p[2];
    }
    double bd[NR_MAX_ANCHORS];
    int bi[NR_MAX_ANCHORS];
#pragma unroll
    for (int s = 0; s < NR_MAX_ANCHORS; ++s) { bd[s] = INFINITY; bi[s] = -1; }
    for (int k0 = 0; k0 < M; k0 += NR_STAGE) {
        const int nk = nr_stage_count(M, k0);
        for (int k = t; k < nk; k += NR_TILE) {
            const float* g = A.nodes + (size_t)(m0 + k0 + k) * 3;
            s_node[k] = make_float4(g[0], g[1], g[2], 0.f);
        }
        __syncthreads();
        if (active) {
            for (int k = 0; k < nk; ++k) {
                const float4 g = s_node[k];
                const double dx = px - (double)g.x, dy = py - (double)g.y, dz = pz - (double)g.z;
                double cd = (dx * dx + dy * dy) + dz * dz;
                if (!(cd < bd[NR_MAX_ANCHORS - 1])) continue;
                int ci = k0 + k;
                bool moved = false;
#pragma unroll
                for (int s = 0; s < NR_MAX_ANCHORS; ++s) {
                    if (moved || cd < bd[s]) {
                        const double td = bd[s]; bd[s] = cd; cd = td;
                        const int ti = bi[s]; bi[s] = ci; ci = ti;
                        moved = true;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    // a slot is filled only by a finite distance: a NaN or Inf coordinate (of the point or of a node) never enters the list, so a point may hold
    // fewer than min(K, M) anchors.  Filled slots come first; only they get a weight, a bit in the map, and a share of the row's sum.
    const int Ke = nr_effective_k(A.K, M);
    int filled = 0;
#pragma unroll
    for (int s = 0; s < NR_MAX_ANCHORS; ++s) filled += (s < Ke && bi[s] >= 0 && bi[s] < M) ? 1 : 0;
    double w[NR_MAX_ANCHORS], sum = 0.0;
#pragma unroll
    for (int s = 0; s < NR_MAX_ANCHORS; ++s) {
        w[s] = 0.0;
        if (s < filled) {
            w[s] = nr_skin(sqrt(bd[s]), A.coverage);
            sum = sum + w[s];
        }
    }
    const size_t row = (size_t)(p0 + q) * A.K;
#pragma unroll
    for (int s = 0; s < NR_MAX_ANCHORS; ++s) {
        if (s >= A.K) continue;
        const bool has = s < filled;
        A.anchor_idx[row + s] = has ? bi[s] : -1;
        A.anchor_w[row + s] = has ? (float)(w[s] / sum) : 0.f;
        if (A.anchor_d) A.anchor_d[row + s] = has ? (float)sqrt(bd[s]) : 0.f;
    }
    if (filled < Ke) atomicOr(&A.status[pair], NR_ST_NONFINITE);
    // two nodes that anchor this point are adjacent (both directions and the self edges come out of the double loop)
#pragma unroll
    for (int a = 0; a < NR_MAX_ANCHORS; ++a) {
#pragma unroll
        for (int b = 0; b < NR_MAX_ANCHORS; ++b) {
            if (a < filled && b < filled) atomicOr(&A.bitmap[nr_bitmap_word(m0, bi[a], A.words, bi[b])], nr_bitmap_bit(bi[b]));
        }
    }
}

// one workgroup per pair, one adjacency row per thread: the row's set bits and the sum of its skinning weights in ascending column order
__global__ __launch_bounds__(NR_EDGE_BLOCK) void ed_edge_count_kernel(GraphArgs A) {
    __shared__ int s_total;
    const int pair = blockIdx.x, t = threadIdx.x;
    int p0 = 0, N = 0, m0 = 0, M = 0;
    const int st = nr_graph_status(A, pair, p0, N, m0, M);
    if (t == 0) s_total = 0;
    __syncthreads();
    int mine = 0;
    if (!st) {
        const int wu = nr_bitmap_words(M);
        for (int i = t; i < M; i += NR_EDGE_BLOCK) {
            int cnt = 0;
            double sum = 0.0;
            for (int wd = 0; wd < wu; ++wd) {
                uint32_t bits = A.bitmap[nr_bitmap_word(m0, i, A.words, wd * 32)];
                cnt += __popc(bits);
                while (bits) {
                    const int j = wd * 32 + __ffs(bits) - 1;
                    bits &= bits - 1;
                    if (j < M) sum = sum + nr_skin(nr_node_distance(A.nodes + (size_t)(m0 + i) * 3, A.nodes + (size_t)(m0 + j) * 3), A.coverage);
                }
            }
            A.row_count[m0 + i] = cnt;
            A.row_sum[m0 + i] = sum;
            mine += cnt;
        }
    }
    if (mine) atomicAdd(&s_total, mine);
    __syncthreads();
    if (t == 0) {
        A.edge_counts[pair] = s_total;
        if (st) atomicOr(&A.status[pair], st);
    }
}

// one workgroup per pair walks the rows in ascending order, NR_EDGE_BLOCK at a time; a row's edges start behind all edges of the rows before it
__global__ __launch_bounds__(NR_EDGE_BLOCK) void ed_edge_write_kernel(GraphArgs A) {
    __shared__ int s_wave[NR_EDGE_BLOCK / WAVE];
    const int pair = blockIdx.x, t = threadIdx.x;
    int p0 = 0, N = 0, m0 = 0, M = 0;
    if (nr_graph_status(A, pair, p0, N, m0, M)) return;
    const long long e_lo = A.e_off[pair], e_hi_raw = A.e_off[pair + 1];
    const long long e_hi = e_hi_raw < A.edge_cap ? e_hi_raw : A.edge_cap;
    if (e_lo < 0) return;
    const int wu = nr_bitmap_words(M);
    long long base = e_lo;
    for (int r0 = 0; r0 < M; r0 += NR_EDGE_BLOCK) {
        const int i = r0 + t;
        const int cnt = i < M ? A.row_count[m0 + i] : 0;
        int incl = cnt;                                     // inclusive prefix inside the wave
#pragma unroll
        for (int d = 1; d < WAVE; d <<= 1) {
            const int o = __shfl_up(incl, d);
            if (lane_id() >= d) incl += o;
        }
        if (lane_id() == WAVE - 1) s_wave[wave_id()] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NR_EDGE_BLOCK / WAVE; ++w) {
            const int c = s_wave[w];
            before += w < wave_id() ? c : 0;
            total += c;
        }
        if (i < M) {
            long long e = base + before + (incl - cnt);
            const double rs = A.row_sum[m0 + i];
            const double den = rs < A.eps ? A.eps : rs;     // .clamp(min=eps)
            for (int wd = 0; wd < wu; ++wd) {
                uint32_t bits = A.bitmap[nr_bitmap_word(m0, i, A.words, wd * 32)];
                while (bits) {
                    const int j = wd * 32 + __ffs(bits) - 1;
                    bits &= bits - 1;
                    if (e >= e_lo && e < e_hi) {
                        const double d = j < M ? nr_node_distance(A.nodes + (size_t)(m0 + i) * 3, A.nodes + (size_t)(m0 + j) * 3) : 0.0;
                        A.edge_idx[2 * e] = i;
                        A.edge_idx[2 * e + 1] = j;
                        A.edge_w[e] = (float)(nr_skin(d, A.coverage) / den);
                        if (A.edge_d) A.edge_d[e] = (float)d;
                    }
                    ++e;
                }
            }
        }
        base += total;
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ warp
struct WarpArgs {
    int P, n_points, n_nodes, K;
    const float* points;
    const int32_t* p_off;
    const float* nodes;
    const int32_t* m_off;
    const float* transforms;
    const long long* anchor_idx;
    const float* anchor_w;
    double eps;
    float* out;
    int32_t* status;
};

__global__ __launch_bounds__(NR_TILE) void ed_warp_kernel(WarpArgs A) {
    int pair, tile;
    if (!nr_tile_to_pair(A.P, A.p_off, A.n_points, blockIdx.x, pair, tile)) return;
    const int p0 = A.p_off[pair], N = A.p_off[pair + 1] - p0;          // usable: nr_tile_to_pair gives an unusable pair no tile
    const int ml = A.m_off[pair], mh = A.m_off[pair + 1];
    if (!nr_slice_ok(ml, mh, A.n_nodes)) {
        if (threadIdx.x == 0 && tile == 0) atomicOr(&A.status[pair], NR_ST_OFFSETS);
        return;
    }
    const int M = mh - ml, q = tile * NR_TILE + threadIdx.x;
    if (q >= N) return;
    const size_t r = (size_t)(p0 + q);
    const double px = A.points[r * 3], py = A.points[r * 3 + 1], pz = A.points[r * 3 + 2];
    double sum = 0.0;
    for (int k = 0; k < A.K; ++k) sum = sum + (double)A.anchor_w[r * A.K + k];
    sum = sum + A.eps;
    double ox = 0.0, oy = 0.0, oz = 0.0;
    bool bad = false;
    for (int k = 0; k < A.K; ++k) {
        const long long a = A.anchor_idx[r * A.K + k];
        if (a < 0 || a >= M) {
            bad = bad || a != -1;
            continue;
        }
        const double w = (double)A.anchor_w[r * A.K + k] / sum;
        const float* g = A.nodes + (size_t)(ml + a) * 3;
        const float* T = A.transforms + (size_t)(ml + a) * 16;
        const double dx = px - (double)g[0], dy = py - (double)g[1], dz = pz - (double)g[2];
        const double x = ((((double)T[0] * dx + (double)T[1] * dy) + (double)T[2] * dz) + (double)T[3]) + (double)g[0];
        const double y = ((((double)T[4] * dx + (double)T[5] * dy) + (double)T[6] * dz) + (double)T[7]) + (double)g[1];
        const double z = ((((double)T[8] * dx + (double)T[9] * dy) + (double)T[10] * dz) + (double)T[11]) + (double)g[2];
        ox = ox + x * w; oy = oy + y * w; oz = oz + z * w;
    }
    A.out[r * 3] = (float)ox; A.out[r * 3 + 1] = (float)oy; A.out[r * 3 + 2] = (float)oz;
    if (bad) atomicOr(&A.status[pair], NR_ST_INDEX);
}

// ------------------------------------------------------------------------------------------------ solver
struct NicpArgs {
    dr_nicp_problem pb;
    // workspace
    double* resid;
    int32_t* anchor;
    float* weight;
    int32_t* lm_ptr;
    int32_t* lm_corr;
    float4* lm_pw;
    int32_t* out_ptr;
    NrAdj* out_adj;
    int32_t* in_ptr;
    NrAdj* in_adj;
    // options
    int iters;
    double lr, gamma, beta1, beta2, eps, wl, wa, wo;
    // state in / out
    dr_nicp_state st;
    int resume;
    // outputs
    float* transforms;
    float* cost;
    float* trace;
    float* grad_rot;
    float* grad_trn;
    int32_t* status;
    int grad_only;                    // dr_nicp_cost_grad_f32: one gradient at the given state, no update
    NrLdsCarve lds;
};

// the warped correspondence c minus its target (compute_landmark_cost's difference), float64 on the LDS state `par`
__device__ __forceinline__ void nr_residual(const NicpArgs& A, const NrPair& S, const float* par, const float* nd, int c, double& rx, double& ry,
                                            double& rz) {
    const size_t r = (size_t)(S.c0 + c);
    const double px = A.pb.src_corr[r * 3], py = A.pb.src_corr[r * 3 + 1], pz = A.pb.src_corr[r * 3 + 2];
    double ox = 0.0, oy = 0.0, oz = 0.0;
    for (int k = 0; k < S.K; ++k) {
        const int a = A.anchor[r * S.K + k];
        if (a < 0) continue;
        const double w = A.weight[r * S.K + k];
        const float* T = par + a * NR_COMP;
        const float* g = nd + a * 3;
        const double gx = g[0], gy = g[1], gz = g[2];
        const double dx = px - gx, dy = py - gy, dz = pz - gz;
        const double x = ((((double)T[0] * dx + (double)T[1] * dy) + (double)T[2] * dz) + (double)T[9]) + gx;
        const double y = ((((double)T[3] * dx + (double)T[4] * dy) + (double)T[5] * dz) + (double)T[10]) + gy;
        const double z = ((((double)T[6] * dx + (double)T[7] * dy) + (double)T[8] * dz) + (double)T[11]) + gz;
        ox = ox + x * w; oy = oy + y * w; oz = oz + z * w;
    }
    rx = ox - (double)A.pb.tgt_corr[r * 3];
    ry = oy - (double)A.pb.tgt_corr[r * 3 + 1];
    rz = oz - (double)A.pb.tgt_corr[r * 3 + 2];
}

// component a of the ARAP difference of the edge i -> j (compute_arap_cost): (R_i (g_j - g_i) + g_i + t_i) - (g_j + t_j)
__device__ __forceinline__ double nr_arap_diff(const float* par, const float* nd, int i, int j, int a) {
    const float* T = par + i * NR_COMP;
    const double dx = (double)nd[j * 3] - (double)nd[i * 3], dy = (double)nd[j * 3 + 1] - (double)nd[i * 3 + 1],
                 dz = (double)nd[j * 3 + 2] - (double)nd[i * 3 + 2];
    const double rot = ((double)T[a * 3] * dx + (double)T[a * 3 + 1] * dy) + (double)T[a * 3 + 2] * dz;
    return ((rot + (double)nd[i * 3 + a]) + (double)T[9 + a]) - ((double)nd[j * 3 + a] + (double)par[j * NR_COMP + 9 + a]);
}

// the three cost terms at the LDS state `par`: every thread returns the same values.  Two barriers; the caller's threads all take part.
__device__ void nr_cost_terms(const NicpArgs& A, const NrPair& S, const float* par, const float* nd, double* red, double out[3]) {
    const int t = threadIdx.x;
    double lm = 0.0, ar = 0.0, orth = 0.0;
    for (int c = t; c < S.N; c += NR_SOLVER_BLOCK) {
        double rx, ry, rz;
        nr_residual(A, S, par, nd, c, rx, ry, rz);
        lm = lm + ((rx * rx + ry * ry) + rz * rz);
    }
    for (int e = t; e < S.E; e += NR_SOLVER_BLOCK) {
        const long long i = A.pb.edges[(size_t)(S.e0 + e) * 2], j = A.pb.edges[(size_t)(S.e0 + e) * 2 + 1];
        if (i < 0 || i >= S.M || j < 0 || j >= S.M) continue;
        const double d0 = nr_arap_diff(par, nd, (int)i, (int)j, 0), d1 = nr_arap_diff(par, nd, (int)i, (int)j, 1),
                     d2 = nr_arap_diff(par, nd, (int)i, (int)j, 2);
        ar = ar + ((d0 * d0 + d1 * d1) + d2 * d2) * (double)A.pb.edge_weights[S.e0 + e];
    }
    for (int i = t; i < S.M; i += NR_SOLVER_BLOCK) {
        const float* T = par + i * NR_COMP;
        double col[3][3];
#pragma unroll
        for (int b = 0; b < 3; ++b)
#pragma unroll
            for (int a = 0; a < 3; ++a) col[b][a] = T[a * 3 + b];
        const double o12 = (col[0][0] * col[1][0] + col[0][1] * col[1][1]) + col[0][2] * col[1][2];
        const double o13 = (col[0][0] * col[2][0] + col[0][1] * col[2][1]) + col[0][2] * col[2][2];
        const double o23 = (col[1][0] * col[2][0] + col[1][1] * col[2][1]) + col[1][2] * col[2][2];
        const double u1 = ((col[0][0] * col[0][0] + col[0][1] * col[0][1]) + col[0][2] * col[0][2]) - 1.0;
        const double u2 = ((col[1][0] * col[1][0] + col[1][1] * col[1][1]) + col[1][2] * col[1][2]) - 1.0;
        const double u3 = ((col[2][0] * col[2][0] + col[2][1] * col[2][1]) + col[2][2] * col[2][2]) - 1.0;
        orth = orth + (((((o12 * o12 + o13 * o13) + o23 * o23) + u1 * u1) + u2 * u2) + u3 * u3);
    }
    lm = wave_sum(lm); ar = wave_sum(ar); orth = wave_sum(orth);
    if (lane_id() == 0) {
        red[wave_id() * 3] = lm; red[wave_id() * 3 + 1] = ar; red[wave_id() * 3 + 2] = orth;
    }
    __syncthreads();
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int w = 0; w < NR_SOLVER_BLOCK / WAVE; ++w) {
        s0 = s0 + red[w * 3]; s1 = s1 + red[w * 3 + 1]; s2 = s2 + red[w * 3 + 2];
    }
    out[0] = s0 / (double)S.N; out[1] = s1 / (double)S.E; out[2] = s2 / (double)S.M;
    __syncthreads();
}

// d(w_l landmark + w_a arap + w_o ortho) / d(parameter `item` = node * 12 + component) at the LDS state `par`, from the residuals in the workspace
__device__ __forceinline__ float nr_gradient(const NicpArgs& A, const NrPair& S, const float* par, const float* nd, int item) {
    const int i = item / NR_COMP, comp = item - i * NR_COMP;
    const bool rot = comp < 9;
    const int a = rot ? comp / 3 : comp - 9, b = rot ? comp - a * 3 : 0;
    const size_t rowp = (size_t)S.m0 + blockIdx.x + i;
    const double gb = nd[i * 3 + b];
    // landmark: sum_c w_c r_c[a] (p_c - g_i)[b]  (rotation)  or  sum_c w_c r_c[a]  (translation), times 2 / N
    double gl = 0.0;
    {
        const size_t base = (size_t)S.c0 * S.K;
        const int lo = A.lm_ptr[rowp], hi = A.lm_ptr[rowp + 1];
        for (int e = lo; e < hi; ++e) {
            const int c = A.lm_corr[base + e];
            const float4 pw = A.lm_pw[base + e];
            const double r = A.resid[(size_t)(S.c0 + c) * 3 + a];
            const double pb = b == 0 ? pw.x : (b == 1 ? pw.y : pw.z);
            const double term = (double)pw.w * r;
            gl = gl + (rot ? term * (pb - gb) : term);
        }
        gl = gl * (2.0 / (double)S.N);
    }
    // ARAP: edges i -> j give +w e[a] (g_j - g_i)[b] to R_i and +w e[a] to t_i; edges k -> i give -w e[a] to t_i; times 2 / E
    double ga = 0.0;
    {
        const int lo = A.out_ptr[rowp], hi = A.out_ptr[rowp + 1];
        for (int e = lo; e < hi; ++e) {
            const NrAdj ad = A.out_adj[S.e0 + e];
            const double d = nr_arap_diff(par, nd, i, ad.other, a) * (double)ad.weight;
            ga = ga + (rot ? d * ((double)nd[ad.other * 3 + b] - gb) : d);
        }
        if (!rot) {
            const int li = A.in_ptr[rowp], hi2 = A.in_ptr[rowp + 1];
            for (int e = li; e < hi2; ++e) {
                const NrAdj ad = A.in_adj[S.e0 + e];
                ga = ga - nr_arap_diff(par, nd, ad.other, i, a) * (double)ad.weight;
            }
        }
        ga = ga * (2.0 / (double)S.E);
    }
    // orthogonality: column b of R_i against itself (unit) and the two others, over M
    double go = 0.0;
    if (rot) {
        const float* T = par + i * NR_COMP;
        for (int b2 = 0; b2 < 3; ++b2) {
            const double dot = ((double)T[b] * (double)T[b2] + (double)T[3 + b] * (double)T[3 + b2]) + (double)T[6 + b] * (double)T[6 + b2];
            go = go + (b2 == b ? 4.0 * (dot - 1.0) : 2.0 * dot) * (double)T[a * 3 + b2];
        }
        go = go / (double)S.M;
    }
    return (float)((A.wl * gl + A.wa * ga) + A.wo * go);
}

__global__ __launch_bounds__(NR_SOLVER_BLOCK) void nicp_kernel(NicpArgs A) {
    extern __shared__ __align__(16) float s_mem[];
    const int pair = blockIdx.x, t = threadIdx.x;
    NrPair S;
    {
        const int ml = A.pb.m_offsets[pair], mh = A.pb.m_offsets[pair + 1], cl = A.pb.c_offsets[pair], ch = A.pb.c_offsets[pair + 1];
        const int el = A.pb.e_offsets[pair], eh = A.pb.e_offsets[pair + 1];
        int st = 0;
        if (!nr_slice_ok(ml, mh, A.pb.n_nodes) || !nr_slice_ok(cl, ch, A.pb.n_corr) || !nr_slice_ok(el, eh, A.pb.n_edges)) st = NR_ST_OFFSETS;
        else if (mh - ml > A.pb.max_nodes) st = NR_ST_NODES;
        if (st) {                                           // uniform over the workgroup: nothing of the pair is read or written
            if (t == 0) A.status[pair] = st;
            return;
        }
        S.m0 = ml; S.M = mh - ml; S.c0 = cl; S.N = ch - cl; S.e0 = el; S.E = eh - el; S.K = A.pb.K;
    }
    float* cur = s_mem + A.lds.param0;
    float* nxt = s_mem + A.lds.param1;
    float* mo = s_mem + A.lds.exp_avg;
    float* vo = s_mem + A.lds.exp_avg_sq;
    float* nd = s_mem + A.lds.node;
    double* red = (double*)((char*)s_mem + A.lds.reduce_byte);
    int* s_status = (int*)((char*)s_mem + A.lds.status_byte);
    const int items = S.M * NR_COMP;
    const bool resume = A.resume != 0;

    // ---- set-up: nodes and state into LDS, anchors narrowed and weights normalised into the workspace
    if (t == 0) *s_status = 0;
    for (int k = t; k < S.M * 3; k += NR_SOLVER_BLOCK) nd[k] = A.pb.nodes[(size_t)S.m0 * 3 + k];
    for (int it = t; it < items; it += NR_SOLVER_BLOCK) {
        const int i = it / NR_COMP, comp = it - i * NR_COMP;
        const size_t g = (size_t)(S.m0 + i);
        const bool rot = comp < 9;
        float p = (comp == 0 || comp == 4 || comp == 8) ? 1.f : 0.f, m = 0.f, v = 0.f;
        if (resume) {
            p = rot ? A.st.rotations[g * 9 + comp] : A.st.translations[g * 3 + comp - 9];
            const float* ms = rot ? A.st.exp_avg_rot : A.st.exp_avg_trn;
            const float* vs = rot ? A.st.exp_avg_sq_rot : A.st.exp_avg_sq_trn;
            if (ms) m = rot ? ms[g * 9 + comp] : ms[g * 3 + comp - 9];
            if (vs) v = rot ? vs[g * 9 + comp] : vs[g * 3 + comp - 9];
        }
        cur[it] = p; mo[it] = m; vo[it] = v;
    }
    __syncthreads();
    // ---- set-up: the anchors, weights and node-major lists of the workspace (nonrigid_lists.h).  The counts and row starts pass through the LDS
    // of the second parameter copy, which no one reads before an iteration has written all of it: 3 (M + 1) <= 12 M ints for M >= 1.
    {
        const NrLists L = {A.anchor, A.weight, A.lm_ptr, A.lm_corr, A.lm_pw, A.out_ptr, A.out_adj, A.in_ptr, A.in_adj};
        nr_setup_lists(A.pb, L, S, pair, (int*)nxt, s_status);
    }

    if (A.grad_only) {
        for (int c = t; c < S.N; c += NR_SOLVER_BLOCK) {
            double rx, ry, rz;
            nr_residual(A, S, cur, nd, c, rx, ry, rz);
            double* r = A.resid + (size_t)(S.c0 + c) * 3;
            r[0] = rx; r[1] = ry; r[2] = rz;
        }
        __syncthreads();
        for (int it = t; it < items; it += NR_SOLVER_BLOCK) {
            const int i = it / NR_COMP, comp = it - i * NR_COMP;
            const float g = nr_gradient(A, S, cur, nd, it);
            if (comp < 9) A.grad_rot[(size_t)(S.m0 + i) * 9 + comp] = g;
            else A.grad_trn[(size_t)(S.m0 + i) * 3 + comp - 9] = g;
        }
        double terms[3];
        nr_cost_terms(A, S, cur, nd, red, terms);
        if (t < 3) A.cost[pair * 3 + t] = (float)terms[t];
        if (t == 0) A.status[pair] = *s_status;
        return;
    }

    // ---- the iterations
    int step0 = (resume && A.st.step) ? A.st.step[pair] : 0;
    if (step0 < 0) {                                        // uniform over the workgroup
        step0 = 0;
        if (t == 0) atomicOr(s_status, NR_ST_STEP);
    }
    double lr = A.lr;
    for (int s = 0; s < step0; ++s) lr = lr * A.gamma;      // ExponentialLR: one multiplication per finished iteration
    const double w1 = 1.0 - A.beta1, omb2 = 1.0 - A.beta2;
    for (int iter = 0; iter < A.iters; ++iter) {
        if (A.trace) {
            double terms[3];
            nr_cost_terms(A, S, cur, nd, red, terms);
            if (t < 3) A.trace[((size_t)pair * A.iters + iter) * 3 + t] = (float)terms[t];
        }
        for (int c = t; c < S.N; c += NR_SOLVER_BLOCK) {
            double rx, ry, rz;
            nr_residual(A, S, cur, nd, c, rx, ry, rz);
            double* r = A.resid + (size_t)(S.c0 + c) * 3;
            r[0] = rx; r[1] = ry; r[2] = rz;
        }
        __syncthreads();                                    // barrier 1: the residuals are visible to the gathering threads
        const int n = step0 + iter + 1;
        const double bc1 = 1.0 - nr_pow_int(A.beta1, n), bc2 = 1.0 - nr_pow_int(A.beta2, n);
        const double bc2_sqrt = sqrt(bc2), step_size = lr / bc1;
        for (int it = t; it < items; it += NR_SOLVER_BLOCK) {
            const float g = nr_gradient(A, S, cur, nd, it);
            // torch's Adam (exp_avg.lerp_, exp_avg_sq.mul_().addcmul_(), addcdiv_ with eps outside the square root) evaluated in float64 on
            // the float32 state; each of the three state values is rounded once
            const double md = (double)mo[it] + ((double)g - (double)mo[it]) * w1;
            const double vd = (double)vo[it] * A.beta2 + omb2 * ((double)g * (double)g);
            const double denom = sqrt(vd) / bc2_sqrt + A.eps;
            nxt[it] = (float)((double)cur[it] - step_size * (md / denom));
            mo[it] = (float)md; vo[it] = (float)vd;
        }
        __syncthreads();                                    // barrier 2: the next state is complete
        float* sw = cur; cur = nxt; nxt = sw;
        lr = lr * A.gamma;
    }

    // ---- the final state
    for (int it = t; it < S.M * 16; it += NR_SOLVER_BLOCK) {
        const int i = it >> 4, e = it & 15, r = e >> 2, c = e & 3;
        float v;
        if (r == 3) v = c == 3 ? 1.f : 0.f;
        else v = c == 3 ? cur[i * NR_COMP + 9 + r] : cur[i * NR_COMP + r * 3 + c];
        A.transforms[(size_t)(S.m0 + i) * 16 + e] = v;
    }
    for (int it = t; it < items; it += NR_SOLVER_BLOCK) {
        const int i = it / NR_COMP, comp = it - i * NR_COMP;
        const size_t g = (size_t)(S.m0 + i);
        if (comp < 9) {
            if (A.st.rotations) A.st.rotations[g * 9 + comp] = cur[it];
            if (A.st.exp_avg_rot) A.st.exp_avg_rot[g * 9 + comp] = mo[it];
            if (A.st.exp_avg_sq_rot) A.st.exp_avg_sq_rot[g * 9 + comp] = vo[it];
        } else {
            if (A.st.translations) A.st.translations[g * 3 + comp - 9] = cur[it];
            if (A.st.exp_avg_trn) A.st.exp_avg_trn[g * 3 + comp - 9] = mo[it];
            if (A.st.exp_avg_sq_trn) A.st.exp_avg_sq_trn[g * 3 + comp - 9] = vo[it];
        }
    }
    if (A.cost) {
        double terms[3];
        nr_cost_terms(A, S, cur, nd, red, terms);
        if (t < 3) A.cost[pair * 3 + t] = (float)terms[t];
    }
    if (t == 0) {
        if (A.st.step) A.st.step[pair] = step0 + A.iters;
        A.status[pair] = *s_status;
    }
}

static bool nr_sizes_ok(long long a) { return a <= 0x7fffffffLL; }

static int nicp_launch(const dr_nicp_problem* pb, NicpArgs& A, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pb || pb->P < 0 || pb->n_corr < 0 || pb->n_nodes < 0 || pb->n_edges < 0) return DR_EINVAL;
    if (pb->K < 1 || pb->K > NR_MAX_ANCHORS || pb->max_nodes < 0 || pb->max_nodes > nr_node_capacity()) return DR_EINVAL;
    if (!A.status && pb->P > 0) return DR_EINVAL;
    if (pb->P == 0) return DR_OK;
    if (!pb->m_offsets || !pb->c_offsets || !pb->e_offsets) return DR_EINVAL;
    if (pb->n_nodes > 0 && !pb->nodes) return DR_EINVAL;
    if (pb->n_corr > 0 && (!pb->src_corr || !pb->tgt_corr || !pb->anchor_indices || !pb->anchor_weights)) return DR_EINVAL;
    if (pb->n_edges > 0 && (!pb->edges || !pb->edge_weights)) return DR_EINVAL;
    if (!nr_sizes_ok((long long)pb->n_corr * pb->K * 4) || !nr_sizes_ok((long long)pb->n_nodes * 16 + pb->P) || !nr_sizes_ok((long long)pb->n_edges * 2))
        return DR_ENOSUP;
    const NrSolveCarve c = nr_solve_carve(pb->P, pb->n_corr, pb->n_nodes, pb->n_edges, pb->K);
    if (!workspace || workspace_bytes < c.bytes) return DR_EWORKSPACE;
    if (!aligned_to(workspace, 16)) return DR_EINVAL;
    char* w = (char*)workspace;
    A.pb = *pb;
    A.resid = (double*)(w + c.resid); A.anchor = (int32_t*)(w + c.anchor); A.weight = (float*)(w + c.weight);
    A.lm_ptr = (int32_t*)(w + c.lm_ptr); A.lm_corr = (int32_t*)(w + c.lm_corr); A.lm_pw = (float4*)(w + c.lm_pw);
    A.out_ptr = (int32_t*)(w + c.out_ptr); A.out_adj = (NrAdj*)(w + c.out_adj);
    A.in_ptr = (int32_t*)(w + c.in_ptr); A.in_adj = (NrAdj*)(w + c.in_adj);
    A.lds = nr_lds_carve(pb->max_nodes);
    hipLaunchKernelGGL(nicp_kernel, dim3((unsigned)pb->P), dim3(NR_SOLVER_BLOCK), (size_t)A.lds.bytes, (hipStream_t)stream, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// dr_init: the solver's dynamic LDS up to the capacity's carve, set once outside any stream capture
int nonrigid_configure() {
    DR_HIP_CHECK(hipFuncSetAttribute((const void*)nicp_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, nr_lds_carve(nr_node_capacity()).bytes));
    return DR_OK;
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_nicp_node_capacity(void) { return nr_node_capacity(); }

size_t dr_ed_graph_workspace_bytes(int n_nodes, int max_nodes) { return nr_graph_carve(n_nodes, max_nodes).bytes; }

int dr_ed_graph_f32(int P, int n_points, int n_nodes, int max_nodes, int K, const float* points, const int32_t* p_offsets, const float* nodes,
                    const int32_t* m_offsets, double node_coverage, double eps, int64_t* anchor_indices, float* anchor_weights,
                    float* anchor_distances, int32_t* edge_counts, const int32_t* e_offsets, long long edge_cap, int64_t* edge_indices,
                    float* edge_weights, float* edge_distances, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || n_points < 0 || n_nodes < 0 || max_nodes < 0 || max_nodes > n_nodes || K < 1 || K > NR_MAX_ANCHORS || !(node_coverage > 0.0))
        return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (!p_offsets || !m_offsets || !status || (n_points > 0 && !points) || (n_nodes > 0 && !nodes)) return DR_EINVAL;
    const bool write_pass = e_offsets != nullptr;
    if (!write_pass && (!edge_counts || (n_points > 0 && (!anchor_indices || !anchor_weights)))) return DR_EINVAL;
    if (write_pass && (edge_cap < 0 || (edge_cap > 0 && (!edge_indices || !edge_weights)))) return DR_EINVAL;
    const long long grid = nr_grid_bound(n_points, P);
    if (!nr_sizes_ok(grid) || !nr_sizes_ok((long long)n_points * K) || !nr_sizes_ok((long long)n_nodes * 3) || !nr_sizes_ok(edge_cap * 2))
        return DR_ENOSUP;
    const NrGraphCarve c = nr_graph_carve(n_nodes, max_nodes);
    if (c.bytes > 0 && (!workspace || workspace_bytes < c.bytes)) return DR_EWORKSPACE;
    if (!aligned_to(workspace, 16)) return DR_EINVAL;
    char* w = (char*)workspace;
    GraphArgs A = {P, n_points, n_nodes, K, points, p_offsets, nodes, m_offsets, node_coverage, eps, (long long*)anchor_indices, anchor_weights,
                   anchor_distances, edge_counts, e_offsets, edge_cap, (long long*)edge_indices, edge_weights, edge_distances, status,
                   (uint32_t*)(w + c.bitmap), (int32_t*)(w + c.row_count), (double*)(w + c.row_sum), nr_bitmap_words(max_nodes), max_nodes};
    hipStream_t st = (hipStream_t)stream;
    if (!write_pass) {
        DR_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)P * sizeof(int32_t), st));
        if (c.row_count > 0) DR_HIP_CHECK(hipMemsetAsync(w + c.bitmap, 0, c.row_count, st));
        if (n_points > 0) {
            hipLaunchKernelGGL(ed_anchor_kernel, dim3((unsigned)grid), dim3(NR_TILE), 0, st, A);
            DR_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(ed_edge_count_kernel, dim3((unsigned)P), dim3(NR_EDGE_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(ed_edge_write_kernel, dim3((unsigned)P), dim3(NR_EDGE_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

int dr_ed_warp_f32(int P, int n_points, int n_nodes, int K, const float* points, const int32_t* p_offsets, const float* nodes,
                   const int32_t* m_offsets, const float* transforms, const int64_t* anchor_indices, const float* anchor_weights, double eps,
                   float* out, int32_t* status, void* stream) {
    if (P < 0 || n_points < 0 || n_nodes < 0 || K < 1 || K > NR_MAX_ANCHORS) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (!p_offsets || !m_offsets || !status || (n_nodes > 0 && (!nodes || !transforms))) return DR_EINVAL;
    if (n_points > 0 && (!points || !anchor_indices || !anchor_weights || !out)) return DR_EINVAL;
    const long long grid = nr_grid_bound(n_points, P);
    if (!nr_sizes_ok(grid) || !nr_sizes_ok((long long)n_points * K) || !nr_sizes_ok((long long)n_nodes * 16)) return DR_ENOSUP;
    hipStream_t st = (hipStream_t)stream;
    DR_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)P * sizeof(int32_t), st));
    if (n_points == 0) return DR_OK;
    WarpArgs A = {P, n_points, n_nodes, K, points, p_offsets, nodes, m_offsets, transforms, (const long long*)anchor_indices, anchor_weights, eps, out,
                  status};
    hipLaunchKernelGGL(ed_warp_kernel, dim3((unsigned)grid), dim3(NR_TILE), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_nicp_workspace_bytes(int P, int n_corr, int n_nodes, int n_edges, int K) { return nr_solve_carve(P, n_corr, n_nodes, n_edges, K).bytes; }

int dr_nicp_cost_grad_f32(const dr_nicp_problem* problem, const float* rotations, const float* translations, double w_landmark, double w_arap,
                          double w_ortho, float* cost, float* grad_rot, float* grad_trn, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (!problem) return DR_EINVAL;
    if (problem->P > 0 && !cost) return DR_EINVAL;
    if (problem->n_nodes > 0 && (!rotations || !translations || !grad_rot || !grad_trn)) return DR_EINVAL;
    NicpArgs A = {};
    A.wl = w_landmark; A.wa = w_arap; A.wo = w_ortho;
    A.st.rotations = const_cast<float*>(rotations);        // read only: grad_only writes no state
    A.st.translations = const_cast<float*>(translations);
    A.resume = 1;
    A.cost = cost; A.grad_rot = grad_rot; A.grad_trn = grad_trn; A.status = status;
    A.grad_only = 1;
    return nicp_launch(problem, A, workspace, workspace_bytes, stream);
}

int dr_nicp_adam_f32(const dr_nicp_problem* problem, const dr_nicp_options* options, const dr_nicp_state* state, int resume,
                     float* transforms, float* cost, float* trace, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (!problem || !options) return DR_EINVAL;
    if (options->num_iterations < 0 || !(options->lr >= 0.0) || !(options->gamma > 0.0) || !(options->beta1 >= 0.0 && options->beta1 < 1.0) ||
        !(options->beta2 >= 0.0 && options->beta2 < 1.0) || !(options->eps >= 0.0))
        return DR_EINVAL;
    if (problem->n_nodes > 0 && !transforms) return DR_EINVAL;
    if (resume && problem->n_nodes > 0 && (!state || !state->rotations || !state->translations)) return DR_EINVAL;
    NicpArgs A = {};
    A.iters = options->num_iterations;
    A.lr = options->lr; A.gamma = options->gamma; A.beta1 = options->beta1; A.beta2 = options->beta2; A.eps = options->eps;
    A.wl = options->w_landmark; A.wa = options->w_arap; A.wo = options->w_ortho;
    if (state) A.st = *state;
    A.resume = resume ? 1 : 0;
    A.transforms = transforms; A.cost = cost; A.trace = trace; A.status = status;
    A.grad_only = 0;
    return nicp_launch(problem, A, workspace, workspace_bytes, stream);
}

}  // extern "C"
