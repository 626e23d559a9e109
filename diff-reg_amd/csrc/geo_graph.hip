// geo_graph.hip -- the geodesic deformation graph of a point cloud (eighteenth set after ABI 0.7.0):
//   dr_geo_graph_f32     build_deformation_graph_from_point_cloud     2D-3D vision3d/csrc/cpu/deformation_graph/deformation_graph.cpp:13-180,
//                                                                      vision3d/array_ops/deformation.py:443-490
//   dr_geo_graph_edges   the neighbour table as the (E, 2) edge list dr_nicp_problem takes
// Ragged over the clouds of a call, asynchronous on the given stream, nothing read back to the host, no floating-point atomic.
//
// Four launches:
//   1. geo_prep_kernel   one workgroup per cloud: the offsets, the sizes, the node indices (range, duplicates), non-finite points -> status
//   2. geo_adj_kernel    one thread per point: its neighbours closer than max_distance, ascending, into a row of max_degree slots
//   3. geo_relax_kernel  one workgroup per node: label-correcting relaxation of g(y) = min(g(y), fl(g(x) + d(x, y))) over the cloud until a
//                        whole round changes nothing, then the node's Kn nearest nodes and its row of the reach table
//   4. geo_anchor_kernel one thread per point: the Ka nearest nodes of the point from its column of the reach table
// The relaxation keeps the distances as the bit patterns of non-negative float32, whose unsigned order is their float order: the only atomic
// is an integer min, which commutes, so the fixed point does not depend on the schedule (DESIGN 5zb has the argument why it is the
// reference's Dijkstra result bit for bit).  The on-chip form holds the cloud's distances in LDS; the streamed form is the same kernel with the
// distances in the node's row of the reach table.  Every selection is a rank under a strict total order: no atomic decides an order.
//
// Every index below comes from geo_graph_index.h (walked on the host by tools/geo_graph_index_check.cpp).
#include <limits.h>
#include "common.h"
#include "kernels.h"
#include "geo_graph_index.h"
#include "../../include/diffreg_hip.h"

// distances and path sums are written operation by operation (and the file is built with -ffp-contract=off): nothing becomes an FMA
#pragma clang fp contract(off)

namespace dr {

struct GeoArgs {
    int P, n_points, n_nodes, max_points, max_nodes, Kn, Ka, D, cap;     // cap: the on-chip capacity of this call
    const float* points;
    const int32_t* p_off;
    const long long* node_idx;
    const int32_t* n_off;
    float max_distance, coverage;
    long long* nbr_idx;
    float* nbr_dist;
    float* nbr_w;
    long long* anc_idx;
    float* anc_dist;
    float* anc_w;
    int32_t* status;
    int32_t* mark;
    int32_t* deg;
    GeoAdj* adj;
    uint32_t* reach;
    GeoLdsCarve lds;
};

__device__ __forceinline__ bool geo_finite3(float x, float y, float z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// std::sqrt((a - b).sq_norm()) of deformation_graph.cpp:62, sq_norm = x x + y y + z z (cloud.h:46); sqrtf is correctly rounded
__device__ __forceinline__ float geo_dist(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
}

// compute_skinning_weight (.cpp:9-11): distance * distance in float32, the rest in double, rounded once
__device__ __forceinline__ float geo_weight(float g, float c) {
    const float gg = __fmul_rn(g, g);
    return (float)exp((double)(-gg) / ((2.0 * (double)c) * (double)c));
}

// ------------------------------------------------------------------------------------------------ 1. status
__global__ __launch_bounds__(256) void geo_prep_kernel(GeoArgs A) {
    const int p = blockIdx.x, tid = threadIdx.x;
    if (!geo_cloud_ok(A.p_off, p, A.n_points) || !geo_cloud_ok(A.n_off, p, A.n_nodes)) {
        if (tid == 0) A.status[p] = GEO_ST_OFFSETS;
        return;
    }
    const int lo = A.p_off[p], n = A.p_off[p + 1] - lo, m0 = A.n_off[p], M = A.n_off[p + 1] - m0;
    if (n > A.max_points || M > A.max_nodes) {
        if (tid == 0) A.status[p] = GEO_ST_SIZE;
        return;
    }
    int bad = 0;
    for (int x = tid; x < n; x += 256) {
        A.mark[lo + x] = 0;
        const float* q = A.points + (size_t)(lo + x) * 3;
        bad |= geo_finite3(q[0], q[1], q[2]) ? 0 : GEO_ST_NONFINITE;
    }
    __syncthreads();
    for (int j = tid; j < M; j += 256) {
        const long long v = A.node_idx[m0 + j];
        if (v < 0 || v >= n) bad |= GEO_ST_INDEX;
        else if (atomicAdd(&A.mark[lo + (int)v], 1) > 0) bad |= GEO_ST_DUPLICATE;       // an integer count: whoever comes second sees it
    }
    int st = 0;
    st |= __syncthreads_or(bad & GEO_ST_NONFINITE) ? GEO_ST_NONFINITE : 0;
    st |= __syncthreads_or(bad & GEO_ST_INDEX) ? GEO_ST_INDEX : 0;
    st |= __syncthreads_or(bad & GEO_ST_DUPLICATE) ? GEO_ST_DUPLICATE : 0;
    if (tid == 0) A.status[p] = st;
}

// ------------------------------------------------------------------------------------------------ 2. adjacency
// Brute force over the cloud: thread x walks k = 0 .. n - 1 (every lane reads the same row: one broadcast load), so a row is ascending in k.
// A point with a NaN / Inf coordinate fails every `d < max_distance` and gets no edge.
__global__ __launch_bounds__(NR_TILE) void geo_adj_kernel(GeoArgs A) {
    int p, tile;
    if (!geo_locate(A.P, A.p_off, A.n_points, NR_TILE, blockIdx.x, p, tile)) return;
    if (A.status[p] & (GEO_ST_SIZE | GEO_ST_OFFSETS)) return;
    const int lo = A.p_off[p], n = A.p_off[p + 1] - lo, x = tile * NR_TILE + threadIdx.x;
    if (x >= n) return;
    const float* __restrict__ pts = A.points + (size_t)lo * 3;
    const float px = pts[3 * x], py = pts[3 * x + 1], pz = pts[3 * x + 2];
    GeoAdj* __restrict__ row = A.adj + geo_adj_slot(lo, x, A.D, 0);
    int cnt = 0;
    for (int k = 0; k < n; ++k) {
        const float d = geo_dist(px, py, pz, pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]);
        if (d < A.max_distance && k != x) {
            if (cnt < A.D) {
                row[cnt].y = k;
                row[cnt].d = d;
            }
            ++cnt;
        }
    }
    A.deg[lo + x] = cnt < A.D ? cnt : A.D;
    if (cnt > A.D) atomicOr(&A.status[p], GEO_ST_DEGREE);
}

// ------------------------------------------------------------------------------------------------ 3. relaxation, neighbours
// the streamed form reads a distance that other lanes lower with an atomic in L2: the load has to come from there too
template <bool ONCHIP>
__device__ __forceinline__ uint32_t geo_load(const uint32_t* g, int x) {
    if (ONCHIP) return g[x];
    return __hip_atomic_load(g + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (g, point descending, node ascending): the pop order of the reference's max-heap of (-g, point); the node breaks what a duplicate leaves
__device__ __forceinline__ bool geo_nbr_before(uint32_t ga, int pa, int ja, uint32_t gb, int pb, int jb) {
    if (ga != gb) return ga < gb;
    if (pa != pb) return pa > pb;
    return ja < jb;
}

template <bool ONCHIP>
__global__ __launch_bounds__(GEO_BLOCK) void geo_relax_kernel(GeoArgs A) {
    extern __shared__ uint32_t geo_lds[];
    const int tid = threadIdx.x;
    int p, i;
    if (!geo_locate(A.P, A.n_off, A.n_nodes, 1, blockIdx.x, p, i)) return;
    if (!geo_cloud_ok(A.p_off, p, A.n_points)) return;
    const int lo = A.p_off[p], n = A.p_off[p + 1] - lo, m0 = A.n_off[p], M = A.n_off[p + 1] - m0;
    const int st = A.status[p];                  // written by the launches before this one
    const bool refused = (st & (GEO_ST_SIZE | GEO_ST_OFFSETS | GEO_ST_DEGREE)) != 0;
    if (!refused && (n <= A.cap) != ONCHIP) return;         // a cloud belongs to exactly one of the two instantiations
    if (refused && !ONCHIP) return;
    const int row = m0 + i;
    if (refused) {                               // padding only (a cloud with bit 1 may have more nodes than the LDS stage holds)
        if (tid < A.Kn) {
            A.nbr_idx[geo_table(row, A.Kn, tid)] = -1;
            A.nbr_dist[geo_table(row, A.Kn, tid)] = 0.0f;
            A.nbr_w[geo_table(row, A.Kn, tid)] = 0.0f;
        }
        return;
    }
    uint32_t* g = ONCHIP ? geo_lds + A.lds.g : A.reach + geo_reach(row, A.max_points, 0);
    uint32_t* done = geo_lds + A.lds.done;       // on-chip form only
    uint32_t* node_g = geo_lds + A.lds.node_g;
    int* node_pt = (int*)(geo_lds + A.lds.node_pt);
    int* count = (int*)(geo_lds + A.lds.count);
    const long long src64 = A.node_idx[row];
    const bool present = src64 >= 0 && src64 < n;            // an index out of range is an absent node: it reaches nothing
    const int src = present ? (int)src64 : 0;
    for (int x = tid; x < n; x += GEO_BLOCK) {
        g[x] = (present && x == src) ? 0u : GEO_UNREACHED;
        if (ONCHIP) done[x] = GEO_UNREACHED;
    }
    if (tid == 0) *count = 0;
    if (!ONCHIP) __threadfence();                // the plain stores above are in L2 before any lane's atomic goes there
    __syncthreads();
    if (present) {
        const double lim = 2.0 * (double)A.coverage;         // .cpp:137: float32 sum against a double bound
        const int32_t* __restrict__ deg = A.deg + lo;
        for (;;) {
            int changed = 0;
            for (int x = tid; x < n; x += GEO_BLOCK) {
                const uint32_t v = geo_load<ONCHIP>(g, x);
                if (v == GEO_UNREACHED) continue;
                if (ONCHIP) {                                // expand a point only when its distance fell since it was last expanded
                    if (v >= done[x]) continue;
                    done[x] = v;
                }
                const float fv = __uint_as_float(v);
                const GeoAdj* __restrict__ e = A.adj + geo_adj_slot(lo, x, A.D, 0);
                const int dg = deg[x];
                for (int k = 0; k < dg; ++k) {
                    const GeoAdj a = e[k];
                    const float nd = __fadd_rn(fv, a.d);
                    if ((double)nd <= lim) {
                        const uint32_t nb = __float_as_uint(nd);
                        const uint32_t old = atomicMin(&g[a.y], nb);
                        changed |= old > nb ? 1 : 0;
                    }
                }
            }
            if (!__syncthreads_or(changed)) break;
        }
    }
    // the nodes' keys, then node i's row: the rank of every reached node under the strict order above
    for (int j = tid; j < M; j += GEO_BLOCK) {
        const long long v = A.node_idx[m0 + j];
        const bool ok = v >= 0 && v < n;
        node_pt[j] = ok ? (int)v : -1;
        node_g[j] = ok ? geo_load<ONCHIP>(g, (int)v) : GEO_UNREACHED;
    }
    __syncthreads();
    for (int j = tid; j < M; j += GEO_BLOCK) {
        const uint32_t gj = node_g[j];
        if (gj == GEO_UNREACHED) continue;
        const int pj = node_pt[j];
        int rank = 0;
        for (int k = 0; k < M; ++k) {
            const uint32_t gk = node_g[k];
            rank += (gk != GEO_UNREACHED && k != j && geo_nbr_before(gk, node_pt[k], k, gj, pj, j)) ? 1 : 0;
        }
        atomicAdd(count, 1);                                 // an integer count
        if (rank < A.Kn) {
            const float d = __uint_as_float(gj);
            A.nbr_idx[geo_table(row, A.Kn, rank)] = j;
            A.nbr_dist[geo_table(row, A.Kn, rank)] = d;
            A.nbr_w[geo_table(row, A.Kn, rank)] = geo_weight(d, A.coverage);
        }
    }
    __syncthreads();
    const int reached = *count;
    if (tid < A.Kn && tid >= reached) {
        A.nbr_idx[geo_table(row, A.Kn, tid)] = -1;
        A.nbr_dist[geo_table(row, A.Kn, tid)] = 0.0f;
        A.nbr_w[geo_table(row, A.Kn, tid)] = 0.0f;
    }
    if (ONCHIP) {
        uint32_t* __restrict__ out = A.reach + geo_reach(row, A.max_points, 0);
        for (int x = tid; x < n; x += GEO_BLOCK) out[x] = g[x];
    }
}

// ------------------------------------------------------------------------------------------------ 4. anchors
// Point x reads its column of the cloud's rows of the reach table, nodes ascending, and keeps the Ka smallest by insertion with a strict <:
// (g ascending, node ascending), std::sort's order on (distance, node) pairs (.cpp:151).  The lists live in registers: every array index
// below is a compile-time constant after unrolling.
__global__ __launch_bounds__(NR_TILE) void geo_anchor_kernel(GeoArgs A) {
    int p, tile;
    if (!geo_locate(A.P, A.p_off, A.n_points, NR_TILE, blockIdx.x, p, tile)) return;
    if (!geo_cloud_ok(A.n_off, p, A.n_nodes)) return;
    const int lo = A.p_off[p], n = A.p_off[p + 1] - lo, x = tile * NR_TILE + threadIdx.x;
    if (x >= n) return;
    const int m0 = A.n_off[p], M = A.n_off[p + 1] - m0, r = lo + x;
    const bool refused = (A.status[p] & (GEO_ST_SIZE | GEO_ST_OFFSETS | GEO_ST_DEGREE)) != 0;
    uint32_t bv[GEO_MAX_K];
    int bi[GEO_MAX_K];
#pragma unroll
    for (int s = 0; s < GEO_MAX_K; ++s) {
        bv[s] = GEO_UNREACHED;
        bi[s] = -1;
    }
    if (!refused) {
        for (int i = 0; i < M; ++i) {
            uint32_t cv = A.reach[geo_reach(m0 + i, A.max_points, x)];
            if (cv == GEO_UNREACHED) continue;
            int ci = i;
#pragma unroll
            for (int s = 0; s < GEO_MAX_K; ++s) {
                const bool take = s < A.Ka && cv < bv[s];
                const uint32_t tv = bv[s];
                const int ti = bi[s];
                bv[s] = take ? cv : tv;
                bi[s] = take ? ci : ti;
                cv = take ? tv : cv;
                ci = take ? ti : ci;
            }
        }
    }
    int cnt = 0;
    float w[GEO_MAX_K];
    float sum = 0.0f;
#pragma unroll
    for (int s = 0; s < GEO_MAX_K; ++s) {
        const bool has = bi[s] >= 0;
        cnt += has ? 1 : 0;
        w[s] = has ? geo_weight(__uint_as_float(bv[s]), A.coverage) : 0.0f;
        sum = has ? __fadd_rn(sum, w[s]) : sum;                   // float32, in list order (.cpp:164-167)
    }
    const float even = cnt > 0 ? (float)(1.0 / (double)(float)cnt) : 0.0f;      // .cpp:174
#pragma unroll
    for (int s = 0; s < GEO_MAX_K; ++s) {
        if (s < A.Ka) {
            const bool has = bi[s] >= 0;
            A.anc_idx[geo_table(r, A.Ka, s)] = has ? bi[s] : -1;
            A.anc_dist[geo_table(r, A.Ka, s)] = has ? __uint_as_float(bv[s]) : 0.0f;
            A.anc_w[geo_table(r, A.Ka, s)] = has ? (sum > 0.0f ? __fdiv_rn(w[s], sum) : even) : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ edge list
// One workgroup per cloud walks the neighbour rows in chunks of GEO_EDGE_BLOCK: a thread counts its row's edges, an inclusive scan over the
// chunk in LDS places the row, a running base places the chunk: row-major order without an atomic.  The count pass stops at the total.
struct GeoEdgeArgs {
    int P, n_nodes, Kn;
    const long long* nbr_idx;
    const float* nbr_w;
    const int32_t* n_off;
    int32_t* counts;
    const int32_t* e_off;
    long long edge_cap;
    long long* edge_idx;
    float* edge_w;
};

__global__ __launch_bounds__(GEO_EDGE_BLOCK) void geo_edge_kernel(GeoEdgeArgs A) {
    __shared__ int scan[GEO_EDGE_BLOCK];
    const int p = blockIdx.x, tid = threadIdx.x;
    const bool ok = geo_cloud_ok(A.n_off, p, A.n_nodes);
    const int m0 = ok ? A.n_off[p] : 0, M = ok ? A.n_off[p + 1] - m0 : 0;
    const bool write = A.e_off != nullptr;
    long long lo = 0, hi = 0;
    if (write) {
        lo = A.e_off[p];
        hi = A.e_off[p + 1];
        hi = hi < A.edge_cap ? hi : A.edge_cap;
        if (lo < 0) hi = 0;                                      // offsets that are no offsets: nothing is written
    }
    int base = 0;
    for (int c = 0; c < geo_edge_chunks(M); ++c) {
        const int i = c * GEO_EDGE_BLOCK + tid;
        int mine = 0;
        if (i < M)
            for (int k = 0; k < A.Kn; ++k) mine += geo_is_edge(A.nbr_idx[geo_table(m0 + i, A.Kn, k)], i, M) ? 1 : 0;
        scan[tid] = mine;
        __syncthreads();
        for (int s = 1; s < GEO_EDGE_BLOCK; s <<= 1) {           // Hillis-Steele, inclusive
            const int v = tid >= s ? scan[tid - s] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int total = scan[GEO_EDGE_BLOCK - 1];
        if (write && i < M) {
            long long at = lo + base + scan[tid] - mine;
            for (int k = 0; k < A.Kn; ++k) {
                const long long j = A.nbr_idx[geo_table(m0 + i, A.Kn, k)];
                if (!geo_is_edge(j, i, M)) continue;
                if (at < hi) {
                    A.edge_idx[2 * at] = i;
                    A.edge_idx[2 * at + 1] = j;
                    if (A.edge_w) A.edge_w[at] = A.nbr_w[geo_table(m0 + i, A.Kn, k)];
                }
                ++at;
            }
        }
        base += total;
        __syncthreads();                                         // scan[] is rewritten by the next chunk
    }
    if (!write && tid == 0) A.counts[p] = base;
}

// dr_init: the relaxation's dynamic LDS up to the capacity's carve, set once outside any stream capture
int geo_graph_configure() {
    const int bytes = geo_lds_carve(GEO_ONCHIP_CAPACITY, GEO_MAX_NODES).bytes;
    DR_HIP_CHECK(hipFuncSetAttribute((const void*)geo_relax_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    DR_HIP_CHECK(hipFuncSetAttribute((const void*)geo_relax_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return DR_OK;
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_geo_graph_onchip_capacity(void) { return geo_onchip_capacity(); }

size_t dr_geo_graph_workspace_bytes(int P, int n_points, int n_nodes, int max_points, int max_degree) {
    if (P <= 0) return 0;
    return geo_carve(n_points, n_nodes, max_points, max_degree).bytes;
}

int dr_geo_graph_f32(int P, int n_points, int n_nodes, int max_points, int max_nodes, const float* points, const int32_t* p_offsets,
                     const int64_t* node_indices, const int32_t* n_offsets, const dr_geo_graph_options* options, int64_t* neighbor_indices,
                     float* neighbor_distances, float* neighbor_weights, int64_t* anchor_indices, float* anchor_distances, float* anchor_weights,
                     int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || n_points < 0 || n_nodes < 0 || max_points < 0 || max_points > n_points || max_nodes < 0 || max_nodes > n_nodes) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (!options || !p_offsets || !n_offsets || !status) return DR_EINVAL;
    const int Kn = options->num_neighbors, Ka = options->num_anchors, D = options->max_degree;
    if (Kn < 1 || Ka < 1 || D < 1 || options->onchip_cap_override < 0) return DR_EINVAL;
    if (Kn > GEO_MAX_K || Ka > GEO_MAX_K) return DR_EINVAL;
    if (!(options->max_distance > 0.0f) || !(options->node_coverage > 0.0f) || !__builtin_isfinite(options->max_distance) ||
        !__builtin_isfinite(options->node_coverage))
        return DR_EINVAL;
    if (n_points > 0 && (!points || !anchor_indices || !anchor_distances || !anchor_weights)) return DR_EINVAL;
    if (n_nodes > 0 && (!node_indices || !neighbor_indices || !neighbor_distances || !neighbor_weights)) return DR_EINVAL;
    if (n_points > INT_MAX / 3 || P > 65535 || max_nodes > GEO_MAX_NODES || D > GEO_MAX_DEGREE) return DR_ENOSUP;
    const GeoCarve c = geo_carve(n_points, n_nodes, max_points, D);
    if (!workspace || workspace_bytes < c.bytes) return DR_EWORKSPACE;
    if (((uintptr_t)workspace & 15) != 0) return DR_EINVAL;
    char* w = (char*)workspace;
    GeoArgs A = {};
    A.P = P; A.n_points = n_points; A.n_nodes = n_nodes; A.max_points = max_points; A.max_nodes = max_nodes;
    A.Kn = Kn; A.Ka = Ka; A.D = D; A.cap = geo_effective_capacity(options->onchip_cap_override);
    A.points = points; A.p_off = p_offsets; A.node_idx = (const long long*)node_indices; A.n_off = n_offsets;
    A.max_distance = options->max_distance; A.coverage = options->node_coverage;
    A.nbr_idx = (long long*)neighbor_indices; A.nbr_dist = neighbor_distances; A.nbr_w = neighbor_weights;
    A.anc_idx = (long long*)anchor_indices; A.anc_dist = anchor_distances; A.anc_w = anchor_weights; A.status = status;
    A.mark = (int32_t*)(w + c.mark); A.deg = (int32_t*)(w + c.deg); A.adj = (GeoAdj*)(w + c.adj); A.reach = (uint32_t*)(w + c.reach);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(geo_prep_kernel, dim3((unsigned)P), dim3(256), 0, st, A);
    DR_LAUNCH_CHECK();
    const long long tiles = nr_grid_bound(n_points, P);
    if (n_points > 0) {
        hipLaunchKernelGGL(geo_adj_kernel, dim3((unsigned)tiles), dim3(NR_TILE), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    if (n_nodes > 0) {
        A.lds = geo_lds_carve(geo_lds_points(max_points, A.cap), max_nodes);
        hipLaunchKernelGGL(geo_relax_kernel<true>, dim3((unsigned)n_nodes), dim3(GEO_BLOCK), (size_t)A.lds.bytes, st, A);
        DR_LAUNCH_CHECK();
        if (max_points > A.cap) {
            A.lds = geo_lds_carve(0, max_nodes);
            hipLaunchKernelGGL(geo_relax_kernel<false>, dim3((unsigned)n_nodes), dim3(GEO_BLOCK), (size_t)A.lds.bytes, st, A);
            DR_LAUNCH_CHECK();
        }
    }
    if (n_points > 0) {
        hipLaunchKernelGGL(geo_anchor_kernel, dim3((unsigned)tiles), dim3(NR_TILE), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

int dr_geo_graph_edges(int P, int n_nodes, int num_neighbors, const int64_t* neighbor_indices, const float* neighbor_weights,
                       const int32_t* n_offsets, int32_t* edge_counts, const int32_t* e_offsets, long long edge_cap, int64_t* edge_indices,
                       float* edge_weights, void* stream) {
    if (P < 0 || n_nodes < 0 || edge_cap < 0) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (num_neighbors < 1 || num_neighbors > GEO_MAX_K || !n_offsets || (n_nodes > 0 && !neighbor_indices)) return DR_EINVAL;
    if (!e_offsets && !edge_counts) return DR_EINVAL;
    if (e_offsets && edge_cap > 0 && (!edge_indices || (edge_weights && !neighbor_weights))) return DR_EINVAL;
    if (P > 65535 || edge_cap > INT_MAX / 2) return DR_ENOSUP;
    GeoEdgeArgs A = {P, n_nodes, num_neighbors, (const long long*)neighbor_indices, neighbor_weights, n_offsets, edge_counts, e_offsets, edge_cap,
                     (long long*)edge_indices, edge_weights};
    hipLaunchKernelGGL(geo_edge_kernel, dim3((unsigned)P), dim3(GEO_EDGE_BLOCK), 0, (hipStream_t)stream, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
