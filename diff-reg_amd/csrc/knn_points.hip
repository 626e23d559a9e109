// knn_points.hip -- the non-rigid evaluation's kernels (nineteenth set after ABI 0.7.0):
//   dr_knn_points_f32     vision3d.ops.knn / keops_knn                                  2D-3D vision3d/ops/knn.py:10-107
//   dr_nn_stats_f32       compute_corr_coverage, compute_chamfer_distance               2D-3D vision3d/ops/metrics.py:359-372
//   dr_flow_metrics_f32   compute_nonrigid_inlier_ratio, compute_scene_flow_accuracy,   2D-3D vision3d/ops/metrics.py:258-356
//                         compute_scene_flow_outlier_ratio, the NFMR predicate
// All are ragged over the pairs of a call, asynchronous on the given stream, read nothing back to the host and use no atomic of any kind.
//
// The search: a workgroup of four waves owns ONE block of KNN_BLOCK = 64 queries; lane l of every wave holds query l's coordinates in registers.
// The pair's supports pass through LDS in tiles of KNN_TILE, structure-of-arrays; wave w walks entries [w, w + 1) KNN_QUARTER of every tile, so
// the four waves split the distance evaluations of their 64 queries four ways.  Every lane of a wave reads the same support: a broadcast read,
// four consecutive supports of one coordinate per 16-byte read.  A lane's K best so far are a sorted register list (d2 ascending, then index
// ascending) updated by a fully unrolled compare-and-shift -- K is a template parameter and no register array is indexed by a run-time value.
// After the last tile waves 1 .. 3 hand their lists to wave 0 through LDS, which merges them in wave order by (d2, index) and writes the rows.
//
// Every index below comes from knn_index.h (walked on the host by tools/knn_index_check.cpp).
#include <limits.h>
#include "common.h"
#include "kernels.h"
#include "knn_index.h"
#include "../../include/diffreg_hip.h"

// d2 = (dx dx + dy dy) + dz dz is written operation by operation (and the file is built with -ffp-contract=off): nothing becomes an FMA
#pragma clang fp contract(off)

namespace dr {

struct KnnArgs {
    int P, n_q, n_s, k;
    const float* q;
    const int32_t* q_off;
    const float* s;
    const int32_t* s_off;
    float* dist;            // [n_q, k] or NULL
    long long* idx;         // [n_q, k] or NULL
    float limit;            // statistics form: distance_limit
    double* partials;       // statistics form: [grid bound, NN_SLOTS]
};

// slot list of one lane.  insert() keeps it ascending by (d2, index) for candidates that arrive in ascending index (ties stay behind what is
// there); insert_keyed() is the same for candidates in any index order (the merge).
template <int K>
struct KnnList {
    float d[K];
    int i[K];

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            d[j] = INFINITY;
            i[j] = -1;
        }
    }
    __device__ __forceinline__ void insert(float c, int ci) {
        // new[j] = c before old[j - 1] ? old[j - 1] : (c before old[j] ? c : old[j]), from the last slot down so that old[j - 1] is still old
#pragma unroll
        for (int j = K - 1; j >= 1; --j) {
            const bool up = c < d[j - 1], here = c < d[j];
            d[j] = up ? d[j - 1] : (here ? c : d[j]);
            i[j] = up ? i[j - 1] : (here ? ci : i[j]);
        }
        const bool first = c < d[0];
        d[0] = first ? c : d[0];
        i[0] = first ? ci : i[0];
    }
    static __device__ __forceinline__ bool before(float c, int ci, float o, int oi) { return c < o || (c == o && (unsigned)ci < (unsigned)oi); }
    __device__ __forceinline__ void insert_keyed(float c, int ci) {
#pragma unroll
        for (int j = K - 1; j >= 1; --j) {
            const bool up = before(c, ci, d[j - 1], i[j - 1]), here = before(c, ci, d[j], i[j]);
            d[j] = up ? d[j - 1] : (here ? c : d[j]);
            i[j] = up ? i[j - 1] : (here ? ci : i[j]);
        }
        const bool first = before(c, ci, d[0], i[0]);
        d[0] = first ? c : d[0];
        i[0] = first ? ci : i[0];
    }
};

__device__ __forceinline__ float knn_d2(float qx, float qy, float qz, float sx, float sy, float sz) {
    const float dx = __fsub_rn(qx, sx), dy = __fsub_rn(qy, sy), dz = __fsub_rn(qz, sz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// the wave's sum of v in the fixed tree lane l += lane l + off, off = 32, 16, 8, 4, 2, 1; lane 0 holds it
__device__ __forceinline__ double knn_wave_sum(double v) {
#pragma unroll
    for (int off = KNN_WAVE / 2; off >= 1; off >>= 1) v += __shfl_down(v, off, KNN_WAVE);
    return v;
}

template <int K, bool STATS>
__global__ __launch_bounds__(KNN_THREADS) void knn_points_kernel(KnnArgs A) {
    __shared__ __attribute__((aligned(16))) float lds[KNN_LDS_WORDS];
    int p, block;
    if (!knn_block_to_pair(A.P, A.q_off, A.n_q, KNN_BLOCK, blockIdx.x, p, block)) return;      // uniform over the workgroup
    const int qlo = A.q_off[p], Q = A.q_off[p + 1] - qlo;
    const int slo = A.s_off[p], shi = A.s_off[p + 1];
    const bool s_ok = nr_slice_ok(slo, shi, A.n_s);
    if (!s_ok && !STATS) return;                     // the pair is skipped (status bit 4); its rows are not written
    const int S = s_ok ? shi - slo : 0;              // the statistics form still writes its partial row (zeros)
    const int tid = threadIdx.x, lane = tid & (KNN_WAVE - 1), wave = tid / KNN_WAVE;
    const int qi = knn_query_of(block, lane);
    const bool owns = qi < Q;
    const float* __restrict__ qp = A.q + knn_coord(qlo, 0, 0);
    const float* __restrict__ sp = A.s + knn_coord(s_ok ? slo : 0, 0, 0);
    // a lane without a query, and a query with a NaN / Inf coordinate, compares false against everything: its list stays +inf / -1
    const float qx = owns ? qp[knn_local_coord(qi, 0)] : NAN;
    const float qy = owns ? qp[knn_local_coord(qi, 1)] : NAN;
    const float qz = owns ? qp[knn_local_coord(qi, 2)] : NAN;

    KnnList<K> L;
    L.clear();
    const int tiles = knn_tiles(S);
    for (int t = 0; t < tiles; ++t) {
        const int count = knn_tile_count(S, t);
        if (t > 0) __syncthreads();                  // every wave has finished the previous tile
#pragma unroll
        for (int e = tid; e < KNN_TILE; e += KNN_THREADS) {
            const bool in = e < count;
            const int r = knn_support_of(t, in ? e : 0);
            const float x = sp[knn_local_coord(r, 0)], y = sp[knn_local_coord(r, 1)], z = sp[knn_local_coord(r, 2)];
            lds[knn_lds_coord(0, e)] = in ? x : NAN;
            lds[knn_lds_coord(1, e)] = in ? y : NAN;
            lds[knn_lds_coord(2, e)] = in ? z : NAN;
        }
        __syncthreads();
        const int e0 = knn_quarter_first(wave), walk = knn_quarter_walk(count, wave);
        for (int j = 0; j < walk; j += KNN_VEC) {
            const float4 sx = *(const float4*)&lds[knn_lds_coord(0, e0 + j)];
            const float4 sy = *(const float4*)&lds[knn_lds_coord(1, e0 + j)];
            const float4 sz = *(const float4*)&lds[knn_lds_coord(2, e0 + j)];
            const float c0 = knn_d2(qx, qy, qz, sx.x, sy.x, sz.x), c1 = knn_d2(qx, qy, qz, sx.y, sy.y, sz.y);
            const float c2 = knn_d2(qx, qy, qz, sx.z, sy.z, sz.z), c3 = knn_d2(qx, qy, qz, sx.w, sy.w, sz.w);
            const float worst = L.d[K - 1];
            // most candidates beat no slot of any lane: the wave then skips the four insertions (a NaN or +inf candidate never enters)
            if (c0 < worst || c1 < worst || c2 < worst || c3 < worst) {
                const int base = knn_support_of(t, e0 + j);
                L.insert(c0, base);
                L.insert(c1, base + 1);
                L.insert(c2, base + 2);
                L.insert(c3, base + 3);
            }
        }
    }
    // merge: waves 1 .. 3 -> LDS -> wave 0, in wave order
    __syncthreads();                                 // the last tile has been read by every wave
    if (wave > 0) {
        int* ilds = (int*)lds;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            lds[knn_merge_word(K, 0, wave, j, lane)] = L.d[j];
            ilds[knn_merge_word(K, 1, wave, j, lane)] = L.i[j];
        }
    }
    __syncthreads();
    if (wave > 0) return;
    {
        const int* ilds = (const int*)lds;
#pragma unroll
        for (int w = 1; w < KNN_WAVES; ++w) {
#pragma unroll
            for (int j = 0; j < K; ++j)
                L.insert_keyed(lds[knn_merge_word(K, 0, w, j, lane)], ilds[knn_merge_word(K, 1, w, j, lane)]);
        }
    }
    if (STATS) {
        const float dist = sqrtf(L.d[0]);
        const bool have = owns && L.i[0] >= 0;
        const double dd = have ? (double)dist : 0.0;
        const double n = knn_wave_sum(have ? 1.0 : 0.0), s1 = knn_wave_sum(dd), s2 = knn_wave_sum(dd * dd);
        const double c = knn_wave_sum((have && dist < A.limit) ? 1.0 : 0.0);
        if (lane == 0) {
            A.partials[knn_partial(blockIdx.x, NN_SLOTS, 0)] = n;
            A.partials[knn_partial(blockIdx.x, NN_SLOTS, 1)] = s1;
            A.partials[knn_partial(blockIdx.x, NN_SLOTS, 2)] = s2;
            A.partials[knn_partial(blockIdx.x, NN_SLOTS, 3)] = c;
        }
        return;
    }
    if (!owns) return;
    const size_t row = knn_row(qlo, qi);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < A.k) {
            if (A.dist) A.dist[knn_out(row, A.k, j)] = sqrtf(L.d[j]);
            if (A.idx) A.idx[knn_out(row, A.k, j)] = (long long)L.i[j];
        }
    }
}

// one workgroup per pair: the status word, written once (bad offsets; a non-finite query)
__global__ __launch_bounds__(KNN_THREADS) void knn_status_kernel(KnnArgs A, int32_t* status) {
    const int p = blockIdx.x;
    const int qlo = A.q_off[p], qhi = A.q_off[p + 1], slo = A.s_off[p], shi = A.s_off[p + 1];
    int st = 0;
    if (!nr_slice_ok(qlo, qhi, A.n_q) || !nr_slice_ok(slo, shi, A.n_s)) {
        st = KNN_ST_OFFSETS;
    } else {
        const float* __restrict__ qp = A.q + knn_coord(qlo, 0, 0);
        int bad = 0;
        for (int i = threadIdx.x; i < qhi - qlo; i += KNN_THREADS) {
            const float x = qp[knn_local_coord(i, 0)], y = qp[knn_local_coord(i, 1)], z = qp[knn_local_coord(i, 2)];
            bad |= (__builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z)) ? 0 : 1;
        }
        if (__syncthreads_or(bad)) st = KNN_ST_NONFINITE;
    }
    if (threadIdx.x == 0) status[p] = st;
}

// the final pass of both reductions: thread (pair, slot) adds the pair's block partials in ascending block order
__global__ void knn_final_kernel(int P, const int32_t* off, int total, int per, int slots, const double* partials, double* out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= P * slots) return;
    const int p = t / slots, s = t - p * slots;
    const int lo = off[p], hi = off[p + 1];
    const int nb = knn_blocks(nr_slice_ok(lo, hi, total) ? hi - lo : 0, per);
    const long long first = knn_first_block(p, off, total, per);
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc += partials[knn_partial(first + b, slots, s)];
    out[(size_t)p * slots + s] = acc;
}

struct FlowArgs {
    int P, n;
    const float* pred;
    const float* target;
    const int32_t* off;
    const uint8_t* mask;
    const float* rot;
    const float* trn;
    float strict_abs, strict_rel, relaxed_abs, relaxed_rel, outlier_abs, outlier_rel, eps;
    double* partials;
};

// one point per thread; the six terms go lanes -> wave (the tree of knn_wave_sum) -> the four waves in wave order -> the block's partial row
__global__ __launch_bounds__(FLOW_BLOCK) void flow_metrics_kernel(FlowArgs A) {
    __shared__ double lds[FLOW_LDS_WORDS];
    int p, block;
    if (!knn_block_to_pair(A.P, A.off, A.n, FLOW_BLOCK, blockIdx.x, p, block)) return;
    const int lo = A.off[p], n = A.off[p + 1] - lo;
    const int tid = threadIdx.x, lane = tid & (KNN_WAVE - 1), wave = tid / KNN_WAVE;
    const int i = block * FLOW_BLOCK + tid;
    double v[FLOW_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < n && (!A.mask || A.mask[knn_row(lo, i)] != 0)) {
        const float* __restrict__ pp = A.pred + knn_coord(lo, i, 0);
        const float* __restrict__ tp = A.target + knn_coord(lo, i, 0);
        float x = pp[0], y = pp[1], z = pp[2];
        if (A.rot) {                                 // apply_transform: R x + t
            const float* R = A.rot + (size_t)p * 9;
            const float* T = A.trn + (size_t)p * 3;
            const float nx = ((R[0] * x + R[1] * y) + R[2] * z) + T[0];
            const float ny = ((R[3] * x + R[4] * y) + R[5] * z) + T[1];
            const float nz = ((R[6] * x + R[7] * y) + R[8] * z) + T[2];
            x = nx; y = ny; z = nz;
        }
        const float tx = tp[0], ty = tp[1], tz = tp[2];
        const float e = sqrtf(knn_d2(x, y, z, tx, ty, tz));
        const float len = sqrtf((tx * tx + ty * ty) + tz * tz);
        const float rel = e / (len + A.eps);
        const bool strict = e < A.strict_abs || rel < A.strict_rel;
        const bool relaxed = e < A.relaxed_abs || rel < A.relaxed_rel;
        const bool outlier = (A.outlier_abs >= 0.0f && e > A.outlier_abs) || (A.outlier_rel >= 0.0f && rel > A.outlier_rel);
        v[0] = 1.0;
        v[1] = (double)e;
        v[2] = strict ? 1.0 : 0.0;
        v[3] = relaxed ? 1.0 : 0.0;
        v[4] = outlier ? 1.0 : 0.0;
        v[5] = e < A.strict_abs ? 1.0 : 0.0;
    }
#pragma unroll
    for (int s = 0; s < FLOW_SLOTS; ++s) {
        const double w = knn_wave_sum(v[s]);
        if (lane == 0) lds[flow_lds_word(wave, s)] = w;
    }
    __syncthreads();
    if (tid < FLOW_SLOTS) {
        double acc = 0.0;
#pragma unroll
        for (int w = 0; w < FLOW_BLOCK / KNN_WAVE; ++w) acc += lds[flow_lds_word(w, tid)];
        A.partials[knn_partial(blockIdx.x, FLOW_SLOTS, tid)] = acc;
    }
}

// status of the flow metrics: bad offsets only
__global__ void flow_status_kernel(int P, const int32_t* off, int total, int32_t* status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < P) status[p] = nr_slice_ok(off[p], off[p + 1], total) ? 0 : KNN_ST_OFFSETS;
}

template <bool STATS>
static int knn_launch(const KnnArgs& A, hipStream_t st) {
    const unsigned grid = (unsigned)knn_grid_bound(A.n_q, A.P, KNN_BLOCK);
    if (grid == 0) return DR_OK;
    if constexpr (STATS) {                           // the statistics form is the k = 1 instantiation alone
        hipLaunchKernelGGL((knn_points_kernel<1, true>), dim3(grid), dim3(KNN_THREADS), 0, st, A);
        DR_LAUNCH_CHECK();
        return DR_OK;
    }
    switch (knn_width(A.k)) {
        case 1: hipLaunchKernelGGL((knn_points_kernel<1, STATS>), dim3(grid), dim3(KNN_THREADS), 0, st, A); break;
        case 4: hipLaunchKernelGGL((knn_points_kernel<4, STATS>), dim3(grid), dim3(KNN_THREADS), 0, st, A); break;
        case 8: hipLaunchKernelGGL((knn_points_kernel<8, STATS>), dim3(grid), dim3(KNN_THREADS), 0, st, A); break;
        case 16: hipLaunchKernelGGL((knn_points_kernel<16, STATS>), dim3(grid), dim3(KNN_THREADS), 0, st, A); break;
        default: return DR_EINVAL;
    }
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// a host mirror of an offset table (or NULL): P + 1 ascending entries inside [0, total]
static bool knn_host_offsets_ok(const int32_t* h, int P, int total) {
    if (!h) return true;
    if (h[0] < 0 || h[P] > total) return false;
    for (int p = 0; p < P; ++p)
        if (h[p + 1] < h[p]) return false;
    return true;
}

static int knn_common_check(int P, int n_q, int n_s, const float* q, const int32_t* q_off, const float* s, const int32_t* s_off,
                            const int32_t* hq, const int32_t* hs) {
    if (P < 0 || n_q < 0 || n_s < 0) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (!q_off || !s_off || (n_q > 0 && !q) || (n_s > 0 && !s)) return DR_EINVAL;
    if (!knn_host_offsets_ok(hq, P, n_q) || !knn_host_offsets_ok(hs, P, n_s)) return DR_EINVAL;
    if (n_q > INT_MAX / 3 || n_s > INT_MAX / 3 || P > 65535) return DR_ENOSUP;
    return DR_OK;
}

static int knn_workspace_check(size_t need, const void* workspace, size_t workspace_bytes) {
    if (need == 0) return DR_OK;
    if (!workspace || workspace_bytes < need) return DR_EWORKSPACE;
    if (((uintptr_t)workspace & 15) != 0) return DR_EINVAL;
    return DR_OK;
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_knn_points_max_k(void) { return knn_max_k(); }
int dr_knn_points_tile(void) { return knn_tile(); }
int dr_knn_points_block(void) { return knn_block(); }

int dr_knn_points_f32(int P, int n_queries, const float* queries, const int32_t* q_offsets, int n_supports, const float* supports,
                      const int32_t* s_offsets, const int32_t* host_q_offsets, const int32_t* host_s_offsets, int k, float* out_distances,
                      int64_t* out_indices, int32_t* status, void* stream) {
    if (k < 1 || k > KNN_MAX_K) return DR_EINVAL;
    const int rc = knn_common_check(P, n_queries, n_supports, queries, q_offsets, supports, s_offsets, host_q_offsets, host_s_offsets);
    if (rc != DR_OK || P == 0) return rc;
    if (!status) return DR_EINVAL;
    KnnArgs A = {P, n_queries, n_supports, k, queries, q_offsets, supports, s_offsets, out_distances, (long long*)out_indices, 0.0f, nullptr};
    hipLaunchKernelGGL(knn_status_kernel, dim3((unsigned)P), dim3(KNN_THREADS), 0, (hipStream_t)stream, A, status);
    DR_LAUNCH_CHECK();
    if (!out_distances && !out_indices) return DR_OK;
    return knn_launch<false>(A, (hipStream_t)stream);
}

size_t dr_nn_stats_workspace_bytes(int P, int n_queries) { return nn_stats_workspace_bytes(P, n_queries); }

int dr_nn_stats_f32(int P, int n_queries, const float* queries, const int32_t* q_offsets, int n_supports, const float* supports,
                    const int32_t* s_offsets, const int32_t* host_q_offsets, const int32_t* host_s_offsets, float distance_limit, double* out,
                    int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = knn_common_check(P, n_queries, n_supports, queries, q_offsets, supports, s_offsets, host_q_offsets, host_s_offsets);
    if (rc != DR_OK || P == 0) return rc;
    if (!out || !status) return DR_EINVAL;
    const int wrc = knn_workspace_check(nn_stats_workspace_bytes(P, n_queries), workspace, workspace_bytes);
    if (wrc != DR_OK) return wrc;
    KnnArgs A = {P, n_queries, n_supports, 1, queries, q_offsets, supports, s_offsets, nullptr, nullptr, distance_limit, (double*)workspace};
    hipLaunchKernelGGL(knn_status_kernel, dim3((unsigned)P), dim3(KNN_THREADS), 0, (hipStream_t)stream, A, status);
    DR_LAUNCH_CHECK();
    const int lrc = knn_launch<true>(A, (hipStream_t)stream);
    if (lrc != DR_OK) return lrc;
    hipLaunchKernelGGL(knn_final_kernel, dim3((unsigned)((P * NN_SLOTS + 63) / 64)), dim3(64), 0, (hipStream_t)stream, P, q_offsets, n_queries,
                       KNN_BLOCK, NN_SLOTS, (const double*)workspace, out);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_flow_metrics_workspace_bytes(int P, int n_points) { return flow_metrics_workspace_bytes(P, n_points); }

int dr_flow_metrics_f32(int P, int n_points, const float* pred, const float* target, const int32_t* offsets, const int32_t* host_offsets,
                        const uint8_t* mask, const float* rot, const float* trn, float strict_abs, float strict_rel, float relaxed_abs,
                        float relaxed_rel, float outlier_abs, float outlier_rel, float eps, double* out, int32_t* status, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (P < 0 || n_points < 0) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (!offsets || !out || !status || (n_points > 0 && (!pred || !target)) || ((rot == nullptr) != (trn == nullptr))) return DR_EINVAL;
    if (!knn_host_offsets_ok(host_offsets, P, n_points)) return DR_EINVAL;
    if (n_points > INT_MAX / 3 || P > 65535) return DR_ENOSUP;
    const int wrc = knn_workspace_check(flow_metrics_workspace_bytes(P, n_points), workspace, workspace_bytes);
    if (wrc != DR_OK) return wrc;
    hipStream_t st = (hipStream_t)stream;
    FlowArgs A = {P, n_points, pred, target, offsets, mask, rot, trn, strict_abs, strict_rel, relaxed_abs, relaxed_rel, outlier_abs, outlier_rel,
                  eps, (double*)workspace};
    hipLaunchKernelGGL(flow_status_kernel, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, st, P, offsets, n_points, status);
    DR_LAUNCH_CHECK();
    const unsigned grid = (unsigned)knn_grid_bound(n_points, P, FLOW_BLOCK);
    hipLaunchKernelGGL(flow_metrics_kernel, dim3(grid), dim3(FLOW_BLOCK), 0, st, A);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_final_kernel, dim3((unsigned)((P * FLOW_SLOTS + 63) / 64)), dim3(64), 0, st, P, offsets, n_points, FLOW_BLOCK,
                       FLOW_SLOTS, (const double*)workspace, out);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
