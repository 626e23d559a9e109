// lgr.hip -- the RANSAC-free rigid estimators (twentieth set after ABI 0.7.0):
//   dr_weighted_procrustes_f32       vision3d.ops.weighted_procrustes                         2D-3D vision3d/ops/weighted_procrustes.py:10-71
//   dr_lgr_f32                       LocalGlobalRegistration.local_to_global_registration     2D-3D vision3d/models/geotransformer/local_global_registration.py:104-161
//   dr_spatial_consistency_f32       spatial_consistency, cross_spatial_consistency           2D-3D vision3d/ops/spatial_consistency.py:7-54
//   dr_sc_row_sums_f32               SpatialConsistencyFiltering's sc_score_mat.sum(dim=1)    2D-3D vision3d/models/geotransformer/spatial_consistency_filtering.py:15-19
//   dr_sc_leading_eigenvector_f32    leading_eigenvector(method="power")                      2D-3D vision3d/ops/eigenvector.py:21-31
// All are ragged over the problems of a call, asynchronous on the given stream, read nothing back to the host and use no floating-point atomic.
//
// The fit: every sum of a group runs in double in ONE order, whichever path serves the group.  Element i of the group belongs to slot
// (virtual wave (i / 64) % 4, lane i % 64); a slot adds its elements in ascending order, the 64 slots of a virtual wave meet in the tree
// lane l += lane l + off (off = 32 .. 1), and the four virtual waves are added in ascending order.  A short group is served by one physical
// wave that plays the four virtual waves in turn, a long one by the four waves of a workgroup that exchange their sums through LDS: the
// same additions in the same order, so the two paths are bit-equal.  The 3 x 3 SVD is svd3_jacobi in double, run redundantly by every lane
// on the same values, so nothing is broadcast.
//
// Every index below comes from lgr_index.h (walked on the host by tools/lgr_index_check.cpp).
#include <limits.h>
#include "common.h"
#include "kernels.h"
#include "svd3.h"
#include "lgr_index.h"
#include "../../include/diffreg_hip.h"

// the residual, the distances and the consistency value are written operation by operation (and the file is built with -ffp-contract=off)
#pragma clang fp contract(off)

namespace dr {

__device__ __forceinline__ float lgr_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// THE RESIDUAL RULE: T = R (row-major, 9) then t (3), already float32
__device__ __forceinline__ bool lgr_inlier(const float (&T)[12], const float* __restrict__ s, const float* __restrict__ t, float radius) {
    const float x = s[0], y = s[1], z = s[2];
    const float ax = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], x), __fmul_rn(T[1], y)), __fmul_rn(T[2], z)), T[9]);
    const float ay = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[3], x), __fmul_rn(T[4], y)), __fmul_rn(T[5], z)), T[10]);
    const float az = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[6], x), __fmul_rn(T[7], y)), __fmul_rn(T[8], z)), T[11]);
    return sqrtf(lgr_d2(t[0], t[1], t[2], ax, ay, az)) < radius;
}

__device__ __forceinline__ double lgr_wave_sum(double v) {
#pragma unroll
    for (int off = LGR_WAVE / 2; off >= 1; off >>= 1) v += __shfl_down(v, off, LGR_WAVE);
    return v;
}

// the sums of N terms over a group of n elements in the fixed order, by a team of NW physical waves (1: this wave alone, no barrier; 4: the
// workgroup, two barriers).  term(i, acc) adds element i's terms to acc.  Every lane of the team returns the same N sums.
template <int N, int NW, class F>
__device__ __forceinline__ void lgr_team_sum(int n, int lane, int w, double* ex, F term, double (&out)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) out[k] = 0.0;
    if (NW == 1) {
        for (int v = 0; v < LGR_VWAVES; ++v) {
            double acc[N];
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k] = 0.0;
            for (int i = lgr_slot_first(v, lane); i < n; i += LGR_STRIDE) term(i, acc);
#pragma unroll
            for (int k = 0; k < N; ++k) out[k] += __shfl(lgr_wave_sum(acc[k]), 0, LGR_WAVE);
        }
    } else {
        double acc[N];
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = 0.0;
        for (int i = lgr_slot_first(w, lane); i < n; i += LGR_STRIDE) term(i, acc);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double s = lgr_wave_sum(acc[k]);
            if (lane == 0) ex[lgr_exchange_word(N, w, k)] = s;
        }
        __syncthreads();
#pragma unroll
        for (int v = 0; v < LGR_VWAVES; ++v)
#pragma unroll
            for (int k = 0; k < N; ++k) out[k] += ex[lgr_exchange_word(N, v, k)];
        __syncthreads();                             // the exchange words are free again
    }
}

// rule 1 on a group of n rows at src / tgt (the group's first row), weights by weight(i) (float32, before the threshold).  T = R (9) and t (3),
// rounded once to float32; flags = 0, LGR_ST_NONFINITE (T untouched) or LGR_ST_DEGENERATE.
template <int NW, class W>
__device__ __forceinline__ void lgr_fit(const float* __restrict__ src, const float* __restrict__ tgt, int n, W weight, float thr, float eps,
                                        int lane, int w, double* ex, float (&T)[12], int& flags) {
    double s1[7];
    lgr_team_sum<7, NW>(n, lane, w, ex, [&](int i, double (&a)[7]) {
        const float wf = weight(i);
        const double wi = (double)(wf < thr ? 0.0f : wf);
        a[0] += wi;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a[1 + c] += wi * (double)src[knn_local_coord(i, c)];
            a[4 + c] += wi * (double)tgt[knn_local_coord(i, c)];
        }
    }, s1);
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) finite = finite && __builtin_isfinite(s1[k]);
    if (!finite) {                                   // a NaN / Inf coordinate or weight reaches a sum whatever its weight (0 * Inf = NaN)
        flags = LGR_ST_NONFINITE;
        return;
    }
    const double inv = 1.0 / (s1[0] + (double)eps);
    const double pc[3] = {s1[1] * inv, s1[2] * inv, s1[3] * inv}, qc[3] = {s1[4] * inv, s1[5] * inv, s1[6] * inv};
    double h[9];
    lgr_team_sum<9, NW>(n, lane, w, ex, [&](int i, double (&a)[9]) {
        const float wf = weight(i);
        const double wi = (double)(wf < thr ? 0.0f : wf) * inv;
        const double p0 = (double)src[knn_local_coord(i, 0)] - pc[0], p1 = (double)src[knn_local_coord(i, 1)] - pc[1];
        const double p2 = (double)src[knn_local_coord(i, 2)] - pc[2];
        const double q0 = wi * ((double)tgt[knn_local_coord(i, 0)] - qc[0]), q1 = wi * ((double)tgt[knn_local_coord(i, 1)] - qc[1]);
        const double q2 = wi * ((double)tgt[knn_local_coord(i, 2)] - qc[2]);
        a[0] += p0 * q0; a[1] += p0 * q1; a[2] += p0 * q2;
        a[3] += p1 * q0; a[4] += p1 * q1; a[5] += p1 * q2;
        a[6] += p2 * q0; a[7] += p2 * q1; a[8] += p2 * q2;
    }, h);
    bool zero = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) zero = zero && h[k] == 0.0;
    double R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    flags = 0;
    if (!(s1[0] > 0.0) || zero) {
        flags = LGR_ST_DEGENERATE;
    } else {
        double A[3][3] = {{h[0], h[1], h[2]}, {h[3], h[4], h[5]}, {h[6], h[7], h[8]}}, U[3][3], S[3], V[3][3];
        svd3_jacobi(A, U, S, V);
        double M[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) M[i][j] = V[i][0] * U[j][0] + V[i][1] * U[j][1] + V[i][2] * U[j][2];
        const double det = det3(M), d = det > 0.0 ? 1.0 : (det < 0.0 ? -1.0 : 0.0);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) R[i][j] = V[i][0] * U[j][0] + V[i][1] * U[j][1] + d * (V[i][2] * U[j][2]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) T[3 * i + j] = (float)R[i][j];
        T[9 + i] = (float)(qc[i] - (R[i][0] * pc[0] + R[i][1] * pc[1] + R[i][2] * pc[2]));
    }
}

__device__ __forceinline__ void lgr_store_transform(float* __restrict__ out, const float (&T)[12]) {
    float4* o = (float4*)out;                        // rows of 16 floats: 64-byte aligned when the array is 16-byte aligned
    o[0] = make_float4(T[0], T[1], T[2], T[9]);
    o[1] = make_float4(T[3], T[4], T[5], T[10]);
    o[2] = make_float4(T[6], T[7], T[8], T[11]);
    o[3] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
}
__device__ __forceinline__ void lgr_load_transform(const float* __restrict__ in, float (&T)[12]) {
    const float4* o = (const float4*)in;
    const float4 a = o[0], b = o[1], c = o[2];
    T[0] = a.x; T[1] = a.y; T[2] = a.z; T[9] = a.w;
    T[3] = b.x; T[4] = b.y; T[5] = b.z; T[10] = b.w;
    T[6] = c.x; T[7] = c.y; T[8] = c.z; T[11] = c.w;
}

struct ProcArgs {
    long long G;                 // groups, or -1: read from n_groups[0]
    const int32_t* n_groups;
    int n;
    const float* src;
    const float* tgt;
    const float* weights;        // or NULL
    const int32_t* lo;           // group g is rows [lo[g], hi[g]) of the stacked arrays (entry 1: hi = lo + 1)
    const int32_t* hi;
    float thr, eps;
    int wave_limit;
    float* T;                    // [G, 16]
    int32_t* status;             // [G] or NULL
};

// workgroup b serves groups [4 b, 4 b + 4): wave w fits group 4 b + w alone when it is short; the long ones are then fitted one after the
// other by all four waves (the branch is uniform over the workgroup: every thread reads the same four ranges)
__global__ __launch_bounds__(LGR_THREADS) void lgr_fit_kernel(ProcArgs A) {
    __shared__ double ex[LGR_EXCHANGE_WORDS];
    const long long G = A.G >= 0 ? A.G : (long long)A.n_groups[0];
    const int tid = threadIdx.x, lane = tid & (LGR_WAVE - 1), w = tid / LGR_WAVE;
    for (int s = 0; s < LGR_GROUPS_PER_BLOCK; ++s) {
        const long long g = lgr_fit_group(blockIdx.x, s);
        if (g >= G) break;                           // uniform
        const int lo = A.lo[g], hi = A.hi[g];
        const bool ok = nr_slice_ok(lo, hi, A.n);
        const int len = ok ? hi - lo : 0;
        const bool by_wave = lgr_uses_wave(len, A.wave_limit);
        if (by_wave && s != w) continue;             // a short group is the business of wave s alone (no barrier on this path)
        float T[12];
        int flags = LGR_ST_OFFSETS;
        if (ok) {
            const float* __restrict__ sp = A.src + knn_coord(lo, 0, 0);
            const float* __restrict__ tp = A.tgt + knn_coord(lo, 0, 0);
            const float* __restrict__ wp = A.weights ? A.weights + knn_row(lo, 0) : nullptr;
            auto weight = [&](int i) { return wp ? wp[i] : 1.0f; };
            if (by_wave) lgr_fit<1>(sp, tp, len, weight, A.thr, A.eps, lane, 0, ex, T, flags);
            else lgr_fit<LGR_VWAVES>(sp, tp, len, weight, A.thr, A.eps, lane, w, ex, T, flags);
        }
        if (lane == 0 && (by_wave || w == 0)) {
            if (A.status) A.status[g] = flags;
            if (!(flags & (LGR_ST_OFFSETS | LGR_ST_NONFINITE))) lgr_store_transform(A.T + lgr_transform_word(g, 0), T);
        }
    }
}

// exclusive scan of one flag per thread over the workgroup; total = the workgroup's count
__device__ __forceinline__ int lgr_block_scan(bool f, int* cnt, int lane, int w, int& total) {
    const unsigned long long m = __ballot(f);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                 // the previous round's counts have been read
    if (lane == 0) cnt[w] = __popcll(m);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int v = 0; v < LGR_VWAVES; ++v) {
        const int c = cnt[v];
        off += v < w ? c : 0;
        total += c;
    }
    return off + pre;
}

struct LgrArgs {
    int P, n_corr, n_verify;
    const float* src;
    const float* tgt;
    const float* scores;
    const int32_t* ids;
    const int32_t* c_off;
    const float* v_src;
    const float* v_tgt;
    const float* v_scores;
    const int32_t* v_off;
    float radius, thr, eps;
    int min_local, steps;
    float* transform;            // [P, 16]
    int32_t* best_chunk;         // [P] or NULL
    float* final_scores;         // [n_verify] or NULL
    int32_t* out_chunk_off;      // [P + 1] or NULL
    int32_t* status;             // [P]
    int32_t *starts, *chunk_lo, *chunk_hi, *n_chunks, *chunk_off, *dense_lo, *dense_hi, *dense_p, *counts;
    float* chunk_T;
};

__device__ __forceinline__ bool lgr_finite3(const float* p) { return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]); }

// launch 1, one workgroup per problem: the status word, then the problem's chunks by a count pass and a scan (twice: runs, then the runs
// that are long enough)
__global__ __launch_bounds__(LGR_THREADS) void lgr_scan_kernel(LgrArgs A) {
    __shared__ int cnt[LGR_VWAVES];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (LGR_WAVE - 1), w = tid / LGR_WAVE;
    int st = 0, nch = 0;
    if (!lgr_prefix_ok(A.c_off, p, A.n_corr) || !lgr_prefix_ok(A.v_off, p, A.n_verify)) {
        st = LGR_ST_OFFSETS;
    } else {
        const int clo = A.c_off[p], nc = A.c_off[p + 1] - clo, vlo = A.v_off[p], nv = A.v_off[p + 1] - vlo;
        if (nc == 0 || nv == 0) {
            st = LGR_ST_EMPTY;
        } else {
            const int32_t* __restrict__ ids = A.ids + knn_row(clo, 0);
            int bad = 0, desc = 0;
            for (int i = tid; i < nc; i += LGR_THREADS) {
                bad |= (lgr_finite3(A.src + knn_coord(clo, i, 0)) && lgr_finite3(A.tgt + knn_coord(clo, i, 0)) &&
                        __builtin_isfinite(A.scores[knn_row(clo, i)])) ? 0 : 1;
                desc |= (i > 0 && ids[i] < ids[i - 1]) ? 1 : 0;
            }
            for (int i = tid; i < nv; i += LGR_THREADS)
                bad |= (lgr_finite3(A.v_src + knn_coord(vlo, i, 0)) && lgr_finite3(A.v_tgt + knn_coord(vlo, i, 0)) &&
                        __builtin_isfinite(A.v_scores[knn_row(vlo, i)])) ? 0 : 1;
            if (__syncthreads_or(desc)) st |= LGR_ST_OFFSETS;
            if (__syncthreads_or(bad)) st |= LGR_ST_NONFINITE;
            if (st == 0) {
                int runs = 0, total;
                for (int t0 = 0; t0 < nc; t0 += LGR_THREADS) {
                    const int i = t0 + tid;
                    const bool f = i < nc && lgr_is_run_start(ids, i);
                    const int at = lgr_block_scan(f, cnt, lane, w, total);
                    if (f) A.starts[lgr_list_slot(clo, runs + at)] = i;
                    runs += total;
                }
                __syncthreads();                     // the run starts are visible to the workgroup
                for (int t0 = 0; t0 < runs; t0 += LGR_THREADS) {
                    const int r = t0 + tid;
                    int s = 0, e = 0;
                    if (r < runs) {
                        s = A.starts[lgr_list_slot(clo, r)];
                        e = r + 1 < runs ? A.starts[lgr_list_slot(clo, r + 1)] : nc;
                    }
                    const bool f = r < runs && e - s >= A.min_local;
                    const int at = lgr_block_scan(f, cnt, lane, w, total);
                    if (f) {
                        A.chunk_lo[lgr_list_slot(clo, nch + at)] = clo + s;
                        A.chunk_hi[lgr_list_slot(clo, nch + at)] = clo + e;
                    }
                    nch += total;
                }
            }
        }
    }
    if (tid == 0) {
        A.status[p] = st;
        A.n_chunks[p] = nch;
        if (st == LGR_ST_EMPTY) {
            const float I[12] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
            lgr_store_transform(A.transform + lgr_transform_word(p, 0), I);
            if (A.best_chunk) A.best_chunk[p] = -1;
        }
    }
}

// launch 2, one workgroup: the scan of the chunk counts over the problems, and the hypotheses in one dense list
__global__ __launch_bounds__(LGR_THREADS) void lgr_offsets_kernel(LgrArgs A) {
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int p = 0; p < A.P; ++p) {
            A.chunk_off[p] = acc;
            acc += A.n_chunks[p];                    // the valid problems are a prefix chain of slices (lgr_prefix_ok): acc <= n_corr
        }
        A.chunk_off[A.P] = acc;
    }
    __syncthreads();
    for (int p = threadIdx.x; p <= A.P; p += LGR_THREADS)
        if (A.out_chunk_off) A.out_chunk_off[p] = A.chunk_off[p];
    for (int p = 0; p < A.P; ++p) {
        const int n = A.n_chunks[p], first = A.chunk_off[p];
        if (n == 0) continue;
        const int clo = A.c_off[p];
        for (int j = threadIdx.x; j < n; j += LGR_THREADS) {
            A.dense_lo[first + j] = A.chunk_lo[lgr_list_slot(clo, j)];
            A.dense_hi[first + j] = A.chunk_hi[lgr_list_slot(clo, j)];
            A.dense_p[first + j] = p;
        }
    }
}

// launch 4, one wave per hypothesis: the integer count of the verification correspondences of its problem inside the radius
__global__ __launch_bounds__(LGR_THREADS) void lgr_verify_kernel(LgrArgs A) {
    const int lane = threadIdx.x & (LGR_WAVE - 1), w = threadIdx.x / LGR_WAVE;
    const long long g = lgr_fit_group(blockIdx.x, w);
    if (g >= A.chunk_off[A.P]) return;
    const int p = A.dense_p[g], vlo = A.v_off[p], nv = A.v_off[p + 1] - vlo;
    float T[12];
    lgr_load_transform(A.chunk_T + lgr_transform_word(g, 0), T);
    int count = 0;
    for (int i = lane; i < nv; i += LGR_WAVE)
        count += lgr_inlier(T, A.v_src + knn_coord(vlo, i, 0), A.v_tgt + knn_coord(vlo, i, 0), A.radius) ? 1 : 0;
#pragma unroll
    for (int off = LGR_WAVE / 2; off >= 1; off >>= 1) count += __shfl_down(count, off, LGR_WAVE);
    if (lane == 0) A.counts[g] = count;
}

// launch 5, one workgroup per problem: the best hypothesis (largest count, lowest chunk), or the degenerate branch's fit on the whole
// verification set; then every refinement round
__global__ __launch_bounds__(LGR_THREADS) void lgr_refine_kernel(LgrArgs A) {
    __shared__ double ex[LGR_EXCHANGE_WORDS];
    __shared__ int best_c[LGR_VWAVES], best_j[LGR_VWAVES];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (LGR_WAVE - 1), w = tid / LGR_WAVE;
    if (A.status[p] != 0) return;                    // uniform: written by launch 1
    const int vlo = A.v_off[p], nv = A.v_off[p + 1] - vlo;
    const float* __restrict__ sp = A.v_src + knn_coord(vlo, 0, 0);
    const float* __restrict__ tp = A.v_tgt + knn_coord(vlo, 0, 0);
    const float* __restrict__ sc = A.v_scores + knn_row(vlo, 0);
    const int nch = A.n_chunks[p], first = A.chunk_off[p];
    float T[12];
    int flags = 0;
    if (nch > 0) {
        int c = -1, j = INT_MAX;
        for (int k = tid; k < nch; k += LGR_THREADS) {
            const int ck = A.counts[first + k];
            if (ck > c) { c = ck; j = k; }           // ascending k: the first of equal counts stays
        }
#pragma unroll
        for (int off = LGR_WAVE / 2; off >= 1; off >>= 1) {
            const int c2 = __shfl_down(c, off, LGR_WAVE), j2 = __shfl_down(j, off, LGR_WAVE);
            if (c2 > c || (c2 == c && j2 < j)) { c = c2; j = j2; }
        }
        if (lane == 0) { best_c[w] = c; best_j[w] = j; }
        __syncthreads();
        c = best_c[0]; j = best_j[0];
#pragma unroll
        for (int v = 1; v < LGR_VWAVES; ++v)
            if (best_c[v] > c || (best_c[v] == c && best_j[v] < j)) { c = best_c[v]; j = best_j[v]; }
        lgr_load_transform(A.chunk_T + lgr_transform_word(first + j, 0), T);
        if (tid == 0 && A.best_chunk) A.best_chunk[p] = j;
    } else {
        lgr_fit<LGR_VWAVES>(sp, tp, nv, [&](int i) { return sc[i]; }, A.thr, A.eps, lane, w, ex, T, flags);
        if (tid == 0 && A.best_chunk) A.best_chunk[p] = -1;
    }
    for (int r = 0; r < A.steps; ++r) {
        auto cur = [&](int i) { return lgr_inlier(T, sp + knn_local_coord(i, 0), tp + knn_local_coord(i, 0), A.radius) ? sc[i] : 0.0f; };
        if (r == A.steps - 1 && A.final_scores)
            for (int i = tid; i < nv; i += LGR_THREADS) A.final_scores[knn_row(vlo, i)] = cur(i);
        float Tn[12];
        lgr_fit<LGR_VWAVES>(sp, tp, nv, cur, A.thr, A.eps, lane, w, ex, Tn, flags);
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = Tn[k];
    }
    if (tid == 0) {
        lgr_store_transform(A.transform + lgr_transform_word(p, 0), T);
        if (flags) A.status[p] = flags;
    }
}

// ---- spatial consistency
__device__ __forceinline__ float sc_value(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz, float dx,
                                          float dy, float dz, float sigma2) {
    const float ds = sqrtf(lgr_d2(ax, ay, az, cx, cy, cz)), dt = sqrtf(lgr_d2(bx, by, bz, dx, dy, dz));
    const float delta = fabsf(__fsub_rn(ds, dt));
    return fmaxf(__fsub_rn(1.0f, __fdiv_rn(__fmul_rn(delta, delta), sigma2)), 0.0f);
}

struct ScArgs {
    int P, n_q, n_s;
    const float* q_src;
    const float* q_tgt;
    const int32_t* q_off;
    const float* s_src;
    const float* s_tgt;
    const int32_t* s_off;
    float sigma2;
    const float* mult;           // [n_s] or NULL: the vector of the matrix-free product
    const int32_t* done;         // [P] or NULL: a problem whose flag is set is left alone
    const int32_t* status;       // [P]: a problem with a non-zero word is skipped
    float* out;                  // rows [n_q], or the dense matrices
    const int64_t* mat_off;      // dense: [P + 1] elements
};

// one workgroup per problem: bad offsets (4), a non-finite coordinate (8).  With v: the eigenvector's start (ones, the flag and the count cleared)
__global__ __launch_bounds__(LGR_THREADS) void sc_status_kernel(ScArgs A, int32_t* status, float* v, int32_t* done, int32_t* iterations) {
    const int p = blockIdx.x;
    const int qlo = A.q_off[p], qhi = A.q_off[p + 1], slo = A.s_off[p], shi = A.s_off[p + 1];
    int st = 0;
    if (!nr_slice_ok(qlo, qhi, A.n_q) || !nr_slice_ok(slo, shi, A.n_s)) {
        st = LGR_ST_OFFSETS;
    } else {
        int bad = 0;
        if (A.q_src)
            for (int i = threadIdx.x; i < qhi - qlo; i += LGR_THREADS)
                bad |= (lgr_finite3(A.q_src + knn_coord(qlo, i, 0)) && lgr_finite3(A.q_tgt + knn_coord(qlo, i, 0))) ? 0 : 1;
        if (A.s_src && A.s_src != A.q_src)
            for (int i = threadIdx.x; i < shi - slo; i += LGR_THREADS)
                bad |= (lgr_finite3(A.s_src + knn_coord(slo, i, 0)) && lgr_finite3(A.s_tgt + knn_coord(slo, i, 0))) ? 0 : 1;
        if (__syncthreads_or(bad)) st = LGR_ST_NONFINITE;
        if (v && st == 0)
            for (int i = threadIdx.x; i < qhi - qlo; i += LGR_THREADS) v[knn_row(qlo, i)] = 1.0f;
    }
    if (threadIdx.x == 0) {
        status[p] = st;
        if (done) done[p] = 0;
        if (iterations) iterations[p] = 0;
    }
}

__global__ __launch_bounds__(SC_DENSE_THREADS) void sc_dense_kernel(ScArgs A) {
    int p, block;
    if (!knn_block_to_pair(A.P, A.q_off, A.n_q, SC_BLOCK, blockIdx.x, p, block)) return;
    if (A.status[p] != 0) return;
    const int qlo = A.q_off[p], Q = A.q_off[p + 1] - qlo, slo = A.s_off[p], S = A.s_off[p + 1] - slo;
    const long long base = A.mat_off[p];
    const int rows = sc_block_rows(Q, block);
    const long long cells = (long long)rows * S;
    for (long long e = threadIdx.x; e < cells; e += SC_DENSE_THREADS) {
        const int r = (int)(e / S), j = (int)(e - (long long)r * S), i = sc_query_of(block, r);
        const float* a = A.q_src + knn_coord(qlo, i, 0);
        const float* b = A.q_tgt + knn_coord(qlo, i, 0);
        const float* c = A.s_src + knn_coord(slo, j, 0);
        const float* d = A.s_tgt + knn_coord(slo, j, 0);
        A.out[sc_dense_at(base, S, i, j)] = sc_value(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], d[0], d[1], d[2], A.sigma2);
    }
}

// one wave per block of SC_BLOCK queries, lane l owns query l; the supports of both point sets (and the multiplier) pass through LDS in tiles;
// a query's sum runs in double over the supports in ascending order
__global__ __launch_bounds__(SC_BLOCK) void sc_row_sums_kernel(ScArgs A) {
    __shared__ float lds[SC_LDS_WORDS];
    int p, block;
    if (!knn_block_to_pair(A.P, A.q_off, A.n_q, SC_BLOCK, blockIdx.x, p, block)) return;
    if (A.status[p] != 0 || (A.done && A.done[p] != 0)) return;        // uniform over the workgroup
    const int qlo = A.q_off[p], Q = A.q_off[p + 1] - qlo, slo = A.s_off[p], S = A.s_off[p + 1] - slo;
    const int lane = threadIdx.x, qi = sc_query_of(block, lane);
    const bool owns = qi < Q;
    const float* __restrict__ qa = A.q_src + knn_coord(qlo, owns ? qi : 0, 0);
    const float* __restrict__ qb = A.q_tgt + knn_coord(qlo, owns ? qi : 0, 0);
    const float ax = qa[0], ay = qa[1], az = qa[2], bx = qb[0], by = qb[1], bz = qb[2];      // Q >= 1 here: row 0 exists
    const float* __restrict__ sa = A.s_src + knn_coord(slo, 0, 0);
    const float* __restrict__ sb = A.s_tgt + knn_coord(slo, 0, 0);
    const float* __restrict__ sm = A.mult ? A.mult + knn_row(slo, 0) : nullptr;
    double acc = 0.0;
    const int tiles = sc_tiles(S);
    for (int t = 0; t < tiles; ++t) {
        const int count = sc_tile_count(S, t);
        if (t > 0) __syncthreads();
        for (int e = lane; e < count; e += SC_BLOCK) {
            const int r = sc_support_of(t, e);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lds[sc_lds_word(c, e)] = sa[knn_local_coord(r, c)];
                lds[sc_lds_word(3 + c, e)] = sb[knn_local_coord(r, c)];
            }
            lds[sc_lds_word(6, e)] = sm ? sm[r] : 1.0f;
        }
        __syncthreads();
#pragma unroll 4
        for (int e = 0; e < count; ++e) {
            const float v = sc_value(ax, ay, az, bx, by, bz, lds[sc_lds_word(0, e)], lds[sc_lds_word(1, e)], lds[sc_lds_word(2, e)],
                                     lds[sc_lds_word(3, e)], lds[sc_lds_word(4, e)], lds[sc_lds_word(5, e)], A.sigma2);
            acc += (double)v * (double)lds[sc_lds_word(6, e)];
        }
    }
    if (owns) A.out[knn_row(qlo, qi)] = (float)acc;
}

struct EigArgs {
    int P, n;
    const int32_t* off;
    const float* mat;
    const int64_t* mat_off;
    float* v;                    // [n]
    float* y;                    // [n]
    int32_t* done;
    int32_t* iterations;
    const int32_t* status;
};

// the caller's own matrix: a wave owns a row; lane l adds columns l, l + 64, ... in ascending order, then the tree
__global__ __launch_bounds__(LGR_THREADS) void eig_dense_kernel(EigArgs A) {
    int p, block;
    if (!knn_block_to_pair(A.P, A.off, A.n, EIG_ROWS_PER_BLOCK, blockIdx.x, p, block)) return;
    if (A.status[p] != 0 || A.done[p] != 0) return;
    const int lo = A.off[p], N = A.off[p + 1] - lo;
    const int lane = threadIdx.x & (LGR_WAVE - 1), row = eig_row_of(block, threadIdx.x / LGR_WAVE);
    if (row >= N) return;
    double acc = 0.0;
    for (int j = lane; j < N; j += LGR_WAVE) acc += (double)A.mat[sc_dense_at(A.mat_off[p], N, row, j)] * (double)A.v[knn_row(lo, j)];
    acc = lgr_wave_sum(acc);
    if (lane == 0) A.y[knn_row(lo, row)] = (float)acc;
}

// one workgroup per problem: F.normalize (eps 1e-12) of y into v, and torch.allclose(v, v_last) under its defaults
__global__ __launch_bounds__(LGR_THREADS) void eig_norm_kernel(EigArgs A, int it) {
    __shared__ double ex[LGR_EXCHANGE_WORDS];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (LGR_WAVE - 1), w = tid / LGR_WAVE;
    if (A.status[p] != 0 || A.done[p] != 0) return;  // uniform
    const int lo = A.off[p], N = A.off[p + 1] - lo;
    const float* __restrict__ y = A.y + knn_row(lo, 0);
    float* __restrict__ v = A.v + knn_row(lo, 0);
    double s[1];
    lgr_team_sum<1, LGR_VWAVES>(N, lane, w, ex, [&](int i, double (&a)[1]) { a[0] += (double)y[i] * (double)y[i]; }, s);
    const float den = fmaxf((float)sqrt(s[0]), 1e-12f);
    int far = 0;
    for (int i = tid; i < N; i += LGR_THREADS) {
        const float now = __fdiv_rn(y[i], den), last = v[i];
        far |= (fabsf(__fsub_rn(now, last)) <= __fadd_rn(1e-8f, __fmul_rn(1e-5f, fabsf(last)))) ? 0 : 1;
        v[i] = now;
    }
    far = __syncthreads_or(far);
    if (tid == 0) {
        A.iterations[p] = it + 1;
        if (!far) A.done[p] = 1;
    }
}

static bool lgr_host_offsets_ok(const int32_t* h, int P, int total) {
    if (!h) return true;
    if (h[0] < 0 || h[P] > total) return false;
    for (int p = 0; p < P; ++p)
        if (h[p + 1] < h[p]) return false;
    return true;
}

static int lgr_workspace_check(size_t need, const void* workspace, size_t workspace_bytes) {
    if (need == 0) return DR_OK;
    if (!workspace || workspace_bytes < need) return DR_EWORKSPACE;
    if (((uintptr_t)workspace & 15) != 0) return DR_EINVAL;
    return DR_OK;
}

static int sc_common_check(int P, int n_q, int n_s, const void* qa, const void* qb, const int32_t* q_off, const void* sa, const void* sb,
                           const int32_t* s_off, const int32_t* hq, const int32_t* hs, float sigma) {
    if (P < 0 || n_q < 0 || n_s < 0 || !(sigma > 0.0f)) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (!q_off || !s_off || (n_q > 0 && (!qa || !qb)) || (n_s > 0 && (!sa || !sb))) return DR_EINVAL;
    if (!lgr_host_offsets_ok(hq, P, n_q) || !lgr_host_offsets_ok(hs, P, n_s)) return DR_EINVAL;
    if (n_q > INT_MAX / 3 || n_s > INT_MAX / 3 || P > 65535) return DR_ENOSUP;
    return DR_OK;
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_lgr_wave_limit(void) { return lgr_wave_limit(); }
int dr_sc_block(void) { return sc_block(); }
int dr_sc_tile(void) { return sc_tile(); }

int dr_weighted_procrustes_f32(int G, int n, const float* src, const float* tgt, const float* weights, const int32_t* offsets,
                               const int32_t* host_offsets, float weight_threshold, float eps, int wave_limit, float* transforms,
                               int32_t* status, void* stream) {
    if (G < 0 || n < 0) return DR_EINVAL;
    if (G == 0) return DR_OK;
    if (!offsets || !transforms || !status || (n > 0 && (!src || !tgt))) return DR_EINVAL;
    if (!lgr_host_offsets_ok(host_offsets, G, n)) return DR_EINVAL;
    if (n > INT_MAX / 3) return DR_ENOSUP;
    if (((uintptr_t)transforms & 15) != 0) return DR_EINVAL;
    ProcArgs A = {G, nullptr, n, src, tgt, weights, offsets, offsets + 1, weight_threshold, eps, wave_limit < 0 ? LGR_WAVE_LIMIT : wave_limit,
                  transforms, status};
    hipLaunchKernelGGL(lgr_fit_kernel, dim3((unsigned)lgr_fit_blocks(G)), dim3(LGR_THREADS), 0, (hipStream_t)stream, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_lgr_workspace_bytes(int P, int n_corr) { return lgr_carve(P, n_corr).total; }

int dr_lgr_f32(int P, int n_corr, const float* src_points, const float* tgt_points, const float* scores, const int32_t* patch_ids,
               const int32_t* corr_offsets, int n_verify, const float* v_src_points, const float* v_tgt_points, const float* v_scores,
               const int32_t* verify_offsets, const int32_t* host_corr_offsets, const int32_t* host_verify_offsets, float acceptance_radius,
               int min_local_correspondences, int num_refinement_steps, float weight_threshold, float eps, float* transform,
               int32_t* best_chunk, float* final_scores, float* chunk_transforms, int32_t* chunk_counts, int32_t* chunk_offsets,
               int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || n_corr < 0 || n_verify < 0 || min_local_correspondences < 1 || num_refinement_steps < 1 ||
        num_refinement_steps > LGR_MAX_STEPS)
        return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (!corr_offsets || !verify_offsets || !transform || !status) return DR_EINVAL;
    if (n_corr > 0 && (!src_points || !tgt_points || !scores || !patch_ids)) return DR_EINVAL;
    if (n_verify > 0 && (!v_src_points || !v_tgt_points || !v_scores)) return DR_EINVAL;
    if (!lgr_host_offsets_ok(host_corr_offsets, P, n_corr) || !lgr_host_offsets_ok(host_verify_offsets, P, n_verify)) return DR_EINVAL;
    if (n_corr > INT_MAX / 16 || n_verify > INT_MAX / 3 || P > 65535) return DR_ENOSUP;
    if (((uintptr_t)transform & 15) != 0 || ((uintptr_t)chunk_transforms & 15) != 0) return DR_EINVAL;
    const LgrCarve c = lgr_carve(P, n_corr);
    const int wrc = lgr_workspace_check(c.total, workspace, workspace_bytes);
    if (wrc != DR_OK) return wrc;
    char* ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    LgrArgs A = {P, n_corr, n_verify, src_points, tgt_points, scores, patch_ids, corr_offsets, v_src_points, v_tgt_points, v_scores,
                 verify_offsets, acceptance_radius, weight_threshold, eps, min_local_correspondences, num_refinement_steps, transform,
                 best_chunk, final_scores, chunk_offsets, status, (int32_t*)(ws + c.starts), (int32_t*)(ws + c.chunk_lo),
                 (int32_t*)(ws + c.chunk_hi), (int32_t*)(ws + c.n_chunks), (int32_t*)(ws + c.chunk_off), (int32_t*)(ws + c.dense_lo),
                 (int32_t*)(ws + c.dense_hi), (int32_t*)(ws + c.dense_p), chunk_counts ? chunk_counts : (int32_t*)(ws + c.counts),
                 chunk_transforms ? chunk_transforms : (float*)(ws + c.transforms)};
    hipLaunchKernelGGL(lgr_scan_kernel, dim3((unsigned)P), dim3(LGR_THREADS), 0, st, A);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(lgr_offsets_kernel, dim3(1), dim3(LGR_THREADS), 0, st, A);
    DR_LAUNCH_CHECK();
    const long long bound = lgr_chunk_bound(n_corr, min_local_correspondences);
    if (bound > 0) {
        ProcArgs F = {-1, A.chunk_off + P, n_corr, src_points, tgt_points, scores, A.dense_lo, A.dense_hi, weight_threshold, eps,
                      LGR_WAVE_LIMIT, A.chunk_T, nullptr};
        hipLaunchKernelGGL(lgr_fit_kernel, dim3((unsigned)lgr_fit_blocks(bound)), dim3(LGR_THREADS), 0, st, F);
        DR_LAUNCH_CHECK();
        hipLaunchKernelGGL(lgr_verify_kernel, dim3((unsigned)lgr_fit_blocks(bound)), dim3(LGR_THREADS), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lgr_refine_kernel, dim3((unsigned)P), dim3(LGR_THREADS), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_spatial_consistency_f32(int P, int n_queries, const float* q_src_points, const float* q_tgt_points, const int32_t* q_offsets,
                               int n_supports, const float* s_src_points, const float* s_tgt_points, const int32_t* s_offsets,
                               const int32_t* host_q_offsets, const int32_t* host_s_offsets, float sigma, const int64_t* mat_offsets, float* out,
                               int32_t* status, void* stream) {
    const int rc = sc_common_check(P, n_queries, n_supports, q_src_points, q_tgt_points, q_offsets, s_src_points, s_tgt_points, s_offsets,
                                   host_q_offsets, host_s_offsets, sigma);
    if (rc != DR_OK || P == 0) return rc;
    if (!status || !mat_offsets || (n_queries > 0 && n_supports > 0 && !out)) return DR_EINVAL;
    ScArgs A = {P, n_queries, n_supports, q_src_points, q_tgt_points, q_offsets, s_src_points, s_tgt_points, s_offsets, sigma * sigma, nullptr,
                nullptr, status, out, mat_offsets};
    hipLaunchKernelGGL(sc_status_kernel, dim3((unsigned)P), dim3(LGR_THREADS), 0, (hipStream_t)stream, A, status, nullptr, nullptr, nullptr);
    DR_LAUNCH_CHECK();
    const unsigned grid = (unsigned)knn_grid_bound(n_queries, P, SC_BLOCK);
    hipLaunchKernelGGL(sc_dense_kernel, dim3(grid), dim3(SC_DENSE_THREADS), 0, (hipStream_t)stream, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_sc_row_sums_f32(int P, int n_queries, const float* q_src_points, const float* q_tgt_points, const int32_t* q_offsets, int n_supports,
                       const float* s_src_points, const float* s_tgt_points, const int32_t* s_offsets, const int32_t* host_q_offsets,
                       const int32_t* host_s_offsets, float sigma, const float* multiplier, float* out, int32_t* status, void* stream) {
    const int rc = sc_common_check(P, n_queries, n_supports, q_src_points, q_tgt_points, q_offsets, s_src_points, s_tgt_points, s_offsets,
                                   host_q_offsets, host_s_offsets, sigma);
    if (rc != DR_OK || P == 0) return rc;
    if (!status || (n_queries > 0 && !out)) return DR_EINVAL;
    ScArgs A = {P, n_queries, n_supports, q_src_points, q_tgt_points, q_offsets, s_src_points, s_tgt_points, s_offsets, sigma * sigma,
                multiplier, nullptr, status, out, nullptr};
    hipLaunchKernelGGL(sc_status_kernel, dim3((unsigned)P), dim3(LGR_THREADS), 0, (hipStream_t)stream, A, status, nullptr, nullptr, nullptr);
    DR_LAUNCH_CHECK();
    const unsigned grid = (unsigned)knn_grid_bound(n_queries, P, SC_BLOCK);
    hipLaunchKernelGGL(sc_row_sums_kernel, dim3(grid), dim3(SC_BLOCK), 0, (hipStream_t)stream, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_sc_leading_eigenvector_workspace_bytes(int P, int n) { return eig_carve(P, n).total; }

int dr_sc_leading_eigenvector_f32(int P, int n, const float* src_points, const float* tgt_points, const int32_t* offsets,
                                  const int32_t* host_offsets, float sigma, const float* mat, const int64_t* mat_offsets, int num_iterations,
                                  float* out, int32_t* iterations, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || n < 0 || num_iterations < 0) return DR_EINVAL;
    if (P == 0) return DR_OK;
    const bool dense = mat != nullptr;
    if (!offsets || !iterations || !status || (n > 0 && !out)) return DR_EINVAL;
    if (dense ? (!mat_offsets || src_points || tgt_points) : (!(sigma > 0.0f) || (n > 0 && (!src_points || !tgt_points)))) return DR_EINVAL;
    if (!lgr_host_offsets_ok(host_offsets, P, n)) return DR_EINVAL;
    if (n > INT_MAX / 3 || P > 65535) return DR_ENOSUP;
    const EigCarve c = eig_carve(P, n);
    const int wrc = lgr_workspace_check(c.total, workspace, workspace_bytes);
    if (wrc != DR_OK) return wrc;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* y = (float*)(ws + c.y);
    int32_t* done = (int32_t*)(ws + c.done);
    ScArgs S = {P, n, n, src_points, tgt_points, offsets, src_points, tgt_points, offsets, sigma * sigma, out, done, status, y, nullptr};
    EigArgs E = {P, n, offsets, mat, mat_offsets, out, y, done, iterations, status};
    hipLaunchKernelGGL(sc_status_kernel, dim3((unsigned)P), dim3(LGR_THREADS), 0, st, S, status, out, done, iterations);
    DR_LAUNCH_CHECK();
    for (int it = 0; it < num_iterations; ++it) {
        if (dense) {
            hipLaunchKernelGGL(eig_dense_kernel, dim3((unsigned)knn_grid_bound(n, P, EIG_ROWS_PER_BLOCK)), dim3(LGR_THREADS), 0, st, E);
        } else {
            hipLaunchKernelGGL(sc_row_sums_kernel, dim3((unsigned)knn_grid_bound(n, P, SC_BLOCK)), dim3(SC_BLOCK), 0, st, S);
        }
        DR_LAUNCH_CHECK();
        hipLaunchKernelGGL(eig_norm_kernel, dim3((unsigned)P), dim3(LGR_THREADS), 0, st, E, it);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

}  // extern "C"
