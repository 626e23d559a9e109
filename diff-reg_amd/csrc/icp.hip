// icp.hip -- multi-pair point-to-point ICP on the device (twenty-first set after ABI 0.7.0):
//   dr_icp_p2p_f32     the loop of Open3D's registration_icp with TransformationEstimationPointToPoint(False), which the reference runs
//                      per scale in multi_scale_icp                                     2D-3D vision3d/utils/open3d.py:378-396
// Ragged over P pairs through int32 device offsets, asynchronous on the given stream, nothing allocated, nothing read back, no floating-point
// atomic: two runs are bit-equal and the call can be captured on one stream.  The rule is stated in include/diffreg_hip.h.
//
// The targets never move: their grid is built once per call by launch_target_grid (item3d.hip), the grid of dr_radius_pairs_ragged_f32 with
// the cell edge r (1 + 2^-7).  Every evaluation is two launches:
//   (A) icp_sweep_kernel   a workgroup owns ICP_BLOCK_ROWS source rows of ONE pair, a wave one row at a time: it moves the row by the pair's
//                          transform (the float32 residual rule), sweeps the 27 cells about it as nine runs of the sorted keys, keeps per lane
//                          the unsigned 64-bit minimum of (bits(d2) << 32 | pair-local target) over the candidates with d2 < r^2 (d2 >= 0: the
//                          bits order as the values do), and meets the other lanes in a wave minimum.  The wave adds the row's count, d2, p, q
//                          and p q^T (p, q about the pair's grid origin) to 17 doubles in registers, rows ascending; the four waves are
//                          added ascending into the workgroup's partial: an order that depends on the shapes alone.
//   (B) icp_finish_kernel  one wave per pair: slot k of the pair's partials is added by lane k, blocks ascending; H from the moments in double,
//                          svd3_jacobi, T = update * T in double rounded once; fitness, rmse, iterations, the stop test and the DEVICE done flag.
// Later launches leave a finished pair untouched.  LDS: 4 x 17 doubles (544 bytes) in the sweep, 17 doubles in the finish.
//
// Every index below comes from icp_index.h (walked on the host by tools/icp_index_check.cpp).
#include <limits.h>
#include "common.h"
#include "kernels.h"
#include "svd3.h"
#include "icp_index.h"
#include "../../include/diffreg_hip.h"

// the move and the distance are written operation by operation (and the file is built with -ffp-contract=off)
#pragma clang fp contract(off)

namespace dr {
namespace {

struct IcpArgs {
    int P, ns, nt;
    const float* src; const int32_t* s_off;
    const float* tgt; const int32_t* t_off;
    const float* init;
    float cell, r2, rel_fitness, rel_rmse;
    int max_it;
    float* T; float* fitness; float* rmse; int32_t* iterations; int32_t* corr; int32_t* status;
    float4* origin; unsigned long long* keys; float4* sorted; double* partial; int32_t* done;
};

__device__ __forceinline__ bool icp_finite3(const float* p) { return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]); }

__device__ __forceinline__ void icp_store_transform(float* __restrict__ out, const float (&T)[12]) {      // R (9) then t (3) -> a 4 x 4 row
    float4* o = (float4*)out;
    o[0] = make_float4(T[0], T[1], T[2], T[9]);
    o[1] = make_float4(T[3], T[4], T[5], T[10]);
    o[2] = make_float4(T[6], T[7], T[8], T[11]);
    o[3] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
}
__device__ __forceinline__ void icp_load_transform(const float* __restrict__ in, float (&T)[12]) {
    const float4* o = (const float4*)in;
    const float4 a = o[0], b = o[1], c = o[2];
    T[0] = a.x; T[1] = a.y; T[2] = a.z; T[9] = a.w;
    T[3] = b.x; T[4] = b.y; T[5] = b.z; T[10] = b.w;
    T[6] = c.x; T[7] = c.y; T[8] = c.z; T[11] = c.w;
}

// set-up, one workgroup per pair: the status word (bad offsets 4, a non-finite coordinate or initial transform 8), the cleared flag and
// count, and the pair's starting transform.  A skipped pair has none of its outputs but the status word written.
__global__ __launch_bounds__(ICP_THREADS) void icp_status_kernel(IcpArgs A) {
    const int p = blockIdx.x, tid = threadIdx.x;
    int st = 0;
    // thread 0 alone walks the offsets up to the pair (O(p) reads); the workgroup shares its answer
    const int bad_off = (tid == 0 && (!lgr_prefix_ok(A.s_off, p, A.ns) || !lgr_prefix_ok(A.t_off, p, A.nt))) ? 1 : 0;
    if (__syncthreads_or(bad_off)) {
        st = ICP_ST_OFFSETS;
    } else {
        const int s0 = A.s_off[p], n_src = A.s_off[p + 1] - s0, t0 = A.t_off[p], n_tgt = A.t_off[p + 1] - t0;
        int bad = 0;
        for (int i = tid; i < n_src; i += ICP_THREADS) bad |= icp_finite3(A.src + knn_coord(s0, i, 0)) ? 0 : 1;
        for (int i = tid; i < n_tgt; i += ICP_THREADS) bad |= icp_finite3(A.tgt + knn_coord(t0, i, 0)) ? 0 : 1;
        if (A.init && tid < 12) bad |= __builtin_isfinite(A.init[lgr_transform_word(p, tid)]) ? 0 : 1;
        if (__syncthreads_or(bad)) st = ICP_ST_NONFINITE;
    }
    if (tid != 0) return;
    A.status[p] = st;
    A.done[p] = 0;
    if (st != 0) return;
    A.iterations[p] = 0;
    float T[12] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
    if (A.init) icp_load_transform(A.init + lgr_transform_word(p, 0), T);
    icp_store_transform(A.T + lgr_transform_word(p, 0), T);
}

// (A)
__global__ __launch_bounds__(ICP_THREADS) void icp_sweep_kernel(IcpArgs A) {
    __shared__ double ex[ICP_LDS_WORDS];
    int p, block;
    if (!knn_block_to_pair(A.P, A.s_off, A.ns, ICP_BLOCK_ROWS, blockIdx.x, p, block)) return;
    if ((A.status[p] & ICP_ST_SKIP) != 0 || A.done[p] != 0) return;                   // uniform over the workgroup
    const int lane = lane_id(), w = wave_id();
    const int s0 = A.s_off[p], n_src = A.s_off[p + 1] - s0, t0 = A.t_off[p], n_tgt = A.t_off[p + 1] - t0;
    float T[12];
    icp_load_transform(A.T + lgr_transform_word(p, 0), T);
    const float4 o = A.origin[p];
    double acc[ICP_SLOTS];
#pragma unroll
    for (int k = 0; k < ICP_SLOTS; ++k) acc[k] = 0.0;
    for (int j = 0; j < ICP_ROWS_PER_WAVE; ++j) {
        const int i = icp_row_of(block, w, j);
        if (i >= n_src) break;                                                         // uniform over the wave
        const float* __restrict__ s = A.src + knn_coord(s0, i, 0);
        const float x = s[0], y = s[1], z = s[2];
        // THE RESIDUAL RULE of dr_lgr_f32
        const float px = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], x), __fmul_rn(T[1], y)), __fmul_rn(T[2], z)), T[9]);
        const float py = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[3], x), __fmul_rn(T[4], y)), __fmul_rn(T[5], z)), T[10]);
        const float pz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[6], x), __fmul_rn(T[7], y)), __fmul_rn(T[8], z)), T[11]);
        unsigned long long best = ~0ull;
        if (n_tgt > 0) {
            const int cx = it3_cell(px, o.x, A.cell), cy = it3_cell(py, o.y, A.cell), cz = it3_cell(pz, o.z, A.cell);
            // lanes 0..8 find the start of run `lane`, lanes 9..17 the end of run `lane - 9`, over ALL sorted targets (the pair is in the key)
            const int r = lane < 9 ? lane : lane - 9;
            unsigned long long first = 0, last = 0;
            int pos = 0;
            if (lane < 18 && it3_run_keys(p, cx, cy, cz, r, first, last))
                pos = lane < 9 ? it3_lower_bound(A.keys, 0, A.nt, first) : it3_lower_bound(A.keys, 0, A.nt, last + 1);
            const int end = __shfl(pos, lane + 9 < ICP_WAVE ? lane + 9 : lane);
            const int run_lo = pos, run_hi = end > pos ? end : pos;                    // meaningful on lanes 0..8
            for (int q = 0; q < 9; ++q) {
                const int lo = __shfl(run_lo, q), hi = __shfl(run_hi, q);
                for (int base = lo; base < hi; base += ICP_WAVE) {
                    const int c = base + lane;
                    if (c < hi) {
                        const float4 t = A.sorted[c];
                        const float dx = __fsub_rn(px, t.x), dy = __fsub_rn(py, t.y), dz = __fsub_rn(pz, t.z);
                        const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
                        if (d2 < A.r2) {
                            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) |
                                                           (unsigned long long)(__float_as_uint(t.w) - (unsigned)t0);
                            best = key < best ? key : best;
                        }
                    }
                }
            }
            best = wave_min(best);
        }
        const bool has = best != ~0ull;
        const int partner = has ? (int)(unsigned)(best & 0xffffffffull) : -1;
        if (lane == 0 && A.corr) A.corr[knn_row(s0, i)] = partner;
        if (has) {                                                                     // uniform: every lane adds the same doubles
            const float* __restrict__ t = A.tgt + knn_coord(t0, partner, 0);
            const double d2 = (double)__uint_as_float((unsigned)(best >> 32));
            // about the pair's grid origin o, the min corner of its targets (float32 differences are exact in double): smaller terms, so
            // less cancellation in H; a target coordinate that EQUALS o's over all partners (one target; targets on a line or plane along
            // an axis) gives an exactly zero column of H, and ONE correspondence an exactly zero H.  Elsewhere a rank-deficient H is
            // rank-deficient only up to rounding of the moments.
            const double pd[3] = {(double)px - (double)o.x, (double)py - (double)o.y, (double)pz - (double)o.z};
            const double qd[3] = {(double)t[0] - (double)o.x, (double)t[1] - (double)o.y, (double)t[2] - (double)o.z};
            acc[0] += 1.0;
            acc[1] += d2;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                acc[2 + a] += pd[a];
                acc[5 + a] += qd[a];
#pragma unroll
                for (int b = 0; b < 3; ++b) acc[8 + 3 * a + b] += pd[a] * qd[b];
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < ICP_SLOTS; ++k) ex[icp_exchange_word(w, k)] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < ICP_SLOTS) {
        double s = ex[icp_exchange_word(0, threadIdx.x)];
        for (int v = 1; v < ICP_WAVES; ++v) s += ex[icp_exchange_word(v, threadIdx.x)];
        A.partial[knn_partial(blockIdx.x, ICP_SLOTS, threadIdx.x)] = s;
    }
}

// (B): the evaluation under the transform after `k` fits, the stop test, and fit k + 1.  ICP_FINISH_THREADS must stay ONE wave (64): every
// lane reads fitness[p] / rmse[p] of the previous evaluation before lane 0 overwrites them, which only lockstep within a wave orders.
__global__ __launch_bounds__(ICP_FINISH_THREADS) void icp_finish_kernel(IcpArgs A, int k) {
    __shared__ double m[ICP_SLOTS];
    const int p = blockIdx.x, tid = threadIdx.x;
    int st = A.status[p];
    if ((st & ICP_ST_SKIP) != 0 || A.done[p] != 0) return;                             // uniform
    const int s0 = A.s_off[p], n_src = A.s_off[p + 1] - s0;
    if (tid < ICP_SLOTS) {
        const long long first = knn_first_block(p, A.s_off, A.ns, ICP_BLOCK_ROWS);
        const int blocks = knn_blocks(n_src, ICP_BLOCK_ROWS);
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += A.partial[knn_partial(first + b, ICP_SLOTS, tid)];
        m[tid] = s;
    }
    __syncthreads();
    const double n = m[0];
    const float fit = n_src > 0 ? (float)(n / (double)n_src) : 0.0f;
    const float rmse = n > 0.0 ? (float)sqrt(m[1] / n) : 0.0f;
    bool stop = false;
    if (k > 0) {                                                                       // float32 compares against the previous result
        const float df = fabsf(__fsub_rn(A.fitness[p], fit)), dr = fabsf(__fsub_rn(A.rmse[p], rmse));
        stop = df < A.rel_fitness && dr < A.rel_rmse;
    }
    if (!(n > 0.0)) {
        st |= ICP_ST_EMPTY;
        stop = true;
    }
    float T[12];
    const bool fits = !stop && k < A.max_it;
    if (fits) {
        float Tc[12];
        icp_load_transform(A.T + lgr_transform_word(p, 0), Tc);
        // rule 1 with unit weights and eps = 0, H from the moments about the pair's grid origin o (H does not depend on o)
        const float4 o4 = A.origin[p];
        const double o[3] = {(double)o4.x, (double)o4.y, (double)o4.z};
        const double inv = 1.0 / n;
        const double pc[3] = {m[2] / n, m[3] / n, m[4] / n}, qc[3] = {m[5] / n, m[6] / n, m[7] / n};
        double H[3][3];
        bool zero = true;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                H[a][b] = (m[8 + 3 * a + b] - m[2 + a] * qc[b]) * inv;
                zero = zero && H[a][b] == 0.0;
            }
        double R[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        if (zero) {
            st |= ICP_ST_DEGENERATE;
        } else {
            double U[3][3], S[3], V[3][3];
            svd3_jacobi(H, U, S, V);
            if (S[1] <= ICP_RANK_TOL * S[0]) st |= ICP_ST_DEGENERATE;
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
        // T = update * T, in double on the float32 current transform, rounded once
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double tu = (qc[i] + o[i]) - (R[i][0] * (pc[0] + o[0]) + R[i][1] * (pc[1] + o[1]) + R[i][2] * (pc[2] + o[2]));
#pragma unroll
            for (int j = 0; j < 3; ++j)
                T[3 * i + j] = (float)(R[i][0] * (double)Tc[j] + R[i][1] * (double)Tc[3 + j] + R[i][2] * (double)Tc[6 + j]);
            T[9 + i] = (float)((R[i][0] * (double)Tc[9] + R[i][1] * (double)Tc[10] + R[i][2] * (double)Tc[11]) + tu);
        }
    }
    if (tid != 0) return;
    A.fitness[p] = fit;
    A.rmse[p] = rmse;
    A.status[p] = st;
    if (fits) {
        icp_store_transform(A.T + lgr_transform_word(p, 0), T);
        A.iterations[p] = k + 1;
    } else {
        A.done[p] = 1;
    }
}

bool icp_host_offsets_ok(const int32_t* h, int P, int total) {
    if (!h) return true;
    if (h[0] < 0 || h[P] > total) return false;
    for (int p = 0; p < P; ++p)
        if (h[p + 1] < h[p]) return false;
    return true;
}

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" {

size_t dr_icp_p2p_workspace_bytes(int P, int ns, int nt) { return icp_carve(P, ns, nt).bytes; }

int dr_icp_p2p_f32(int P, int ns, const float* src, const int32_t* s_offsets, int nt, const float* tgt, const int32_t* t_offsets,
                   const int32_t* host_s_offsets, const int32_t* host_t_offsets, const float* init_transforms,
                   float max_correspondence_distance, int max_iteration, float relative_fitness, float relative_rmse, float* transforms,
                   float* fitness, float* inlier_rmse, int32_t* iterations, int32_t* correspondence, int32_t* status, void* workspace,
                   size_t workspace_bytes, void* stream) {
    const float r = max_correspondence_distance;
    if (P < 0 || ns < 0 || nt < 0 || max_iteration < 0 || max_iteration > ICP_MAX_ITERATIONS || !(r > 0.0f) || !__builtin_isfinite(r) ||
        !(relative_fitness >= 0.0f) || !(relative_rmse >= 0.0f))
        return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (!s_offsets || !t_offsets || !transforms || !fitness || !inlier_rmse || !iterations || !status || (ns > 0 && !src) || (nt > 0 && !tgt))
        return DR_EINVAL;
    if (!icp_host_offsets_ok(host_s_offsets, P, ns) || !icp_host_offsets_ok(host_t_offsets, P, nt)) return DR_EINVAL;
    if (P > ICP_MAX_PAIRS || ns > INT_MAX / 3 || nt > INT_MAX / 3) return DR_ENOSUP;
    if (!aligned_to(transforms, 16) || !aligned_to(init_transforms, 16)) return DR_EINVAL;
    const IcpCarve c = icp_carve(P, ns, nt);
    if (!workspace || workspace_bytes < c.bytes) return DR_EWORKSPACE;
    if (!aligned_to(workspace, 16)) return DR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    IcpArgs A;
    A.P = P; A.ns = ns; A.nt = nt;
    A.src = src; A.s_off = s_offsets; A.tgt = tgt; A.t_off = t_offsets; A.init = init_transforms;
    A.cell = r * (1.0f + 1.0f / 128.0f); A.r2 = r * r; A.rel_fitness = relative_fitness; A.rel_rmse = relative_rmse;
    A.max_it = max_iteration;
    A.T = transforms; A.fitness = fitness; A.rmse = inlier_rmse; A.iterations = iterations; A.corr = correspondence; A.status = status;
    A.origin = (float4*)(ws + c.origin); A.keys = (unsigned long long*)(ws + c.keys); A.sorted = (float4*)(ws + c.sorted);
    A.partial = (double*)(ws + c.partial); A.done = (int32_t*)(ws + c.done);
    hipLaunchKernelGGL(icp_status_kernel, dim3((unsigned)P), dim3(ICP_THREADS), 0, st, A);
    DR_LAUNCH_CHECK();
    const int grc = launch_target_grid(P, nt, tgt, t_offsets, A.cell, A.origin, A.keys, (unsigned*)(ws + c.vals), A.sorted, st);
    if (grc != DR_OK) return grc;
    const unsigned grid = (unsigned)icp_grid(ns, P);
    for (int k = 0; k <= max_iteration; ++k) {                   // evaluation k runs under the transform after k fits
        hipLaunchKernelGGL(icp_sweep_kernel, dim3(grid), dim3(ICP_THREADS), 0, st, A);
        DR_LAUNCH_CHECK();
        hipLaunchKernelGGL(icp_finish_kernel, dim3((unsigned)P), dim3(ICP_FINISH_THREADS), 0, st, A, k);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

}  // extern "C"
