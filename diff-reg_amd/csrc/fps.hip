// fps.hip -- furthest-point sampling (seventeenth set after ABI 0.7.0):
//   dr_fps_nodes_f32   sample_nodes_with_fps / native_furthest_point_sample   2D-3D vision3d/csrc/cpu/node_sampling/node_sampling.cpp:10-78,
//                                                                              vision3d/array_ops/furthest_point_sample.py:22-66
//   dr_fps_batch_f32   furthest_point_sample_kernel                           2D-3D vision3d/csrc/cuda/furthest_point_sample/
//                                                                              furthest_point_sample_cuda.cuh:29-88
// Both are ragged over the clouds of a call, asynchronous on the given stream, read nothing back to the host and use no atomic of any kind.
//
// ONE workgroup of FPS_BLOCK threads owns a cloud for all its iterations; clouds of a call run side by side on different compute units.  The
// loop is serial in the selections, so what an iteration costs is what the kernel costs:
//   1. every lane updates d[i] = min(d[i], dist(p_i, p_last)) for its points and keeps its best (distance, index, x, y, z);
//   2. a wave arg-max by DPP (quad_perm, row_half_mirror, row_mirror inside a row of 16 lanes, v_readlane across the four rows);
//   3. the lane that owns the wave's winner writes it, coordinates included, to the wave's LDS row;
//   4. ONE barrier;
//   5. every wave reads the 16 rows, reduces them by the same DPP steps and reads the winner's coordinates from its row: the next p_last.
// The rows are double-buffered by iteration parity (fps_index.h says why one barrier is then enough).
//
// The on-chip form keeps coordinates and running distances of up to FPS_CAPACITY points in registers (FPS_SLOTS points per lane); the streaming
// form is the same kernel with the running distances in the workspace and the coordinates re-read each iteration.  Both evaluate the same
// float32 expressions per point and reduce by the same key (distance descending, index ascending), a strict total order: the result does not
// depend on lane, wave or form.
//
// Every index below comes from fps_index.h (walked on the host by tools/fps_index_check.cpp).
#include <limits.h>
#include "common.h"
#include "kernels.h"
#include "fps_index.h"
#include "../../include/diffreg_hip.h"

// the distance is written operation by operation (and the file is built with -ffp-contract=off): nothing becomes an FMA
#pragma clang fp contract(off)

namespace dr {

constexpr int FPS_ST_SIZE = 1;   // status bit: the cloud has more points than the call's max_points: nothing is computed
constexpr int FPS_NONE = INT_MAX;   // index of "no candidate"

struct FpsArgs {
    int P, n_points, max_points, N;      // N: points per cloud of the batch form
    const float* points;
    const int32_t* p_off;                // NULL in the batch form
    float min_distance;
    int num_samples, cap;                // cap: row length of the outputs (sample_cap; num_samples in the batch form)
    long long* out_idx;
    float* out_pts;
    float* out_dist;
    int32_t* counts;
    int32_t* status;
    float* work;                         // running distances of the streaming form
    int force_streaming;
};

// BATCH: the squared distance of .cuh:64, (x1 - x2) (x1 - x2) + (y1 - y2) (y1 - y2) + (z1 - z2) (z1 - z2) with 1 = the last selection;
// otherwise std::sqrt((cur - point).sq_norm()) of node_sampling.cpp:51, sq_norm = x x + y y + z z (cloud.h:46).  sqrtf is correctly rounded.
template <bool BATCH>
__device__ __forceinline__ float fps_dist(float x, float y, float z, float lx, float ly, float lz) {
    const float dx = __fsub_rn(lx, x), dy = __fsub_rn(ly, y), dz = __fsub_rn(lz, z);
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return BATCH ? s : sqrtf(s);
}

__device__ __forceinline__ bool fps_finite3(float x, float y, float z) {
    return __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
}

// (d, i) beats (bd, bi): further, or as far with the lower index
__device__ __forceinline__ bool fps_beats(float d, int i, float bd, int bi) { return d > bd || (d == bd && i < bi); }

constexpr int FPS_DPP_XOR1 = 0xB1;          // quad_perm [1, 0, 3, 2]
constexpr int FPS_DPP_XOR2 = 0x4E;          // quad_perm [2, 3, 0, 1]
constexpr int FPS_DPP_HALF_MIRROR = 0x141;  // lane l of 8 <-> 7 - l: pairs the two reduced quads
constexpr int FPS_DPP_MIRROR = 0x140;       // lane l of 16 <-> 15 - l: pairs the two reduced halves

template <int CTRL>
__device__ __forceinline__ int fps_dpp(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }

// one exchange step of the arg-max; w is a payload that travels with the winner
template <int CTRL>
__device__ __forceinline__ void fps_step(float& d, int& i, int& w) {
    const float od = __int_as_float(fps_dpp<CTRL>(__float_as_int(d)));
    const int oi = fps_dpp<CTRL>(i), ow = fps_dpp<CTRL>(w);
    const bool take = fps_beats(od, oi, d, i);
    d = take ? od : d;
    i = take ? oi : i;
    w = take ? ow : w;
}

// after this every lane of a row of 16 holds the row's winner; must be called by all 64 lanes
__device__ __forceinline__ void fps_row_argmax(float& d, int& i, int& w) {
    fps_step<FPS_DPP_XOR1>(d, i, w);
    fps_step<FPS_DPP_XOR2>(d, i, w);
    fps_step<FPS_DPP_HALF_MIRROR>(d, i, w);
    fps_step<FPS_DPP_MIRROR>(d, i, w);
}

// the wave's winner from the four rows' winners, uniform over the wave
__device__ __forceinline__ void fps_wave_argmax(float& d, int& i) {
    int w = 0;
    fps_row_argmax(d, i, w);
    float bd = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 0));
    int bi = __builtin_amdgcn_readlane(i, 0);
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        const float od = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 16 * r));
        const int oi = __builtin_amdgcn_readlane(i, 16 * r);
        const bool take = fps_beats(od, oi, bd, bi);
        bd = take ? od : bd;
        bi = take ? oi : bi;
    }
    d = bd;
    i = bi;
}

// the rows behind a cloud's count, its count and its status word (node form)
__device__ __forceinline__ void fps_finish(const FpsArgs& A, int p, int count, int st) {
    const int tid = threadIdx.x;
    for (int k = count + tid; k < A.cap; k += FPS_BLOCK) {
        A.out_idx[fps_out(p, A.cap, k)] = -1;
        if (A.out_pts) {
            A.out_pts[fps_out_coord(p, A.cap, k, 0)] = 0.0f;
            A.out_pts[fps_out_coord(p, A.cap, k, 1)] = 0.0f;
            A.out_pts[fps_out_coord(p, A.cap, k, 2)] = 0.0f;
        }
        if (A.out_dist) A.out_dist[fps_out(p, A.cap, k)] = 0.0f;
    }
    if (tid == 0) {
        A.counts[p] = count;
        A.status[p] = st;
    }
}

// one cloud of n > 0 points, all its iterations.  S: the slots a lane keeps (a compile-time count: the slot loops carry no test, and the arrays
// stay in registers); the on-chip form needs n <= S FPS_BLOCK.  The streaming form keeps nothing (S = 1, unused).
template <bool ONCHIP, bool BATCH, int S>
__device__ __forceinline__ void fps_cloud(const FpsArgs& A, int* lds, int p, int lo, int n, int st) {
    const int tid = threadIdx.x, lane = tid & (FPS_WAVE - 1), wave = tid / FPS_WAVE;
    const float thresh = BATCH ? -1.0f : 0.0f;         // a candidate has to lie strictly beyond it (.cuh:56, node_sampling.cpp:47)
    const float init = BATCH ? 1e10f : INFINITY;       // ops/furthest_point_sample.py:34; array_ops/furthest_point_sample.py:30
    // the cloud's own rows: a uniform base and a 32-bit offset per lane (3 n < 2^31 is checked by the entries)
    const float* __restrict__ pts = A.points + fps_coord(lo, 0, 0);
    float* __restrict__ work = ONCHIP ? nullptr : A.work + fps_row(lo, 0);
    float x[S], y[S], z[S], d[S];
    int bad = 0;
    // a point with a NaN / Inf coordinate, and a slot behind the cloud, carries the running distance -inf for good: fminf keeps it there
    // whatever the distance evaluates to, so it is never a candidate
    if (ONCHIP) {
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const int i = fps_point_of(tid, k);
            const bool in = i < n;
            const int r = in ? i : 0;                    // a slot behind the cloud reads row 0 and is never a candidate
            x[k] = pts[fps_local_coord(r, 0)];
            y[k] = pts[fps_local_coord(r, 1)];
            z[k] = pts[fps_local_coord(r, 2)];
            const bool fin = fps_finite3(x[k], y[k], z[k]);
            d[k] = (in && fin) ? init : -INFINITY;
            bad |= (in && !fin) ? 1 : 0;
            __builtin_amdgcn_sched_barrier(0);           // one slot's addresses at a time
        }
    } else {
        for (int i = tid; i < n; i += FPS_BLOCK) {       // a thread re-reads only what it wrote itself: no barrier is needed for `work`
            const bool fin = fps_finite3(pts[fps_local_coord(i, 0)], pts[fps_local_coord(i, 1)], pts[fps_local_coord(i, 2)]);
            work[i] = fin ? init : -INFINITY;
            bad |= fin ? 0 : 1;
        }
    }
    if (__syncthreads_or(bad)) st |= FPS_ST_NONFINITE;

    float lx = pts[fps_local_coord(0, 0)], ly = pts[fps_local_coord(0, 1)], lz = pts[fps_local_coord(0, 2)];
    const float p0x = lx, p0y = ly, p0z = lz;
    const bool start_ok = BATCH || fps_finite3(lx, ly, lz);
    if (!start_ok) st |= FPS_ST_START;

    int count = 0;
    if (start_ok && A.cap > 0) {
        if (tid == 0) {
            A.out_idx[fps_out(p, A.cap, 0)] = 0;
            if (A.out_pts) {
                A.out_pts[fps_out_coord(p, A.cap, 0, 0)] = lx;
                A.out_pts[fps_out_coord(p, A.cap, 0, 1)] = ly;
                A.out_pts[fps_out_coord(p, A.cap, 0, 2)] = lz;
            }
            if (A.out_dist) A.out_dist[fps_out(p, A.cap, 0)] = 0.0f;
        }
        count = 1;
        // the batch form takes exactly num_samples (= cap); the node form stops at num_samples BEFORE the scan (node_sampling.cpp:44)
        const int limit = BATCH ? A.cap : (A.num_samples > 0 ? A.num_samples : INT_MAX);
        int parity = 0;
        while (count < limit) {
            float bd = thresh, bx = 0.0f, by = 0.0f, bz = 0.0f;
            int bi = FPS_NONE;
            if (ONCHIP) {
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const float nd = fminf(d[k], fps_dist<BATCH>(x[k], y[k], z[k], lx, ly, lz));
                    d[k] = nd;
                    const bool take = nd > bd;   // slots ascend in index: strict > keeps the lowest index of equal distances
                    bd = take ? nd : bd;
                    bi = take ? fps_point_of(tid, k) : bi;
                    bx = take ? x[k] : bx;
                    by = take ? y[k] : by;
                    bz = take ? z[k] : bz;
                }
            } else {
                for (int i = tid; i < n; i += FPS_BLOCK) {
                    const float px = pts[fps_local_coord(i, 0)], py = pts[fps_local_coord(i, 1)], pz = pts[fps_local_coord(i, 2)];
                    const float nd = fminf(work[i], fps_dist<BATCH>(px, py, pz, lx, ly, lz));
                    work[i] = nd;
                    if (nd > bd) {
                        bd = nd;
                        bi = i;
                        bx = px;
                        by = py;
                        bz = pz;
                    }
                }
            }
            float wd = bd;
            int wi = bi;
            fps_wave_argmax(wd, wi);
            // exactly one lane owns the wave's winner (indices are distinct); lane 0 writes the row of a wave without a candidate
            if (wi == FPS_NONE ? lane == 0 : bi == wi) {
                lds[fps_partial_word(parity, wave, 0)] = __float_as_int(bd);
                lds[fps_partial_word(parity, wave, 1)] = bi;
                lds[fps_partial_word(parity, wave, 2)] = __float_as_int(bx);
                lds[fps_partial_word(parity, wave, 3)] = __float_as_int(by);
                lds[fps_partial_word(parity, wave, 4)] = __float_as_int(bz);
            }
            __syncthreads();
            int ww = lane & (FPS_WAVES - 1);
            wd = __int_as_float(lds[fps_partial_word(parity, ww, 0)]);
            wi = lds[fps_partial_word(parity, ww, 1)];
            fps_row_argmax(wd, wi, ww);          // FPS_WAVES == 16: one DPP row holds every wave's partial
            if (wi == FPS_NONE) {
                if (!BATCH) break;               // every remaining distance is 0 (or the point cannot be a candidate): the cloud is used up
                wi = 0;                          // .cuh:55, 85: besti stays 0
                wd = thresh;
                lx = p0x; ly = p0y; lz = p0z;
            } else {
                if (!BATCH && wd < A.min_distance) break;                       // node_sampling.cpp:67
                if (!BATCH && count >= A.cap) { st |= FPS_ST_CAP; break; }      // the stop rule has not been met, the row is full
                lx = __int_as_float(lds[fps_partial_word(parity, ww, 2)]);
                ly = __int_as_float(lds[fps_partial_word(parity, ww, 3)]);
                lz = __int_as_float(lds[fps_partial_word(parity, ww, 4)]);
            }
            if (tid == 0) {
                A.out_idx[fps_out(p, A.cap, count)] = wi;
                if (A.out_pts) {
                    A.out_pts[fps_out_coord(p, A.cap, count, 0)] = lx;
                    A.out_pts[fps_out_coord(p, A.cap, count, 1)] = ly;
                    A.out_pts[fps_out_coord(p, A.cap, count, 2)] = lz;
                }
                if (A.out_dist) A.out_dist[fps_out(p, A.cap, count)] = wd;
            }
            ++count;
            parity ^= 1;
        }
    }
    if (!BATCH) fps_finish(A, p, count, st);
}

template <bool ONCHIP, bool BATCH>
__global__ __launch_bounds__(FPS_BLOCK) void fps_kernel(FpsArgs A) {
    __shared__ int lds[FPS_LDS_WORDS];
    const int p = blockIdx.x;
    int lo, n, st = 0;
    if (BATCH) {
        lo = fps_batch_lo(p, A.N);
        n = A.N;                             // > 0: the entry refuses an empty batch cloud
    } else {
        lo = A.p_off[p];
        const int hi = A.p_off[p + 1];
        n = hi - lo;
        if (!nr_slice_ok(lo, hi, A.n_points)) { st = FPS_ST_OFFSETS; lo = 0; n = 0; }
        else if (n > A.max_points) { st = FPS_ST_SIZE; n = 0; }
    }
    // a cloud belongs to exactly one of the two instantiations (both are launched with one workgroup per cloud)
    if ((A.force_streaming ? false : fps_fits_onchip(n)) != ONCHIP) return;
    if (n == 0) {
        fps_finish(A, p, 0, st);
        return;
    }
    if (!ONCHIP) {
        fps_cloud<false, BATCH, 1>(A, lds, p, lo, n, st);
        return;
    }
    const int nslots = fps_slots_used(n);    // uniform over the workgroup
    if (nslots <= 1) fps_cloud<true, BATCH, 1>(A, lds, p, lo, n, st);
    else if (nslots <= 2) fps_cloud<true, BATCH, 2>(A, lds, p, lo, n, st);
    else if (nslots <= 4) fps_cloud<true, BATCH, 4>(A, lds, p, lo, n, st);
    else if (nslots <= 9) fps_cloud<true, BATCH, 9>(A, lds, p, lo, n, st);
    else fps_cloud<true, BATCH, FPS_SLOTS>(A, lds, p, lo, n, st);
}

static int g_fps_force_streaming = 0;
void fps_force_streaming(int on) { g_fps_force_streaming = on != 0; }

template <bool BATCH>
static int fps_launch(const FpsArgs& A, hipStream_t st) {
    if (!A.force_streaming) {
        hipLaunchKernelGGL((fps_kernel<true, BATCH>), dim3((unsigned)A.P), dim3(FPS_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    if (A.force_streaming || !fps_fits_onchip(A.max_points)) {
        hipLaunchKernelGGL((fps_kernel<false, BATCH>), dim3((unsigned)A.P), dim3(FPS_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

// a missing or short workspace, where one is needed
static int fps_workspace_check(size_t need, const void* workspace, size_t workspace_bytes) {
    if (need == 0) return DR_OK;
    if (!workspace || workspace_bytes < need) return DR_EWORKSPACE;
    if (((uintptr_t)workspace & 15) != 0) return DR_EINVAL;
    return DR_OK;
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_fps_onchip_capacity(void) { return fps_onchip_capacity(); }

size_t dr_fps_workspace_bytes(int P, int n_points, int max_points) {
    if (P <= 0) return 0;
    return fps_workspace_bytes(n_points, max_points, g_fps_force_streaming != 0);
}

int dr_fps_nodes_f32(int P, int n_points, int max_points, const float* points, const int32_t* p_offsets, float min_distance, int num_samples,
                     int sample_cap, int64_t* out_indices, float* out_points, float* out_distances, int32_t* out_counts, int32_t* status,
                     void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || n_points < 0 || max_points < 0 || max_points > n_points) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (sample_cap < 1 || !p_offsets || !out_indices || !out_counts || !status || (n_points > 0 && !points)) return DR_EINVAL;
    // with neither stop rule the reference indexes out of range once every distance is 0 (array_ops/furthest_point_sample.py:34 on an empty list)
    if (!(min_distance > 0.0f) && num_samples <= 0) return DR_EINVAL;
    if (n_points > INT_MAX / 3 || P > 65535) return DR_ENOSUP;
    const int rc = fps_workspace_check(fps_workspace_bytes(n_points, max_points, g_fps_force_streaming != 0), workspace, workspace_bytes);
    if (rc != DR_OK) return rc;
    FpsArgs A = {P, n_points, max_points, 0, points, p_offsets, min_distance, num_samples, sample_cap, (long long*)out_indices, out_points,
                 out_distances, out_counts, status, (float*)workspace, g_fps_force_streaming};
    return fps_launch<false>(A, (hipStream_t)stream);
}

int dr_fps_batch_f32(int B, int N, int num_samples, const float* points, int64_t* out_indices, void* workspace, size_t workspace_bytes,
                     void* stream) {
    if (B < 0 || N < 0 || num_samples < 0) return DR_EINVAL;
    if (B == 0 || num_samples == 0) return DR_OK;
    if (N == 0 || !points || !out_indices) return DR_EINVAL;        // the reference's kernel reads point 0 of every cloud
    if ((long long)B * N > INT_MAX / 3 || B > 65535) return DR_ENOSUP;
    const int rc = fps_workspace_check(fps_workspace_bytes(B * N, N, g_fps_force_streaming != 0), workspace, workspace_bytes);
    if (rc != DR_OK) return rc;
    FpsArgs A = {B, B * N, N, N, points, nullptr, 0.0f, num_samples, num_samples, (long long*)out_indices, nullptr, nullptr, nullptr, nullptr,
                 (float*)workspace, g_fps_force_streaming};
    return fps_launch<true>(A, (hipStream_t)stream);
}

}  // extern "C"
