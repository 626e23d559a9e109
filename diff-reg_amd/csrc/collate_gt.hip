// collate_gt.hip -- the ground-truth half of the 3D / 4D training collate on the device (eleventh set after ABI 0.7.0):
//   dr_blend_flow_knn3_f32     blend_scene_flow(query, reference, reference_flow, knn=3)            3D/datasets/utils.py:23-59
//   dr_coarse_gt_matches_f32   the per-pair block of collate_fn_3dmatch / collate_fn_4dmatch          3D/datasets/dataloader.py:253-257, 512-520
//                              + multual_nn_correspondence(..., knn=1)                                3D/datasets/utils.py:62-80
// Both are ragged over P pairs in one call (offset arrays of P + 1 int32 entries on the device), asynchronous on the given stream, and read
// nothing back to the host.  No atomics of any kind: two runs are bit-equal.
//
// Every index below comes from collate_gt_index.h (walked on the host by tools/collate_gt_index_check.cpp).  One query per thread; the pair's
// reference cloud streams through LDS in stages of CG_STAGE float4 points; every lane reads the same LDS address at the same time (a broadcast
// ds_read_b128 per reference point) and keeps a running nearest / three nearest by insertion.  The top-3 insertion is the one nrfmr_kernel of
// metrics.hip writes inline for its anchors; that kernel reads its anchors through a match list and is left as it is.
#include "common.h"
#include "collate_gt_index.h"
#include "../../include/diffreg_hip.h"

// The float32 expressions restate numpy operation by operation: no a * b + c below becomes an FMA.
#pragma clang fp contract(off)

namespace dr {

constexpr int CG_ST_FEW = 1;      // status bit: the pair has too few points for the reference's argpartition (nothing is computed)
constexpr int CG_ST_OFFSETS = 2;  // status bit: the pair's offsets do not describe a slice of the stacked array (nothing is read)

// (dx dx + dy dy) + dz dz: np.sum((reference - query) ** 2, -1) over an axis of three
__device__ __forceinline__ float cg_d2(float rx, float ry, float rz, float qx, float qy, float qz) {
    const float dx = rx - qx, dy = ry - qy, dz = rz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// a source point as the ground-truth block sees it: p + flow (4D), then ((r0 x + r1 y) + r2 z) + t per row
__device__ __forceinline__ void cg_warp(const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ p,
                                        const float* __restrict__ f, float& ox, float& oy, float& oz) {
    float x = p[0], y = p[1], z = p[2];
    if (f) {
        x = x + f[0];
        y = y + f[1];
        z = z + f[2];
    }
    ox = ((R[0] * x + R[1] * y) + R[2] * z) + T[0];
    oy = ((R[3] * x + R[4] * y) + R[5] * z) + T[1];
    oz = ((R[6] * x + R[7] * y) + R[8] * z) + T[2];
}

// ------------------------------------------------------------------------------------------------------------
// blend_scene_flow, knn = 3
// ------------------------------------------------------------------------------------------------------------
struct BlendArgs {
    int P, nq, nr;
    const float* query; const int* q_off;
    const float* ref; const float* ref_flow; const int* r_off;
    float* out; int* status;
};

__global__ __launch_bounds__(CG_BLOCK) void blend_flow_knn3_kernel(BlendArgs A) {
    __shared__ float4 s_ref[CG_STAGE];
    int pair, tile;
    if (!cg_tile_to_pair(A.P, A.q_off, A.nq, blockIdx.x, pair, tile)) return;
    const int t = threadIdx.x;
    const int q0 = A.q_off[pair], q1 = A.q_off[pair + 1], r0 = A.r_off[pair], r1 = A.r_off[pair + 1];
    const bool ok = cg_slice_ok(q0, q1, A.nq) && cg_slice_ok(r0, r1, A.nr);
    const int Q = ok ? q1 - q0 : 0, K = ok ? r1 - r0 : 0;
    const int st = !ok ? CG_ST_OFFSETS : (K < 4 ? CG_ST_FEW : 0);      // np.argpartition(kth=3) needs 4 references (utils.py:13)
    if (tile == 0 && t == 0) A.status[pair] = st;
    if (st) return;
    const int q = tile * CG_BLOCK + t;
    const bool active = q < Q;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (active) {
        const float* p = A.query + (size_t)(q0 + q) * 3;
        qx = p[0]; qy = p[1]; qz = p[2];
    }
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = 0, i1 = 0, i2 = 0;
    for (int k0 = 0; k0 < K; k0 += CG_STAGE) {
        const int nk = cg_stage_count(K, k0);
        for (int k = t; k < nk; k += CG_BLOCK) {
            const float* p = A.ref + (size_t)(r0 + k0 + k) * 3;
            s_ref[k] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
        if (active) {
            for (int k = 0; k < nk; ++k) {
                const float4 r = s_ref[k];
                const float d = cg_d2(r.x, r.y, r.z, qx, qy, qz);
                if (d < d2) {       // ascending insertion; equal distances keep the lower index first
                    if (d < d1) {
                        d2 = d1; i2 = i1;
                        if (d < d0) { d1 = d0; i1 = i0; d0 = d; i0 = k0 + k; }
                        else { d1 = d; i1 = k0 + k; }
                    } else { d2 = d; i2 = k0 + k; }
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    float dd[3] = {sqrtf(d0), sqrtf(d1), sqrtf(d2)};
    const int id[3] = {i0, i1, i2};
    float w[3];
#pragma unroll
    for (int n = 0; n < 3; ++n) {
        if (dd[n] < 1e-10f) dd[n] = 1e-10f;             // utils.py:54
        w[n] = 1.0f / dd[n];
    }
    const float ws = (w[0] + w[1]) + w[2];
#pragma unroll
    for (int n = 0; n < 3; ++n) w[n] = w[n] / ws;
    const float* f0 = A.ref_flow + (size_t)(r0 + id[0]) * 3;
    const float* f1 = A.ref_flow + (size_t)(r0 + id[1]) * 3;
    const float* f2 = A.ref_flow + (size_t)(r0 + id[2]) * 3;
    float* o = A.out + (size_t)(q0 + q) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (f0[c] * w[0] + f1[c] * w[1]) + f2[c] * w[2];
}

// ------------------------------------------------------------------------------------------------------------
// coarse ground-truth matches: nearest target of every warped source, nearest warped source of every target, the mutual ones inside the radius
// ------------------------------------------------------------------------------------------------------------
struct MatchArgs {
    int P, ns, nt;
    const float* src; const int* s_off;
    const float* tgt; const int* t_off;
    const float* flow; const float* rot; const float* trn;
    float radius;
    int* nn_st; float* d2_st; int* nn_ts;
    long long* out_src; long long* out_tgt; int* counts; int* status;
};

__device__ __forceinline__ int cg_match_status(const MatchArgs& A, int pair, int& s0, int& S, int& t0, int& T) {
    s0 = A.s_off[pair];
    t0 = A.t_off[pair];
    const int s1 = A.s_off[pair + 1], t1 = A.t_off[pair + 1];
    if (!cg_slice_ok(s0, s1, A.ns) || !cg_slice_ok(t0, t1, A.nt)) {
        S = T = 0;
        return CG_ST_OFFSETS;
    }
    S = s1 - s0;
    T = t1 - t0;
    return (S < 2 || T < 2) ? CG_ST_FEW : 0;            // np.argpartition(kth=1) needs 2 points on either side (utils.py:13)
}

// DIR 0: queries = warped sources, references = targets (-> nn_st, d2_st); DIR 1: queries = targets, references = warped sources (-> nn_ts)
template <int DIR>
__global__ __launch_bounds__(CG_BLOCK) void match_nn_kernel(MatchArgs A) {
    __shared__ float4 s_ref[CG_STAGE];
    int pair, tile;
    if (!cg_tile_to_pair(A.P, DIR == 0 ? A.s_off : A.t_off, DIR == 0 ? A.ns : A.nt, blockIdx.x, pair, tile)) return;
    int s0, S, t0, T;
    if (cg_match_status(A, pair, s0, S, t0, T)) return;
    const int t = threadIdx.x;
    const float* R = A.rot + (size_t)pair * 9;
    const float* Tr = A.trn + (size_t)pair * 3;
    const int Q = DIR == 0 ? S : T, K = DIR == 0 ? T : S;
    const int q = tile * CG_BLOCK + t;
    const bool active = q < Q;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (active) {
        if (DIR == 0) {
            const size_t r = (size_t)(s0 + q) * 3;
            cg_warp(R, Tr, A.src + r, A.flow ? A.flow + r : nullptr, qx, qy, qz);
        } else {
            const float* p = A.tgt + (size_t)(t0 + q) * 3;
            qx = p[0]; qy = p[1]; qz = p[2];
        }
    }
    float best = INFINITY;
    int arg = 0;
    for (int k0 = 0; k0 < K; k0 += CG_STAGE) {
        const int nk = cg_stage_count(K, k0);
        for (int k = t; k < nk; k += CG_BLOCK) {
            float x, y, z;
            if (DIR == 0) {
                const float* p = A.tgt + (size_t)(t0 + k0 + k) * 3;
                x = p[0]; y = p[1]; z = p[2];
            } else {
                const size_t r = (size_t)(s0 + k0 + k) * 3;
                cg_warp(R, Tr, A.src + r, A.flow ? A.flow + r : nullptr, x, y, z);
            }
            s_ref[k] = make_float4(x, y, z, 0.f);
        }
        __syncthreads();
        if (active) {
            for (int k = 0; k < nk; ++k) {
                const float4 r = s_ref[k];
                const float d = cg_d2(r.x, r.y, r.z, qx, qy, qz);
                if (d < best) { best = d; arg = k0 + k; }       // equal distances keep the lower index
            }
        }
        __syncthreads();
    }
    if (!active) return;
    if (DIR == 0) {
        A.nn_st[s0 + q] = arg;
        A.d2_st[s0 + q] = best;
    } else {
        A.nn_ts[t0 + q] = arg;
    }
}

constexpr int CG_COMPACT = 256;

// one workgroup per pair walks its sources in ascending order and writes the kept ones densely from row s_off[pair]
__global__ __launch_bounds__(CG_COMPACT) void match_compact_kernel(MatchArgs A) {
    __shared__ int s_wave[CG_COMPACT / WAVE];
    const int pair = blockIdx.x, t = threadIdx.x;
    int s0, S, t0, T;
    const int st = cg_match_status(A, pair, s0, S, t0, T);
    if (st) {
        if (t == 0) {
            A.counts[pair] = 0;
            A.status[pair] = st;
        }
        return;
    }
    int base = 0;
    for (int c0 = 0; c0 < S; c0 += CG_COMPACT) {
        const int i = c0 + t;
        bool keep = false;
        int j = 0;
        if (i < S) {
            j = A.nn_st[s0 + i];
            keep = (unsigned)j < (unsigned)T && A.nn_ts[t0 + j] == i && sqrtf(A.d2_st[s0 + i]) < A.radius;
        }
        const unsigned long long b = __ballot(keep);
        if (lane_id() == 0) s_wave[wave_id()] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < CG_COMPACT / WAVE; ++w) {
            const int c = s_wave[w];
            before += w < wave_id() ? c : 0;
            total += c;
        }
        if (keep) {
            const int rank = base + before + __popcll(b & ((1ull << lane_id()) - 1ull));
            A.out_src[s0 + rank] = i;
            A.out_tgt[s0 + rank] = j;
        }
        base += total;
        __syncthreads();
    }
    if (t == 0) {
        A.counts[pair] = base;
        A.status[pair] = 0;
    }
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_blend_flow_knn3_f32(int P, int nq, int nr, const float* query, const int32_t* q_offsets, const float* reference,
                           const float* reference_flow, const int32_t* r_offsets, float* out_flow, int32_t* status, void* stream) {
    if (P < 0 || nq < 0 || nr < 0) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (!q_offsets || !r_offsets || !status || (nq > 0 && (!query || !out_flow)) || (nr > 0 && (!reference || !reference_flow)))
        return DR_EINVAL;
    const long long grid = cg_grid_bound(nq, P);
    if (grid > 0x7fffffffLL || (long long)nq * 3 > 0x7fffffffLL || (long long)nr * 3 > 0x7fffffffLL) return DR_ENOSUP;
    BlendArgs A = {P, nq, nr, query, q_offsets, reference, reference_flow, r_offsets, out_flow, status};
    hipLaunchKernelGGL(blend_flow_knn3_kernel, dim3((unsigned)grid), dim3(CG_BLOCK), 0, (hipStream_t)stream, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_coarse_gt_matches_workspace_bytes(int ns, int nt) { return cg_match_carve(ns, nt).bytes; }

int dr_coarse_gt_matches_f32(int P, int ns, int nt, const float* src, const int32_t* s_offsets, const float* tgt, const int32_t* t_offsets,
                             const float* src_flow, const float* rot, const float* trn, float radius, int64_t* out_src, int64_t* out_tgt,
                             int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || ns < 0 || nt < 0) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (!s_offsets || !t_offsets || !rot || !trn || !counts || !status || (ns > 0 && (!src || !out_src || !out_tgt)) || (nt > 0 && !tgt))
        return DR_EINVAL;
    const long long gs = cg_grid_bound(ns, P), gt = cg_grid_bound(nt, P);
    if (gs > 0x7fffffffLL || gt > 0x7fffffffLL || (long long)ns * 3 > 0x7fffffffLL || (long long)nt * 3 > 0x7fffffffLL) return DR_ENOSUP;
    const CgMatchCarve c = cg_match_carve(ns, nt);
    if (c.bytes > 0 && (!workspace || workspace_bytes < c.bytes)) return DR_EWORKSPACE;
    if (!aligned_to(workspace, 4)) return DR_EINVAL;
    char* w = (char*)workspace;
    MatchArgs A = {P, ns, nt, src, s_offsets, tgt, t_offsets, src_flow, rot, trn, radius,
                   (int*)(w + c.nn_st), (float*)(w + c.d2_st), (int*)(w + c.nn_ts),
                   (long long*)out_src, (long long*)out_tgt, counts, status};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(match_nn_kernel<0>, dim3((unsigned)gs), dim3(CG_BLOCK), 0, st, A);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_nn_kernel<1>, dim3((unsigned)gt), dim3(CG_BLOCK), 0, st, A);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(match_compact_kernel, dim3((unsigned)P), dim3(CG_COMPACT), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
