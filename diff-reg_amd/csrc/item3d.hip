// item3d.hip -- the 3D / 4D dataset item on the device (fifteenth set after ABI 0.7.0): what _3DMatch.__getitem__ and
// _4DMatch.__getitem__ compute behind their file reads, for all pairs of a batch in one call each:
//   dr_item3d_prepare_f32        subsample, rotate one side, jitter, recompute s2t_flow, compose rot / trans
//                                3D/datasets/_3dmatch.py:70-106, 126-133; 3D/datasets/_4dmatch.py:77, 85-124, 135-142
//   dr_radius_pairs_ragged_f32   get_correspondences / KDTree_corr                         3D/lib/benchmark_utils.py:166-185
// Both are ragged over P pairs (offset arrays of P + 1 int32 entries on the device), asynchronous on the given stream, and read nothing back
// to the host.  The only atomics are integer ORs into the status words: two runs are bit-equal.
//
// Every index below comes from item3d_index.h (walked on the host by tools/item3d_index_check.cpp).
//
// The pair list: the targets of all pairs are sorted by (pair, cell) with cells of edge radius (1 + 2^-7), as build_ball_index (collate.hip)
// sorts its supports; one wave per source row then sweeps the 27 cells about the row as nine runs of the sorted list, each found by two binary
// searches (the lanes 0..17 of the wave search at the same time).  Three launches share that sweep: count, scan (one workgroup per pair), write.
// The sweep meets a row's partners in cell order; the write pass ranks every partner by the number of the row's partners with a lower target
// index, counted by a second sweep in which all lanes read the same candidate (a broadcast load), so the list comes out in ascending (i, j)
// whatever the schedule and however many partners a row has.
#include "common.h"
#include "item3d_index.h"
#include "kernels.h"
#include "../../include/diffreg_hip.h"

namespace dr {
namespace {

// ------------------------------------------------------------------------------------------------------------
// prepare
// ------------------------------------------------------------------------------------------------------------
struct SideArgs {
    const float* raw; const int* raw_off; int n_raw;
    const long long* sel; const int* off; int n;
    const double* jitter; float* out;
};

struct PrepArgs {
    int P;
    SideArgs side[2];                     // 0: source, 1: target
    const float* flow_raw; float* flow_out; int recompute_flow;
    const double* rot_ab; const double* coin; double noise;
    const double* rot; const double* trans;
    float* rot_out; float* trans_out; float* tsfm_out;
    int* status;
};

// R x of np.matmul(rot_ab, cloud.T).T in float64, one row
__device__ __forceinline__ void rot3(const double* __restrict__ R, double x, double y, double z, double* o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = (R[3 * k] * x + R[3 * k + 1] * y) + R[3 * k + 2] * z;
}

// blockIdx.y = side; one output row per thread
__global__ __launch_bounds__(IT3_BLOCK) void item3d_rows_kernel(PrepArgs A) {
    const int s = blockIdx.y;
    const SideArgs& S = A.side[s];
    const int row = blockIdx.x * IT3_BLOCK + threadIdx.x;
    if (row >= S.n) return;
    const int p = it3_pair_of(A.P, S.off, S.n, row);
    float* o = S.out + (size_t)row * 3;
    // a row of no pair, or of a pair whose raw slice is unusable, is written as zero (the pair's status bit is set by item3d_pose_kernel)
    const int raw_lo = p < A.P ? S.raw_off[p] : 0, raw_hi = p < A.P ? S.raw_off[p + 1] : -1;
    if (p >= A.P || !it3_slice_ok(raw_lo, raw_hi, S.n_raw)) {
        o[0] = o[1] = o[2] = 0.f;
        return;
    }
    const int raw_n = raw_hi - raw_lo, local = row - S.off[p];
    const long long r = S.sel ? S.sel[row] : (long long)local;
    if (!it3_sel_ok(r, raw_n)) {
        atomicOr(A.status + p, IT3_ST_SELECT);
        o[0] = o[1] = o[2] = 0.f;
        return;
    }
    const float* x = S.raw + ((size_t)raw_lo + (size_t)r) * 3;
    const bool turn_src = A.rot_ab && A.coin[p] > 0.5;                      // _3dmatch.py:97
    const bool turned = A.rot_ab && (turn_src == (s == 0));
    const double* R = A.rot_ab ? A.rot_ab + (size_t)p * 9 : nullptr;
    const bool f64 = turned || S.jitter;
    double v[3] = {(double)x[0], (double)x[1], (double)x[2]};
    if (turned) rot3(R, (double)x[0], (double)x[1], (double)x[2], v);
    if (S.jitter) {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] + (S.jitter[(size_t)row * 3 + k] - 0.5) * A.noise;       // _3dmatch.py:105-106
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = f64 ? (float)v[k] : x[k];
    if (s != 0 || !A.flow_raw || !A.recompute_flow) return;
    // _4dmatch.py:77, 115, 124: the deformed copy is built BEFORE the subsample and never indexed by it, so its row is `local`, not r
    if (local >= raw_n) { atomicOr(A.status + p, IT3_ST_FLOW); return; }
    const float* xs = A.side[0].raw + ((size_t)raw_lo + (size_t)local) * 3;
    const float* fl = A.flow_raw + ((size_t)raw_lo + (size_t)local) * 3;
    float* fo = A.flow_out + ((size_t)raw_lo + (size_t)local) * 3;
    float d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = xs[k] + fl[k];                       // float32 + float32, as numpy adds the loaded arrays
    double dd[3] = {(double)d[0], (double)d[1], (double)d[2]};
    if (turned) rot3(R, (double)d[0], (double)d[1], (double)d[2], dd);
    // a turned source stays float64 until the collate; an unturned one was jittered in place in float32
#pragma unroll
    for (int k = 0; k < 3; ++k) fo[k] = (float)(dd[k] - (turned ? v[k] : (double)o[k]));
}

// one thread per pair: the composed rot / trans (_3dmatch.py:97-103) and the 3 x 4 transform the pair list reads
__global__ __launch_bounds__(IT3_BLOCK) void item3d_pose_kernel(PrepArgs A) {
    const int p = blockIdx.x * IT3_BLOCK + threadIdx.x;
    if (p >= A.P) return;
    int st = 0;
    for (int s = 0; s < 2; ++s) {
        const SideArgs& S = A.side[s];
        if (!it3_slice_ok(S.off[p], S.off[p + 1], S.n) || !it3_slice_ok(S.raw_off[p], S.raw_off[p + 1], S.n_raw)) st |= IT3_ST_OFFSETS;
    }
    if (st) atomicOr(A.status + p, st);
    const double* R0 = A.rot + (size_t)p * 9;
    const double* t0 = A.trans + (size_t)p * 3;
    double R[9], t[3] = {t0[0], t0[1], t0[2]};
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = R0[k];
    if (A.rot_ab) {
        const double* Q = A.rot_ab + (size_t)p * 9;
        double N[9];
        if (A.coin[p] > 0.5) {                                              // rot = rot rot_ab^T
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) N[3 * i + j] = (R[3 * i] * Q[3 * j] + R[3 * i + 1] * Q[3 * j + 1]) + R[3 * i + 2] * Q[3 * j + 2];
        } else {                                                            // rot = rot_ab rot, trans = rot_ab trans
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) N[3 * i + j] = (Q[3 * i] * R[j] + Q[3 * i + 1] * R[3 + j]) + Q[3 * i + 2] * R[6 + j];
            double nt[3];
            rot3(Q, t[0], t[1], t[2], nt);
            t[0] = nt[0]; t[1] = nt[1]; t[2] = nt[2];
        }
        for (int k = 0; k < 9; ++k) R[k] = N[k];
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            A.rot_out[(size_t)p * 9 + 3 * i + j] = (float)R[3 * i + j];
            A.tsfm_out[(size_t)p * 12 + 4 * i + j] = (float)R[3 * i + j];
        }
        A.trans_out[(size_t)p * 3 + i] = (float)t[i];
        A.tsfm_out[(size_t)p * 12 + 4 * i + 3] = (float)t[i];
    }
}

// ------------------------------------------------------------------------------------------------------------
// ragged radius pairs
// ------------------------------------------------------------------------------------------------------------
struct PairsArgs {
    int P, ns, nt, n_pad;
    const float* src; const int* s_off;
    const float* tgt; const int* t_off;
    const float* transforms;
    float cell, r2;
    float* moved; long long* row_start; float4* origin;
    unsigned long long* keys; unsigned* vals; float4* sorted;
    const long long* c_off; long long capacity;
    long long* out_src; long long* out_tgt; int* counts; int* status;
};

// the float32 expressions of dr_radius_pairs_f32 (partition2d3d.hip: move_points_kernel, RadiusPred)
__device__ __forceinline__ float rp_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return dx * dx + dy * dy + dz * dz;
}

__global__ __launch_bounds__(IT3_BLOCK) void rp_move_kernel(PairsArgs A) {
    const int i = blockIdx.x * IT3_BLOCK + threadIdx.x;
    if (i >= A.ns) return;
    const int p = it3_pair_of(A.P, A.s_off, A.ns, i);
    const float x = A.src[3 * (size_t)i], y = A.src[3 * (size_t)i + 1], z = A.src[3 * (size_t)i + 2];
    const float* T = (A.transforms && p < A.P) ? A.transforms + (size_t)p * 12 : nullptr;
    A.moved[3 * (size_t)i] = T ? x * T[0] + y * T[1] + z * T[2] + T[3] : x;
    A.moved[3 * (size_t)i + 1] = T ? x * T[4] + y * T[5] + z * T[6] + T[7] : y;
    A.moved[3 * (size_t)i + 2] = T ? x * T[8] + y * T[9] + z * T[10] + T[11] : z;
}

// one workgroup per pair: the min corner of its targets (fminf skips NaN; an empty pair keeps +inf, which nothing reads)
__global__ __launch_bounds__(IT3_BLOCK) void rp_origin_kernel(PairsArgs A) {
    __shared__ float s_mn[IT3_BLOCK / WAVE][3];
    const int p = blockIdx.x, t = threadIdx.x;
    const int lo = A.t_off[p], hi = A.t_off[p + 1];
    float mn[3] = {INFINITY, INFINITY, INFINITY};
    if (it3_slice_ok(lo, hi, A.nt)) {
        for (int i = lo + t; i < hi; i += IT3_BLOCK) {
#pragma unroll
            for (int c = 0; c < 3; ++c) mn[c] = fminf(mn[c], A.tgt[(size_t)i * 3 + c]);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) mn[c] = wave_min(mn[c]);
    if (lane_id() == 0)
        for (int c = 0; c < 3; ++c) s_mn[wave_id()][c] = mn[c];
    __syncthreads();
    if (t != 0) return;
    for (int w = 1; w < IT3_BLOCK / WAVE; ++w)
        for (int c = 0; c < 3; ++c) mn[c] = fminf(mn[c], s_mn[w][c]);
    A.origin[p] = make_float4(mn[0], mn[1], mn[2], 0.f);
}

// (key, stacked target row) of every target; rows >= nt and rows of no pair sort behind every pair's rows
__global__ __launch_bounds__(IT3_BLOCK) void rp_key_kernel(PairsArgs A) {
    const int i = blockIdx.x * IT3_BLOCK + threadIdx.x;
    if (i >= A.n_pad) return;
    A.vals[i] = (unsigned)i;
    if (i >= A.nt) { A.keys[i] = IT3_PAD_KEY; return; }
    const int p = it3_pair_of(A.P, A.t_off, A.nt, i);
    if (p >= A.P) { A.keys[i] = it3_key(A.P, 0, 0, 0); return; }
    const float4 o = A.origin[p];
    A.keys[i] = it3_key(p, it3_cell(A.tgt[(size_t)i * 3], o.x, A.cell), it3_cell(A.tgt[(size_t)i * 3 + 1], o.y, A.cell),
                        it3_cell(A.tgt[(size_t)i * 3 + 2], o.z, A.cell));
}

// the targets in key order, w = the stacked target row
__global__ __launch_bounds__(IT3_BLOCK) void rp_gather_kernel(PairsArgs A) {
    const int i = blockIdx.x * IT3_BLOCK + threadIdx.x;
    if (i >= A.nt) return;
    const unsigned v = A.vals[i];                       // < nt: the nt real keys sort in front of the padding
    A.sorted[i] = make_float4(A.tgt[(size_t)v * 3], A.tgt[(size_t)v * 3 + 1], A.tgt[(size_t)v * 3 + 2], __uint_as_float(v));
}

// what one wave knows about its source row
struct RowCtx {
    int pair, local, t0, t1;          // pair < 0: nothing to do
    float qx, qy, qz;
    int lo, hi;                       // lane r < 9: run r of the sorted list
};

__device__ __forceinline__ RowCtx rp_row(const PairsArgs& A, int i, int lane) {
    RowCtx C;
    C.pair = -1; C.local = 0; C.t0 = C.t1 = 0; C.lo = C.hi = 0;
    C.qx = C.qy = C.qz = 0.f;
    if (i >= A.ns) return C;
    const int p = it3_pair_of(A.P, A.s_off, A.ns, i);
    if (p >= A.P) return C;
    const int t0 = A.t_off[p], t1 = A.t_off[p + 1];
    if (!it3_slice_ok(t0, t1, A.nt)) return C;
    C.pair = p; C.local = i - A.s_off[p]; C.t0 = t0; C.t1 = t1;
    C.qx = A.moved[3 * (size_t)i]; C.qy = A.moved[3 * (size_t)i + 1]; C.qz = A.moved[3 * (size_t)i + 2];
    if (t1 <= t0) return C;
    const float4 o = A.origin[p];
    const int cx = it3_cell(C.qx, o.x, A.cell), cy = it3_cell(C.qy, o.y, A.cell), cz = it3_cell(C.qz, o.z, A.cell);
    // lanes 0..8 find the start of run `lane`, lanes 9..17 the end of run `lane - 9`: 18 binary searches side by side
    const int r = lane < 9 ? lane : lane - 9;
    unsigned long long first = 0, last = 0;
    int pos = 0;
    if (lane < 18 && it3_run_keys(p, cx, cy, cz, r, first, last))
        // over ALL sorted targets: the pair sits in the key's high bits, and rows of no pair in front of t_off[0] sort behind every pair, so a
        // pair's targets need not lie at sorted positions [t0, t1)
        pos = lane < 9 ? it3_lower_bound(A.keys, 0, A.nt, first) : it3_lower_bound(A.keys, 0, A.nt, last + 1);
    const int end = __shfl(pos, lane + 9 < 64 ? lane + 9 : lane);
    if (lane < 9) { C.lo = pos; C.hi = end > pos ? end : pos; }
    return C;
}

// the row's partners: body(hit, stacked target row) once per 64 candidates, with every lane of the wave taking part
template <class Body>
__device__ __forceinline__ void rp_sweep(const PairsArgs& A, const RowCtx& C, int lane, Body&& body) {
    for (int r = 0; r < 9; ++r) {
        const int lo = __shfl(C.lo, r), hi = __shfl(C.hi, r);
        for (int base = lo; base < hi; base += WAVE) {
            const int j = base + lane;
            bool hit = false;
            unsigned id = 0;
            if (j < hi) {
                const float4 s = A.sorted[j];
                hit = rp_d2(C.qx, C.qy, C.qz, s.x, s.y, s.z) < A.r2;
                id = __float_as_uint(s.w);
            }
            body(hit, id);
        }
    }
}

__global__ __launch_bounds__(IT3_ROWS * WAVE) void rp_count_kernel(PairsArgs A) {
    const int i = blockIdx.x * IT3_ROWS + wave_id(), lane = lane_id();
    if (i >= A.ns) return;
    const RowCtx C = rp_row(A, i, lane);
    long long n = 0;
    if (C.pair >= 0) rp_sweep(A, C, lane, [&](bool hit, unsigned) { n += __popcll(__ballot(hit)); });
    if (lane == 0) A.row_start[i] = n;
}

// one workgroup per pair: exclusive scan of its rows' counts in place (the ranks are pair-local), the pair's counts and status
__global__ __launch_bounds__(1024) void rp_scan_kernel(PairsArgs A) {
    __shared__ long long s_w[16];
    __shared__ long long s_base;
    const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int s0 = A.s_off[p], s1 = A.s_off[p + 1];
    const bool ok = it3_slice_ok(s0, s1, A.ns) && it3_slice_ok(A.t_off[p], A.t_off[p + 1], A.nt);
    const int rows = ok ? s1 - s0 : 0;
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < rows; i0 += 1024) {
        const int i = i0 + t;
        const long long v = i < rows ? A.row_start[s0 + i] : 0;
        long long inc = v;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const long long o = __shfl_up(inc, m);
            if (lane >= m) inc += o;
        }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        long long before = s_base;
        for (int q = 0; q < w; ++q) before += s_w[q];
        if (i < rows) A.row_start[s0 + i] = before + inc - v;
        __syncthreads();
        if (t == 0) { long long tot = 0; for (int q = 0; q < 16; ++q) tot += s_w[q]; s_base += tot; }
        __syncthreads();
    }
    if (t == 0) {
        const long long room = A.c_off ? it3_room(A.c_off[p], A.c_off[p + 1], A.capacity) : 0;
        A.counts[2 * p] = it3_saturate(s_base < room ? s_base : room);
        A.counts[2 * p + 1] = it3_saturate(s_base);
        A.status[p] = ok ? 0 : IT3_ST_OFFSETS;
    }
}

__global__ __launch_bounds__(IT3_ROWS * WAVE) void rp_write_kernel(PairsArgs A) {
    const int i = blockIdx.x * IT3_ROWS + wave_id(), lane = lane_id();
    if (i >= A.ns) return;
    const RowCtx C = rp_row(A, i, lane);
    if (C.pair < 0) return;
    const long long base = A.c_off[C.pair], room = it3_room(base, A.c_off[C.pair + 1], A.capacity);
    const long long start = A.row_start[i];
    if (start >= room) return;                                              // every entry of this row lies behind the pair's room
    rp_sweep(A, C, lane, [&](bool hit, unsigned id) {
        if (!__ballot(hit)) return;
        // rank of this lane's partner among the row's partners by target row: all lanes walk the same candidates (broadcast loads)
        int rank = 0;
        for (int r = 0; r < 9; ++r) {
            const int lo = __shfl(C.lo, r), hi = __shfl(C.hi, r);
            for (int c = lo; c < hi; ++c) {
                const float4 s = A.sorted[c];
                rank += (rp_d2(C.qx, C.qy, C.qz, s.x, s.y, s.z) < A.r2 && __float_as_uint(s.w) < id) ? 1 : 0;
            }
        }
        const long long pos = start + rank;
        if (hit && pos < room) {
            A.out_src[base + pos] = C.local;
            A.out_tgt[base + pos] = (long long)id - C.t0;
        }
    });
}

}  // namespace

// the targets of all pairs sorted by (pair, cell): origin -> keys -> sort -> the targets in key order.  The grid of dr_radius_pairs_ragged_f32,
// shared with the point-to-point ICP (icp.hip), whose targets never move (kernels.h)
int launch_target_grid(int P, int nt, const float* tgt, const int* t_off, float cell, float4* origin, unsigned long long* keys, unsigned* vals,
                       float4* sorted, hipStream_t st) {
    if (nt <= 0) return DR_OK;
    PairsArgs A = {};
    A.P = P; A.nt = nt; A.n_pad = next_pow2(nt);
    A.tgt = tgt; A.t_off = t_off; A.cell = cell;
    A.origin = origin; A.keys = keys; A.vals = vals; A.sorted = sorted;
    hipLaunchKernelGGL(rp_origin_kernel, dim3(P), dim3(IT3_BLOCK), 0, st, A);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(rp_key_kernel, dim3(it3_blocks(A.n_pad, IT3_BLOCK)), dim3(IT3_BLOCK), 0, st, A);
    DR_LAUNCH_CHECK();
    const int rc = launch_bitonic_sort(A.keys, A.vals, A.n_pad, st);
    if (rc != DR_OK) return rc;
    hipLaunchKernelGGL(rp_gather_kernel, dim3(it3_blocks(nt, IT3_BLOCK)), dim3(IT3_BLOCK), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_item3d_prepare_f32(const dr_item3d_args* a, void* stream) {
    if (!a || a->P < 0 || a->n_src_raw < 0 || a->n_tgt_raw < 0 || a->n_src < 0 || a->n_tgt < 0) return DR_EINVAL;
    if (a->P == 0) return DR_OK;
    if (a->P > IT3_MAX_PAIRS || a->n_src_raw > IT3_MAX_ROWS || a->n_tgt_raw > IT3_MAX_ROWS || a->n_src > IT3_MAX_ROWS || a->n_tgt > IT3_MAX_ROWS)
        return DR_ENOSUP;
    if (!a->s_raw_offsets || !a->t_raw_offsets || !a->s_offsets || !a->t_offsets || !a->rot || !a->trans || !a->rot_out || !a->trans_out ||
        !a->tsfm_out || !a->status || (a->n_src_raw > 0 && !a->src_raw) || (a->n_tgt_raw > 0 && !a->tgt_raw) || (a->n_src > 0 && !a->src_out) ||
        (a->n_tgt > 0 && !a->tgt_out) || (a->rot_ab && !a->coin) || (a->flow_raw && a->n_src_raw > 0 && !a->flow_out))
        return DR_EINVAL;
    // without a selection a side's rows are its raw rows
    if ((!a->src_sel && a->n_src != a->n_src_raw) || (!a->tgt_sel && a->n_tgt != a->n_tgt_raw)) return DR_EINVAL;
    // _4dmatch.py:124 `src_pcd_deformed - src_pcd`: the deformed copy keeps the raw row count, so a shorter selection has no flow to recompute
    if (a->flow_raw && a->recompute_flow && a->n_src != a->n_src_raw) return DR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    PrepArgs A;
    A.P = a->P;
    A.side[0] = {a->src_raw, a->s_raw_offsets, a->n_src_raw, (const long long*)a->src_sel, a->s_offsets, a->n_src, a->src_jitter, a->src_out};
    A.side[1] = {a->tgt_raw, a->t_raw_offsets, a->n_tgt_raw, (const long long*)a->tgt_sel, a->t_offsets, a->n_tgt, a->tgt_jitter, a->tgt_out};
    A.flow_raw = a->flow_raw; A.flow_out = a->flow_out; A.recompute_flow = a->recompute_flow;
    A.rot_ab = a->rot_ab; A.coin = a->coin; A.noise = a->noise;
    A.rot = a->rot; A.trans = a->trans; A.rot_out = a->rot_out; A.trans_out = a->trans_out; A.tsfm_out = a->tsfm_out;
    A.status = a->status;
    DR_HIP_CHECK(hipMemsetAsync(a->status, 0, sizeof(int32_t) * (size_t)a->P, st));
    if (a->flow_raw && !a->recompute_flow && a->n_src_raw > 0)               // the flow comes back as loaded: unselected (the header's note)
        DR_HIP_CHECK(hipMemcpyAsync(a->flow_out, a->flow_raw, sizeof(float) * 3 * (size_t)a->n_src_raw, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(item3d_pose_kernel, dim3(it3_blocks(a->P, IT3_BLOCK)), dim3(IT3_BLOCK), 0, st, A);
    DR_LAUNCH_CHECK();
    const int rows = a->n_src > a->n_tgt ? a->n_src : a->n_tgt;
    if (rows > 0) {
        hipLaunchKernelGGL(item3d_rows_kernel, dim3(it3_blocks(rows, IT3_BLOCK), 2), dim3(IT3_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

size_t dr_radius_pairs_ragged_workspace_bytes(int P, int ns, int nt) { return it3_pairs_carve(P, ns, nt).bytes; }

int dr_radius_pairs_ragged_f32(int P, int ns, int nt, const float* src, const int32_t* s_offsets, const float* tgt, const int32_t* t_offsets,
                               const float* transforms, float radius, const int64_t* c_offsets, long long capacity, int64_t* out_src,
                               int64_t* out_tgt, int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0 || ns < 0 || nt < 0 || capacity < 0 || !(radius > 0.f)) return DR_EINVAL;
    if (P == 0) return DR_OK;
    if (P > IT3_MAX_PAIRS || ns > IT3_MAX_ROWS || nt > IT3_MAX_ROWS) return DR_ENOSUP;
    if (!s_offsets || !t_offsets || !counts || !status || (ns > 0 && !src) || (nt > 0 && !tgt) ||
        (capacity > 0 && (!c_offsets || !out_src || !out_tgt)))
        return DR_EINVAL;
    const It3PairsCarve c = it3_pairs_carve(P, ns, nt);
    if (!workspace || workspace_bytes < c.bytes) return DR_EWORKSPACE;
    if (!aligned_to(workspace, 16)) return DR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)workspace;
    PairsArgs A;
    A.P = P; A.ns = ns; A.nt = nt; A.n_pad = nt > 0 ? next_pow2(nt) : 0;
    A.src = src; A.s_off = s_offsets; A.tgt = tgt; A.t_off = t_offsets; A.transforms = transforms;
    A.cell = radius * (1.0f + 1.0f / 128.0f); A.r2 = radius * radius;
    A.moved = (float*)(w + c.moved); A.row_start = (long long*)(w + c.row_start); A.origin = (float4*)(w + c.origin);
    A.keys = (unsigned long long*)(w + c.keys); A.vals = (unsigned*)(w + c.vals); A.sorted = (float4*)(w + c.sorted);
    A.c_off = capacity > 0 ? (const long long*)c_offsets : nullptr; A.capacity = capacity;
    A.out_src = (long long*)out_src; A.out_tgt = (long long*)out_tgt; A.counts = counts; A.status = status;
    if (ns > 0) {
        hipLaunchKernelGGL(rp_move_kernel, dim3(it3_blocks(ns, IT3_BLOCK)), dim3(IT3_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    const int grc = launch_target_grid(P, nt, tgt, t_offsets, A.cell, A.origin, A.keys, A.vals, A.sorted, st);
    if (grc != DR_OK) return grc;
    if (ns > 0) {
        hipLaunchKernelGGL(rp_count_kernel, dim3(it3_blocks(ns, IT3_ROWS)), dim3(IT3_ROWS * WAVE), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(rp_scan_kernel, dim3(P), dim3(1024), 0, st, A);
    DR_LAUNCH_CHECK();
    if (ns > 0 && A.c_off) {
        hipLaunchKernelGGL(rp_write_kernel, dim3(it3_blocks(ns, IT3_ROWS)), dim3(IT3_ROWS * WAVE), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

}  // extern "C"
