// eval2d3d.hip -- the evaluation metrics of the 2D-3D model on the device (ABI 0.7.0):
//   PIR (list form)           EvalFunction.evaluate_coarse_matching                 EXP/loss.py:247-264
//   PIR / recall / hit ratio  evaluate_sparse_correspondences                       vision3d/array_ops/registration_utils.py:202-225
//   IR (depth-masked)         EvalFunction.evaluate_fine_matching                   EXP/loss.py:266-278
//   IR / overlap / residual   evaluate_correspondences                              registration_utils.py:151-173, array_ops/metrics.py:144-166
//   RMSE, RRE, RTE, recall    registration_rmse, isotropic_registration_error       array_ops/metrics.py:25-74, 102-121
//                             EvalFunction.evaluate_registration                    EXP/loss.py:280-294
// EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.  The reference runs the first and third after every step on a dense
// float matrix and the others on the host per pair (numpy + a scipy KD-tree); here one pair per call is enqueued on the stream and nothing is
// read back.  Double arithmetic on the float32 inputs.  No float atomics: integer atomicOr on bitmaps and integer atomicAdd on counters (neither
// depends on the order of arrival); every sum of reals is a per-workgroup double partial (wave butterfly, then the waves in order) and the
// partials are added by one workgroup in one fixed order -- two runs are bit-identical.
#include "kernels.h"

namespace dr {

// bit 1 of the process-wide sticky word of dr_device_status (kernels.h: device_status_word): an entry skipped an index outside its range
constexpr unsigned STATUS_BAD_INDEX = 2u;

constexpr int EV_BLOCK = 256;
constexpr long long SPARSE_MAX_CELLS = 1ll << 26;     // img_num_nodes * round_up(pcd_num_nodes, 32)
constexpr int CORR_MAX = 16384;                       // correspondences that take part in dr_corr_eval_f32
constexpr int REG_MAX_BLOCKS = 256;

// sum over the workgroup (EV_BLOCK threads), valid in thread 0: butterfly inside a wave, then the waves in ascending order
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* s_w) {
    v = wave_sum(v);
    __syncthreads();                                   // s_w may still be read from the previous call
    if (lane_id() == 0) s_w[wave_id()] = v;
    __syncthreads();
    T r = s_w[0];
#pragma unroll
    for (int k = 1; k < EV_BLOCK / WAVE; ++k) r += s_w[k];
    return r;
}

// ------------------------------------------------------------------------------------------------------------
// sparse (node-level) correspondences: two bit matrices [img][ceil(pcd / 32)] in the workspace
// ------------------------------------------------------------------------------------------------------------
struct SparseWs {
    unsigned *gt, *pred;          // [img * W]
    unsigned *col_gt, *col_pos;   // [W]      bit c: some row holds a GT / a positive in column c
    unsigned *row_gt, *row_pos;   // [RW]     bit r: row r holds a GT / a positive
    int* cnt;                     // [4]      unique predictions, unique GT, unique positives, listed positives
    int W, RW;
    size_t words;                 // img * W
};
__host__ __device__ inline size_t sparse_ws_words(int img, int pcd) {
    const size_t W = ((size_t)pcd + 31) / 32, RW = ((size_t)img + 31) / 32;
    return 2 * (size_t)img * W + 2 * W + 2 * RW + 4;
}
static SparseWs sparse_ws(void* ws, int img, int pcd) {
    SparseWs s;
    s.W = (pcd + 31) / 32; s.RW = (img + 31) / 32; s.words = (size_t)img * s.W;
    unsigned* p = (unsigned*)ws;
    s.gt = p; p += s.words;
    s.pred = p; p += s.words;
    s.col_gt = p; p += s.W;
    s.col_pos = p; p += s.W;
    s.row_gt = p; p += s.RW;
    s.row_pos = p; p += s.RW;
    s.cnt = (int*)p;
    return s;
}

struct SparseArgs {
    int img, pcd, K, G;
    const long long *pi, *pp, *gi, *gp;
    const float* gov; float thr;
    SparseWs w;
    unsigned* status;
    double* out; int* counts;
};

// entries [0, G): ground truth (where its overlap passes), [G, G + K): predictions
__global__ __launch_bounds__(EV_BLOCK) void sparse_mark_kernel(SparseArgs A) {
    const long long e = (long long)blockIdx.x * EV_BLOCK + threadIdx.x;
    if (e >= (long long)A.G + A.K) return;
    const bool is_gt = e < A.G;
    const long long k = is_gt ? e : e - A.G;
    if (is_gt && A.gov && !(A.gov[k] > A.thr)) return;                  // torch.gt(gt_node_corr_min_overlaps, acceptance_overlap), loss.py:258
    const long long i = is_gt ? A.gi[k] : A.pi[k], j = is_gt ? A.gp[k] : A.pp[k];
    if ((unsigned long long)i >= (unsigned long long)A.img || (unsigned long long)j >= (unsigned long long)A.pcd) {
        atomicOr(A.status, STATUS_BAD_INDEX);
        return;
    }
    atomicOr((is_gt ? A.w.gt : A.w.pred) + (size_t)i * A.w.W + (size_t)(j >> 5), 1u << (j & 31));
}

// thread e < words: one word of both matrices; thread e < K: GT membership of listed prediction e (duplicates count each time)
__global__ __launch_bounds__(EV_BLOCK) void sparse_count_kernel(SparseArgs A) {
    __shared__ int s_w[EV_BLOCK / WAVE];
    const size_t e = (size_t)blockIdx.x * EV_BLOCK + threadIdx.x;
    int n_pred = 0, n_gt = 0, n_pos = 0, n_list = 0;
    if (e < A.w.words) {
        const unsigned g = A.w.gt[e], p = A.w.pred[e], b = g & p;
        n_pred = __popc(p); n_gt = __popc(g); n_pos = __popc(b);
        const size_t row = e / A.w.W, cw = e % A.w.W;
        if (g) { atomicOr(A.w.col_gt + cw, g); atomicOr(A.w.row_gt + (row >> 5), 1u << (row & 31)); }
        if (b) { atomicOr(A.w.col_pos + cw, b); atomicOr(A.w.row_pos + (row >> 5), 1u << (row & 31)); }
    }
    if (e < (size_t)A.K) {
        const long long i = A.pi[e], j = A.pp[e];
        if ((unsigned long long)i < (unsigned long long)A.img && (unsigned long long)j < (unsigned long long)A.pcd)
            n_list = (A.w.gt[(size_t)i * A.w.W + (size_t)(j >> 5)] >> (j & 31)) & 1u;
    }
    const int v[4] = {n_pred, n_gt, n_pos, n_list};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int s = block_sum(v[c], s_w);
        if (threadIdx.x == 0 && s) atomicAdd(A.w.cnt + c, s);
    }
}

__global__ __launch_bounds__(EV_BLOCK) void sparse_final_kernel(SparseArgs A) {
    __shared__ int s_w[EV_BLOCK / WAVE];
    int v[4] = {0, 0, 0, 0};                                            // columns with a GT / a positive, rows with a GT / a positive
    for (int c = threadIdx.x; c < A.w.W; c += EV_BLOCK) { v[0] += __popc(A.w.col_gt[c]); v[1] += __popc(A.w.col_pos[c]); }
    for (int r = threadIdx.x; r < A.w.RW; r += EV_BLOCK) { v[2] += __popc(A.w.row_gt[r]); v[3] += __popc(A.w.row_pos[r]); }
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = block_sum(v[c], s_w);
    if (threadIdx.x != 0) return;
    const int n_pred = A.w.cnt[0], n_gt = A.w.cnt[1], n_pos = A.w.cnt[2], n_list = A.w.cnt[3];
    A.out[0] = A.K > 0 ? (double)n_list / (double)A.K : (double)NAN;    // torch.mean of nothing
    A.out[1] = (double)n_pos / ((double)n_pred + 1e-12);
    A.out[2] = (double)n_pos / ((double)n_gt + 1e-12);
    const double src_hit = (double)v[3] / ((double)v[2] + 1e-12), tgt_hit = (double)v[1] / ((double)v[0] + 1e-12);
    A.out[3] = 0.5 * (src_hit + tgt_hit);
    A.counts[0] = n_pred; A.counts[1] = n_gt; A.counts[2] = n_pos; A.counts[3] = n_list;
}

// ------------------------------------------------------------------------------------------------------------
// fine correspondences
// ------------------------------------------------------------------------------------------------------------
struct CorrPartial { double resid; int inl, ovl, kept, kept_inl; };

struct CorrArgs {
    int n, m;
    const float *pcd, *img;
    const double* T;
    double radius;
    const long long* sel;
    int depth_mask;
    CorrPartial* part; int nblk;
    unsigned* status;
    double* out; int* counts;
};

__device__ __forceinline__ void apply_T(const double* __restrict__ T, double x, double y, double z, double& ox, double& oy, double& oz) {
    ox = T[0] * x + T[1] * y + T[2] * z + T[3];
    oy = T[4] * x + T[5] * y + T[6] * z + T[7];
    oz = T[8] * x + T[9] * y + T[10] * z + T[11];
}

// one image point per thread; the transformed cloud points of ALL selected correspondences pass through LDS in tiles of EV_BLOCK
// (point_cloud_overlap is knn(tgt = image points, src = transformed cloud points): every IMAGE point looks for its nearest CLOUD point)
__global__ __launch_bounds__(EV_BLOCK) void corr_eval_kernel(CorrArgs A) {
    __shared__ double s_q[EV_BLOCK * 3];
    __shared__ double s_wd[EV_BLOCK / WAVE];
    __shared__ int s_wi[EV_BLOCK / WAVE];
    __shared__ double s_T[12];
    const int t = threadIdx.x, e = blockIdx.x * EV_BLOCK + t;
    if (t < 12) s_T[t] = A.T[t];
    __syncthreads();
    bool have = false;
    double ix = 0, iy = 0, iz = 0, dist = 0;
    if (e < A.m) {
        const long long r = A.sel ? A.sel[e] : (long long)e;
        if ((unsigned long long)r < (unsigned long long)A.n) {
            have = true;
            ix = (double)A.img[r * 3]; iy = (double)A.img[r * 3 + 1]; iz = (double)A.img[r * 3 + 2];
            double qx, qy, qz;
            apply_T(s_T, (double)A.pcd[r * 3], (double)A.pcd[r * 3 + 1], (double)A.pcd[r * 3 + 2], qx, qy, qz);
            const double dx = ix - qx, dy = iy - qy, dz = iz - qz;
            dist = sqrt(dx * dx + dy * dy + dz * dz);
        } else {
            atomicOr(A.status, STATUS_BAD_INDEX);
        }
    }
    double best = INFINITY;
    for (int j0 = 0; j0 < A.m; j0 += EV_BLOCK) {
        const int nj = min(EV_BLOCK, A.m - j0);
        __syncthreads();
        if (t < nj) {
            const long long r = A.sel ? A.sel[j0 + t] : (long long)(j0 + t);
            double qx = INFINITY, qy = INFINITY, qz = INFINITY;         // a skipped selection is nobody's neighbour
            if ((unsigned long long)r < (unsigned long long)A.n)
                apply_T(s_T, (double)A.pcd[r * 3], (double)A.pcd[r * 3 + 1], (double)A.pcd[r * 3 + 2], qx, qy, qz);
            s_q[t * 3] = qx; s_q[t * 3 + 1] = qy; s_q[t * 3 + 2] = qz;
        }
        __syncthreads();
        if (have) {
            for (int j = 0; j < nj; ++j) {
                const double dx = ix - s_q[j * 3], dy = iy - s_q[j * 3 + 1], dz = iz - s_q[j * 3 + 2];
                const double d2 = dx * dx + dy * dy + dz * dz;
                best = d2 < best ? d2 : best;
            }
        }
    }
    const bool inl = have && dist < A.radius;
    // torch.gt(img_corr_points[..., -1], 0.0), loss.py:272; without the mask all m take part (a skipped selection stays in the denominator)
    const bool kept = A.depth_mask ? have && (float)iz > 0.0f : e < A.m;
    const double resid = block_sum(have ? dist : 0.0, s_wd);
    const int n_inl = block_sum(inl ? 1 : 0, s_wi);
    const int n_ovl = block_sum(have && sqrt(best) < A.radius ? 1 : 0, s_wi);
    const int n_kept = block_sum(kept ? 1 : 0, s_wi);
    const int n_kinl = block_sum(kept && inl ? 1 : 0, s_wi);
    if (t == 0) {
        CorrPartial p; p.resid = resid; p.inl = n_inl; p.ovl = n_ovl; p.kept = n_kept; p.kept_inl = n_kinl;
        A.part[blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(64) void corr_final_kernel(CorrArgs A) {
    if (threadIdx.x != 0) return;
    double resid = 0.0;
    int inl = 0, ovl = 0, kept = 0, kinl = 0;
    for (int b = 0; b < A.nblk; ++b) {                                   // at most CORR_MAX / EV_BLOCK = 64 partials, in block order
        const CorrPartial p = A.part[b];
        resid += p.resid; inl += p.inl; ovl += p.ovl; kept += p.kept; kinl += p.kept_inl;
    }
    const double m = (double)A.m;
    A.out[0] = A.m > 0 ? (double)inl / m : 0.0;                          // eval.py:156: no correspondences -> {0, 0, 0}
    A.out[1] = A.m > 0 ? resid / m : 0.0;
    A.out[2] = A.m > 0 ? (double)ovl / m : 0.0;
    A.out[3] = kept > 0 ? (double)kinl / (double)kept : 0.0;             // mean of nothing -> NaN -> nan_to_num_ -> 0, loss.py:277
    A.counts[0] = inl; A.counts[1] = ovl; A.counts[2] = kept; A.counts[3] = kinl;
}

// ------------------------------------------------------------------------------------------------------------
// registration
// ------------------------------------------------------------------------------------------------------------
struct RegArgs {
    int N;
    const float* pts;
    const double *Tg, *Te;
    double thr;
    double* part; int nblk;          // [nblk][2]: sum |T_gt p - T_est p|^2, sum |inv(T_gt) T_est p - p|
    double* out; int* recall;
};

// the upper 3 x 4 of inv(G) E for affine G, E (last rows 0 0 0 1): a true inverse of the 3 x 3 block (adjugate), as torch.linalg.inv
// inverts what it is given (loss.py:288)
__device__ __forceinline__ void realign_transform(const double* __restrict__ G, const double* __restrict__ E, double* __restrict__ Q) {
    const double a = G[0], b = G[1], c = G[2], d = G[4], e = G[5], f = G[6], g = G[8], h = G[9], i = G[10];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    const double I[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det,
                         (f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det,
                         (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) Q[r * 4 + k] = I[r * 3] * E[k] + I[r * 3 + 1] * E[4 + k] + I[r * 3 + 2] * E[8 + k];
        Q[r * 4 + 3] = I[r * 3] * (E[3] - G[3]) + I[r * 3 + 1] * (E[7] - G[7]) + I[r * 3 + 2] * (E[11] - G[11]);
    }
}

__global__ __launch_bounds__(EV_BLOCK) void reg_partial_kernel(RegArgs A) {
    __shared__ double s_w[EV_BLOCK / WAVE];
    __shared__ double s_G[12], s_E[12], s_Q[12];
    const int t = threadIdx.x;
    if (t < 12) { s_G[t] = A.Tg[t]; s_E[t] = A.Te[t]; }
    __syncthreads();
    if (t == 0) realign_transform(s_G, s_E, s_Q);
    __syncthreads();
    double sq = 0.0, nm = 0.0;
    for (long long p = (long long)blockIdx.x * EV_BLOCK + t; p < A.N; p += (long long)gridDim.x * EV_BLOCK) {
        const double x = (double)A.pts[p * 3], y = (double)A.pts[p * 3 + 1], z = (double)A.pts[p * 3 + 2];
        double gx, gy, gz, ex, ey, ez, qx, qy, qz;
        apply_T(s_G, x, y, z, gx, gy, gz);
        apply_T(s_E, x, y, z, ex, ey, ez);
        apply_T(s_Q, x, y, z, qx, qy, qz);
        const double dx = gx - ex, dy = gy - ey, dz = gz - ez;
        sq += dx * dx + dy * dy + dz * dz;
        const double rx = qx - x, ry = qy - y, rz = qz - z;
        nm += sqrt(rx * rx + ry * ry + rz * rz);
    }
    sq = block_sum(sq, s_w);
    nm = block_sum(nm, s_w);
    if (t == 0) { A.part[blockIdx.x * 2] = sq; A.part[blockIdx.x * 2 + 1] = nm; }
}

__global__ __launch_bounds__(EV_BLOCK) void reg_final_kernel(RegArgs A) {
    __shared__ double s_w[EV_BLOCK / WAVE];
    const int t = threadIdx.x;
    double sq = 0.0, nm = 0.0;
    if (t < A.nblk) { sq = A.part[t * 2]; nm = A.part[t * 2 + 1]; }      // nblk <= REG_MAX_BLOCKS = EV_BLOCK: one partial per thread
    sq = block_sum(sq, s_w);
    nm = block_sum(nm, s_w);
    if (t != 0) return;
    const double n = (double)A.N;
    const double rmse = A.N > 0 ? sqrt(sq / n) : (double)NAN;            // np.sqrt(np.sum(d ** 2, axis=1).mean()), array_ops/metrics.py:119
    const double realign = A.N > 0 ? nm / n : (double)NAN;               // torch.linalg.norm(., dim=1).mean(), loss.py:290
    const double *G = A.Tg, *E = A.Te;
    double trace = 0.0;                                                  // trace(R_est^T R_gt)
#pragma unroll
    for (int k = 0; k < 3; ++k) trace += E[k] * G[k] + E[4 + k] * G[4 + k] + E[8 + k] * G[8 + k];
    double x = 0.5 * (trace - 1.0);
    x = x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x);                           // np.clip(x, -1, 1) before arccos, array_ops/metrics.py:37-38
    const double tx = G[3] - E[3], ty = G[7] - E[7], tz = G[11] - E[11];
    A.out[0] = rmse;
    A.out[1] = realign;
    A.out[2] = 180.0 * acos(x) / 3.141592653589793;
    A.out[3] = sqrt(tx * tx + ty * ty + tz * tz);
    A.recall[0] = rmse < A.thr ? 1 : 0;                                  // a NaN compares false: no points, no recall
    A.recall[1] = realign < A.thr ? 1 : 0;
}

}  // namespace dr

// ------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------
using namespace dr;

extern "C" {

size_t dr_sparse_corr_eval_workspace_bytes(int img_num_nodes, int pcd_num_nodes) {
    if (img_num_nodes <= 0 || pcd_num_nodes <= 0) return 0;
    if ((long long)img_num_nodes * (((long long)pcd_num_nodes + 31) / 32 * 32) > SPARSE_MAX_CELLS) return 0;
    return sparse_ws_words(img_num_nodes, pcd_num_nodes) * sizeof(unsigned);
}

int dr_sparse_corr_eval_i64(int img_num_nodes, int pcd_num_nodes, int K, const int64_t* img_node_corr_indices,
                            const int64_t* pcd_node_corr_indices, int G, const int64_t* gt_img_node_corr_indices,
                            const int64_t* gt_pcd_node_corr_indices, const float* gt_node_corr_min_overlaps, float acceptance_overlap,
                            double* out, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (img_num_nodes <= 0 || pcd_num_nodes <= 0 || K < 0 || G < 0 || !out || !counts) return DR_EINVAL;
    if ((K > 0 && (!img_node_corr_indices || !pcd_node_corr_indices)) || (G > 0 && (!gt_img_node_corr_indices || !gt_pcd_node_corr_indices)))
        return DR_EINVAL;
    if ((long long)img_num_nodes * (((long long)pcd_num_nodes + 31) / 32 * 32) > SPARSE_MAX_CELLS) return DR_ENOSUP;
    const size_t need = dr_sparse_corr_eval_workspace_bytes(img_num_nodes, pcd_num_nodes);
    if (!workspace || workspace_bytes < need) return DR_EWORKSPACE;
    unsigned* status = device_status_word();
    if (!status) return DR_ELAUNCH;
    hipStream_t st = (hipStream_t)stream;
    SparseArgs A{};
    A.img = img_num_nodes; A.pcd = pcd_num_nodes; A.K = K; A.G = G;
    A.pi = (const long long*)img_node_corr_indices; A.pp = (const long long*)pcd_node_corr_indices;
    A.gi = (const long long*)gt_img_node_corr_indices; A.gp = (const long long*)gt_pcd_node_corr_indices;
    A.gov = gt_node_corr_min_overlaps; A.thr = acceptance_overlap;
    A.w = sparse_ws(workspace, img_num_nodes, pcd_num_nodes);
    A.status = status; A.out = out; A.counts = (int*)counts;
    DR_HIP_CHECK(hipMemsetAsync(workspace, 0, need, st));
    const long long marks = (long long)G + K;
    if (marks > 0) {
        hipLaunchKernelGGL(sparse_mark_kernel, dim3((unsigned)((marks + EV_BLOCK - 1) / EV_BLOCK)), dim3(EV_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    const size_t span = A.w.words > (size_t)K ? A.w.words : (size_t)K;
    hipLaunchKernelGGL(sparse_count_kernel, dim3((unsigned)((span + EV_BLOCK - 1) / EV_BLOCK)), dim3(EV_BLOCK), 0, st, A);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(sparse_final_kernel, dim3(1), dim3(EV_BLOCK), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_corr_eval_workspace_bytes(int m) {
    if (m <= 0 || m > CORR_MAX) return 0;
    return (size_t)((m + EV_BLOCK - 1) / EV_BLOCK) * sizeof(CorrPartial);
}

int dr_corr_eval_f32(int n, const float* pcd_corr_points, const float* img_corr_points, const double* transform, double positive_radius,
                     int n_sel, const int64_t* sel_indices, int depth_mask, double* out, int32_t* counts, void* workspace,
                     size_t workspace_bytes, void* stream) {
    if (n < 0 || n_sel < 0 || !transform || !out || !counts || (n > 0 && (!pcd_corr_points || !img_corr_points))) return DR_EINVAL;
    if (!sel_indices && n_sel != 0) return DR_EINVAL;
    const int m = sel_indices ? n_sel : n;
    if (m > CORR_MAX) return DR_ENOSUP;
    const size_t need = dr_corr_eval_workspace_bytes(m);
    if (m > 0 && (!workspace || workspace_bytes < need)) return DR_EWORKSPACE;
    unsigned* status = device_status_word();
    if (!status) return DR_ELAUNCH;
    hipStream_t st = (hipStream_t)stream;
    CorrArgs A{};
    A.n = n; A.m = m; A.pcd = pcd_corr_points; A.img = img_corr_points; A.T = transform; A.radius = positive_radius;
    A.sel = (const long long*)sel_indices; A.depth_mask = depth_mask != 0;
    A.part = (CorrPartial*)workspace; A.nblk = (m + EV_BLOCK - 1) / EV_BLOCK;
    A.status = status; A.out = out; A.counts = (int*)counts;
    if (m > 0) {
        hipLaunchKernelGGL(corr_eval_kernel, dim3(A.nblk), dim3(EV_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(corr_final_kernel, dim3(1), dim3(64), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

static int reg_blocks(int N) {
    const int b = (N + EV_BLOCK - 1) / EV_BLOCK;
    return b > REG_MAX_BLOCKS ? REG_MAX_BLOCKS : b;
}

size_t dr_registration_eval_workspace_bytes(int N) {
    if (N <= 0) return 0;
    return (size_t)reg_blocks(N) * 2 * sizeof(double);
}

int dr_registration_eval_f64(int N, const float* pcd_points, const double* gt_transform, const double* est_transform, double rmse_threshold,
                             double* out, int32_t* recall, void* workspace, size_t workspace_bytes, void* stream) {
    if (N < 0 || !gt_transform || !est_transform || !out || !recall || (N > 0 && !pcd_points)) return DR_EINVAL;
    if (N > 0 && (!workspace || workspace_bytes < dr_registration_eval_workspace_bytes(N))) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    RegArgs A{};
    A.N = N; A.pts = pcd_points; A.Tg = gt_transform; A.Te = est_transform; A.thr = rmse_threshold;
    A.part = (double*)workspace; A.nblk = N > 0 ? reg_blocks(N) : 0;
    A.out = out; A.recall = (int*)recall;
    if (N > 0) {
        hipLaunchKernelGGL(reg_partial_kernel, dim3(A.nblk), dim3(EV_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(reg_final_kernel, dim3(1), dim3(EV_BLOCK), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
