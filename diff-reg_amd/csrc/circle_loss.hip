// circle_loss.hip -- the non-GEMM parts of the 2D-3D coarse loss (Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1/loss.py:30-75):
// the row L2 normalisation in front of it (F.normalize, EXP/model.py:552-553) and the weighted circle loss (vision3d/loss/circle_loss.py:11-52)
// on feat_dists = sqrt(clamp(2 - 2 img pcd^T, 0) + 1e-8) (vision3d/ops/pairwise_distance.py:38-56), forward and backward.
//   img [M, C] (anchor rows), pcd [N, C] (columns), both normalised; the similarity img pcd^T on launch_gemm.
//   The overlap lists scatter to dense [M, N] matrices; one element-wise pass builds the positive / negative logits (their weights are constants
//   of the graph, as the reference detaches them); row and column log-sum-exps in double, each in one fixed order; one workgroup forms the
//   anchor-masked means (an empty anchor set: 0 / 0 = NaN, as torch's mean of an empty selection) and the per-row / per-column coefficients of
//   the gradient; the backward's element-wise pass writes d loss / d sim AND its transpose (zero-padded for the GEMM's k extent), and two GEMMs
//   carry it to the features.  No atomics.
#include "train_common.h"

namespace dr {
namespace {

struct CircleArgs {
    float pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale, pos_overlap, neg_overlap;
};

__global__ __launch_bounds__(256) void overlap_scatter_kernel(int K, int M, int N, const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
                                                              const float* __restrict__ omin, const float* __restrict__ omax, float* __restrict__ Omin,
                                                              float* __restrict__ Omax) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int64_t i = ii[k], j = jj[k];
    if (i < 0 || i >= M || j < 0 || j >= N) return;          // (the reference raises on an index outside the matrix)
    Omin[i * N + j] = omin[k];
    Omax[i * N + j] = omax[k];
}

// the reference's float32 arithmetic of feat_dists and both weights, in its operation order
struct Elem { float D, pw, nw; bool pos, neg, pass; };
__device__ __forceinline__ Elem circle_elem(float s, float omin, float omax, const CircleArgs& a) {
    Elem e;
    const float t = 2.0f - 2.0f * s;
    e.pass = t >= 0.f;                                        // clamp(min = 0) lets the gradient through where t >= 0
    e.D = sqrtf(fmaxf(t, 0.f) + 1e-8f);
    e.pos = omin > a.pos_overlap;
    e.neg = omax < a.neg_overlap;
    const float sc = sqrtf(omin * (e.pos ? 1.f : 0.f));
    e.pw = fmaxf(0.f, (e.D - (e.pos ? 0.f : 1e5f)) - a.pos_optimal) * sc;
    e.nw = fmaxf(0.f, a.neg_optimal - (e.D + (e.neg ? 0.f : 1e5f)));
    return e;
}

__global__ __launch_bounds__(256) void circle_logits_kernel(long long MN, const float* __restrict__ S, const float* __restrict__ Omin,
                                                            const float* __restrict__ Omax, CircleArgs a, float* __restrict__ A, float* __restrict__ Bn,
                                                            uint8_t* __restrict__ flags) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= MN) return;
    const Elem el = circle_elem(S[e], Omin[e], Omax[e], a);
    A[e] = a.log_scale * (el.D - a.pos_margin) * el.pw;
    Bn[e] = a.log_scale * (a.neg_margin - el.D) * el.nw;
    flags[e] = (el.pos ? 1 : 0) | (el.neg ? 2 : 0);
}

// row i: log-sum-exp of A and Bn over the N columns (double), and whether the row holds a positive and a negative.  One wave per row.
__global__ __launch_bounds__(256) void circle_rows_kernel(int M, int N, const float* __restrict__ A, const float* __restrict__ Bn,
                                                          const uint8_t* __restrict__ flags, double* __restrict__ la, double* __restrict__ lb,
                                                          int* __restrict__ rm) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= M) return;
    const size_t o = (size_t)i * N;
    float ma = -INFINITY, mb = -INFINITY;
    int f = 0;
    for (int j = lane; j < N; j += 64) { ma = fmaxf(ma, A[o + j]); mb = fmaxf(mb, Bn[o + j]); f |= flags[o + j]; }
    ma = wave_max(ma); mb = wave_max(mb);
    double sa = 0.0, sb = 0.0;
    for (int j = lane; j < N; j += 64) { sa += exp((double)A[o + j] - ma); sb += exp((double)Bn[o + j] - mb); }
    sa = wave_sum(sa); sb = wave_sum(sb);
    int fp = f & 1, fn = (f >> 1) & 1;
    fp = wave_max(fp); fn = wave_max(fn);
    if (lane == 0) { la[i] = ma + log(sa); lb[i] = mb + log(sb); rm[i] = fp && fn; }
}

// column j: the same over the M rows.  A workgroup owns 16 columns; 16 row stripes per column, combined in stripe order.
__global__ __launch_bounds__(256) void circle_cols_kernel(int M, int N, const float* __restrict__ A, const float* __restrict__ Bn,
                                                          const uint8_t* __restrict__ flags, double* __restrict__ la, double* __restrict__ lb,
                                                          int* __restrict__ cm) {
    __shared__ float smax[2][16][16];
    __shared__ double ssum[2][16][16];
    __shared__ int sf[16][16];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4, j = blockIdx.x * 16 + tx;
    float ma = -INFINITY, mb = -INFINITY;
    int f = 0;
    if (j < N)
        for (int i = ty; i < M; i += 16) { const size_t e = (size_t)i * N + j; ma = fmaxf(ma, A[e]); mb = fmaxf(mb, Bn[e]); f |= flags[e]; }
    smax[0][ty][tx] = ma; smax[1][ty][tx] = mb; sf[ty][tx] = f;
    __syncthreads();
    ma = -INFINITY; mb = -INFINITY; f = 0;
    for (int r = 0; r < 16; ++r) { ma = fmaxf(ma, smax[0][r][tx]); mb = fmaxf(mb, smax[1][r][tx]); f |= sf[r][tx]; }
    double sa = 0.0, sb = 0.0;
    if (j < N)
        for (int i = ty; i < M; i += 16) { const size_t e = (size_t)i * N + j; sa += exp((double)A[e] - ma); sb += exp((double)Bn[e] - mb); }
    ssum[0][ty][tx] = sa; ssum[1][ty][tx] = sb;
    __syncthreads();
    if (ty == 0 && j < N) {
        sa = 0.0; sb = 0.0;
        for (int r = 0; r < 16; ++r) { sa += ssum[0][r][tx]; sb += ssum[1][r][tx]; }
        la[j] = ma + log(sa); lb[j] = mb + log(sb); cm[j] = (f & 1) && (f & 2);
    }
}

__device__ __forceinline__ double softplus20(double x) { return x > 20.0 ? x : log1p(exp(x)); }   // F.softplus(beta = 1, threshold = 20)
__device__ __forceinline__ double softplus20_grad(double x) { if (x > 20.0) return 1.0; const double z = exp(x); return z / (z + 1.0); }

// sum of v[0..n) over one workgroup, fixed order (strided per thread, then a tree over the 256 threads)
__device__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// loss = (mean over the anchor rows of softplus(la + lb) / ls + the same over the anchor columns) / 2; coefficient of row i in d loss / d D:
// 0.5 / |rows| * softplus'(la_i + lb_i) (the 1 / ls of the loss cancels the ls of the logits), 0 outside the anchors
__global__ __launch_bounds__(256) void circle_final_kernel(int M, int N, float log_scale, const double* __restrict__ la_r, const double* __restrict__ lb_r,
                                                           const int* __restrict__ rm, const double* __restrict__ la_c, const double* __restrict__ lb_c,
                                                           const int* __restrict__ cm, double* __restrict__ cr, double* __restrict__ cc,
                                                           float* __restrict__ loss) {
    __shared__ double red[256];
    double s = 0.0, n = 0.0;
    for (int i = threadIdx.x; i < M; i += 256)
        if (rm[i]) { s += softplus20(la_r[i] + lb_r[i]) / (double)log_scale; n += 1.0; }
    const double sr = block_sum(s, red), nr = block_sum(n, red);
    s = 0.0; n = 0.0;
    for (int j = threadIdx.x; j < N; j += 256)
        if (cm[j]) { s += softplus20(la_c[j] + lb_c[j]) / (double)log_scale; n += 1.0; }
    const double sc = block_sum(s, red), nc = block_sum(n, red);
    for (int i = threadIdx.x; i < M; i += 256) cr[i] = (rm[i] && nr > 0) ? 0.5 / nr * softplus20_grad(la_r[i] + lb_r[i]) : 0.0;
    for (int j = threadIdx.x; j < N; j += 256) cc[j] = (cm[j] && nc > 0) ? 0.5 / nc * softplus20_grad(la_c[j] + lb_c[j]) : 0.0;
    if (threadIdx.x == 0 && loss) *loss = (float)((sr / nr + sc / nc) / 2.0);
}

// d loss / d sim [M, ldg = N4] and its transpose [N, ldgt = M4] (zeros in the pad), 32 x 32 tiles
__global__ __launch_bounds__(256) void circle_grad_kernel(int M, int N, int M4, int N4, const float* __restrict__ S, const float* __restrict__ Omin,
                                                          const float* __restrict__ Omax, const float* __restrict__ A, const float* __restrict__ Bn, CircleArgs a,
                                                          const double* __restrict__ la_r, const double* __restrict__ lb_r, const double* __restrict__ la_c,
                                                          const double* __restrict__ lb_c, const double* __restrict__ cr, const double* __restrict__ cc,
                                                          const float* __restrict__ grad_loss, float* __restrict__ G, float* __restrict__ GT) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    const float gl = grad_loss ? *grad_loss : 1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = i0 + ty + 8 * k, j = j0 + tx;
        float v = 0.f;
        if (i < M && j < N) {
            const size_t e = (size_t)i * N + j;
            const Elem el = circle_elem(S[e], Omin[e], Omax[e], a);
            const double ea = (double)A[e], eb = (double)Bn[e];
            const double gD = cr[i] * (exp(ea - la_r[i]) * el.pw - exp(eb - lb_r[i]) * el.nw) +
                              cc[j] * (exp(ea - la_c[j]) * el.pw - exp(eb - lb_c[j]) * el.nw);
            v = el.pass ? (float)(-gD / (double)el.D * (double)gl) : 0.f;
        }
        tile[ty + 8 * k][tx] = v;
        if (i < M && j < N4) G[(size_t)i * N4 + j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = j0 + ty + 8 * k, i = i0 + tx;
        if (j < N && i < M4) GT[(size_t)j * M4 + i] = tile[tx][ty + 8 * k];
    }
}

__global__ __launch_bounds__(256) void l2norm_fwd_kernel(int rows, int C, const float* __restrict__ x, float eps, float* __restrict__ y,
                                                         float* __restrict__ nrm) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float* xr = x + (size_t)r * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(xr[c], xr[c], s);
    const float n = sqrtf(wave_sum(s)), den = fmaxf(n, eps);
    for (int c = lane; c < C; c += 64) y[(size_t)r * C + c] = xr[c] / den;
    if (lane == 0) nrm[r] = n;
}

// x / max(|x|, eps): grad_x = (g - y (g . y)) / |x| where |x| >= eps (clamp_min passes the gradient there), g / eps below
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(int rows, int C, const float* __restrict__ y, const float* __restrict__ nrm, float eps,
                                                         const float* __restrict__ g, float* __restrict__ gx) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= rows) return;
    const size_t o = (size_t)r * C;
    const float n = nrm[r];
    if (n >= eps) {
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s = fmaf(g[o + c], y[o + c], s);
        s = wave_sum(s);
        for (int c = lane; c < C; c += 64) gx[o + c] = (g[o + c] - y[o + c] * s) / n;
    } else {
        for (int c = lane; c < C; c += 64) gx[o + c] = g[o + c] / eps;
    }
}

struct CircleWs {
    float *S, *Omin, *Omax, *A, *Bn, *G, *GT, *Timg, *Tpcd;
    uint8_t* flags;
    double *la_r, *lb_r, *la_c, *lb_c, *cr, *cc;
    int *rm, *cm;
    static size_t carve(void* buf, CircleWs& w, int M, int N, int C) {
        Carver c(buf);
        const size_t MN = (size_t)M * N, M4 = up4(M), N4 = up4(N);
        w.S = c.take<float>(MN); w.Omin = c.take<float>(MN); w.Omax = c.take<float>(MN); w.A = c.take<float>(MN); w.Bn = c.take<float>(MN);
        w.G = c.take<float>((size_t)M * N4); w.GT = c.take<float>((size_t)N * M4); w.Timg = c.take<float>((size_t)C * M4); w.Tpcd = c.take<float>((size_t)C * N4);
        w.flags = reinterpret_cast<uint8_t*>(c.take<float>((MN + 3) / 4));
        w.la_r = reinterpret_cast<double*>(c.take<float>(2 * (size_t)M)); w.lb_r = reinterpret_cast<double*>(c.take<float>(2 * (size_t)M));
        w.la_c = reinterpret_cast<double*>(c.take<float>(2 * (size_t)N)); w.lb_c = reinterpret_cast<double*>(c.take<float>(2 * (size_t)N));
        w.cr = reinterpret_cast<double*>(c.take<float>(2 * (size_t)M)); w.cc = reinterpret_cast<double*>(c.take<float>(2 * (size_t)N));
        w.rm = reinterpret_cast<int*>(c.take<float>(M)); w.cm = reinterpret_cast<int*>(c.take<float>(N));
        return c.off + 256;
    }
};

CircleArgs circle_args(const dr_circle_loss_params* p) {
    CircleArgs a;
    a.pos_margin = p->pos_margin; a.neg_margin = p->neg_margin; a.pos_optimal = p->pos_optimal; a.neg_optimal = p->neg_optimal;
    a.log_scale = p->log_scale; a.pos_overlap = p->pos_overlap; a.neg_overlap = p->neg_overlap;
    return a;
}

// similarity, overlaps, logits, row / column statistics, loss and gradient coefficients
int circle_forward(int M, int N, int C, const float* img, const float* pcd, int K, const int64_t* ii, const int64_t* jj, const float* omin,
                   const float* omax, const CircleArgs& a, float* loss, CircleWs& w, hipStream_t st) {
    Gemms G;
    G.add(img, C, pcd, w.S, N, M, N, C);
    int rc = G.launch(st);
    if (rc) return rc;
    const size_t MN = (size_t)M * N;
    DR_HIP_CHECK(hipMemsetAsync(w.Omin, 0, MN * sizeof(float), st));
    DR_HIP_CHECK(hipMemsetAsync(w.Omax, 0, MN * sizeof(float), st));
    if (K > 0) {
        hipLaunchKernelGGL(overlap_scatter_kernel, dim3((K + 255) / 256), dim3(256), 0, st, K, M, N, ii, jj, omin, omax, w.Omin, w.Omax);
        DR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(circle_logits_kernel, dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, st, (long long)MN, w.S, w.Omin, w.Omax, a, w.A, w.Bn,
                       w.flags);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(circle_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, st, M, N, w.A, w.Bn, w.flags, w.la_r, w.lb_r, w.rm);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(circle_cols_kernel, dim3((N + 15) / 16), dim3(256), 0, st, M, N, w.A, w.Bn, w.flags, w.la_c, w.lb_c, w.cm);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(circle_final_kernel, dim3(1), dim3(256), 0, st, M, N, a.log_scale, w.la_r, w.lb_r, w.rm, w.la_c, w.lb_c, w.cm, w.cr, w.cc,
                       loss);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

bool circle_args_ok(int M, int N, int C, const float* img, const float* pcd, int K, const int64_t* ii, const int64_t* jj, const float* omin,
                    const float* omax, const dr_circle_loss_params* p) {
    if (M < 1 || N < 1 || C < 4 || C % 4 || !img || !pcd || !p || K < 0) return false;
    if (K > 0 && (!ii || !jj || !omin || !omax)) return false;
    return p->log_scale > 0.f;
}

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" {

int dr_l2_normalize_f32(int rows, int C, const float* x, float eps, float* y, float* norms, void* stream) {
    if (rows < 0 || C < 1 || !x || !y || !norms || !(eps > 0.f)) return DR_EINVAL;
    if (rows == 0) return DR_OK;
    hipLaunchKernelGGL(l2norm_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, rows, C, x, eps, y, norms);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_l2_normalize_backward_f32(int rows, int C, const float* y, const float* norms, float eps, const float* grad_y, float* grad_x, void* stream) {
    if (rows < 0 || C < 1 || !y || !norms || !grad_y || !grad_x || !(eps > 0.f)) return DR_EINVAL;
    if (rows == 0) return DR_OK;
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, rows, C, y, norms, eps, grad_y, grad_x);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_circle_loss_workspace_bytes(int M, int N, int C) {
    if (M < 1 || N < 1 || C < 1) return 0;
    CircleWs w;
    return CircleWs::carve(nullptr, w, M, N, C);
}

int dr_circle_loss_f32(int M, int N, int C, const float* img, const float* pcd, int K, const int64_t* img_idx, const int64_t* pcd_idx,
                       const float* min_overlaps, const float* max_overlaps, const dr_circle_loss_params* params, float* loss, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!circle_args_ok(M, N, C, img, pcd, K, img_idx, pcd_idx, min_overlaps, max_overlaps, params) || !loss) return DR_EINVAL;
    if (!workspace || workspace_bytes < dr_circle_loss_workspace_bytes(M, N, C)) return DR_EWORKSPACE;
    CircleWs w;
    CircleWs::carve(workspace, w, M, N, C);
    return circle_forward(M, N, C, img, pcd, K, img_idx, pcd_idx, min_overlaps, max_overlaps, circle_args(params), loss, w, (hipStream_t)stream);
}

int dr_circle_loss_backward_f32(int M, int N, int C, const float* img, const float* pcd, int K, const int64_t* img_idx, const int64_t* pcd_idx,
                                const float* min_overlaps, const float* max_overlaps, const dr_circle_loss_params* params, const float* grad_loss,
                                float* loss, float* grad_img, float* grad_pcd, void* workspace, size_t workspace_bytes, void* stream) {
    if (!circle_args_ok(M, N, C, img, pcd, K, img_idx, pcd_idx, min_overlaps, max_overlaps, params) || !grad_img || !grad_pcd) return DR_EINVAL;
    if (!workspace || workspace_bytes < dr_circle_loss_workspace_bytes(M, N, C)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    CircleWs w;
    CircleWs::carve(workspace, w, M, N, C);
    const CircleArgs a = circle_args(params);
    int rc = circle_forward(M, N, C, img, pcd, K, img_idx, pcd_idx, min_overlaps, max_overlaps, a, loss, w, st);
    if (rc) return rc;
    const int M4 = up4(M), N4 = up4(N);
    Transposer T;
    T.add(img, M, C, C, w.Timg, M4);
    T.add(pcd, N, C, C, w.Tpcd, N4);
    if ((rc = T.launch(st))) return rc;
    hipLaunchKernelGGL(circle_grad_kernel, dim3((N4 + 31) / 32, (M4 + 31) / 32), dim3(256), 0, st, M, N, M4, N4, w.S, w.Omin, w.Omax, w.A, w.Bn, a,
                       w.la_r, w.lb_r, w.la_c, w.lb_c, w.cr, w.cc, grad_loss, w.G, w.GT);
    DR_LAUNCH_CHECK();
    Gemms G;
    G.add(w.G, N4, w.Tpcd, grad_img, C, M, C, N4);      // G pcd
    G.add(w.GT, M4, w.Timg, grad_pcd, C, N, C, M4);     // G^T img
    return G.launch(st);
}

}  // extern "C"
