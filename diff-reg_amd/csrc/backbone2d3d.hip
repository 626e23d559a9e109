// backbone2d3d.hip -- the three pieces of the 2D-3D model's point backbone (EXP/point_backbone.py:8-95, vision3d's KPConv FPN) that the
// KPFCN kernels (backbone.hip / backbone_bwd.hip) do not already cover.  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.
//   group_norm_stats / group_norm_apply   GroupNormPackMode (vision3d/layers/basic_layers/norm.py:53-65): nn.GroupNorm(G, C, eps, affine)
//                   over the transposed [1, C, N] rows -- per group statistics over all N rows x C/G channels, biased variance -- with the
//                   per-channel affine, fused with the residual sum of KPResidualBlock (vision3d/layers/kpconv.py:266-280: the shortcut's own
//                   GroupNorm, or the identity shortcut added raw) and LeakyReLU.  Statistics are float64 partials over a fixed grid of row
//                   slabs (no float atomics), then one fixed-order pass per group.
//   group_norm_backward   the same chain backwards: d a, d b, d gamma, d beta of each normalised operand; the LeakyReLU derivative is read off
//                   the output's sign (as norm_backward); column reductions in float64 over the same fixed grid.
//   knn_interpolate   knn_interpolate_pack_mode with k = None (vision3d/ops/knn_interpolate.py:43-77): weights mask / (d^2 + 1e-8)
//                   normalised by (sum + 1e-8); the shadow support point (index Ns, at the origin) is masked out, an all-shadow row gives
//                   zeros.  One wave per query row, written straight into a column slice (ldo) of the decoder's concatenation buffer.
//                   Backward: fp32 atomics into the support rows (the upsampling relation is not symmetric: no gather form without inverse
//                   lists).
//   kpconv_neighbor_count   the neighbour count of KPConv's normalisation (kpconv.py:137-139) as kpconv_gather_kernel computes it (same
//                   per-lane channel order, same wave reduction): read by the tests, never on the hot path.
#include "kernels.h"

namespace dr {

constexpr int GN_MAXH = 64;

static int gn_slabs(int N) {
    const int R = (N + 255) / 256;
    return R > 64 ? 64 : (R > 0 ? R : 1);
}

// ---- GroupNorm statistics: stage 1 per-column partial (sum, sum of squares) in float64 over R row slabs ------------------------------------------
__global__ __launch_bounds__(256) void gn_partial_kernel(int N, int C, const float* __restrict__ x, int ldx, int rows_per, double* __restrict__ part) {
    // block = 32 channels x 8 row lanes; grid = (ceil(C/32), R)
    __shared__ double s_s[8][32], s_q[8][32];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    const int r0 = blockIdx.y * rows_per, r1 = min(N, r0 + rows_per);
    double s = 0.0, qq = 0.0;
    if (c < C)
        for (int r = r0 + rl; r < r1; r += 8) {
            const double v = (double)x[(size_t)r * ldx + c];
            s += v; qq += v * v;
        }
    s_s[rl][cl] = s; s_q[rl][cl] = qq;
    __syncthreads();
    if (rl == 0 && c < C) {
        for (int k = 1; k < 8; ++k) { s += s_s[k][cl]; qq += s_q[k][cl]; }
        part[((size_t)blockIdx.y * C + c) * 2] = s;
        part[((size_t)blockIdx.y * C + c) * 2 + 1] = qq;
    }
}

// stage 2: one thread per group, columns then slabs in a fixed order
__global__ __launch_bounds__(256) void gn_final_kernel(int N, int C, int G, int R, const double* __restrict__ part, float eps, float* __restrict__ mean,
                                                       float* __restrict__ rstd) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int Cg = C / G;
    double s = 0.0, qq = 0.0;
    for (int c = g * Cg; c < (g + 1) * Cg; ++c)
        for (int r = 0; r < R; ++r) { s += part[((size_t)r * C + c) * 2]; qq += part[((size_t)r * C + c) * 2 + 1]; }
    const double cnt = (double)N * Cg;
    const double m = s / cnt;
    double var = qq / cnt - m * m;                                  // biased variance (nn.GroupNorm)
    if (var < 0) var = 0;
    mean[g] = (float)m;
    rstd[g] = (float)(1.0 / sqrt(var + (double)eps));
}

// out = act( gamma_a (a - mean_a[g]) rstd_a[g] + beta_a + [ gamma_b (b - mean_b[g]) rstd_b[g] + beta_b  |  b  |  0 ] )
__global__ __launch_bounds__(256) void gn_apply_kernel(int N, int C, int Cg, const float* __restrict__ a, int lda, const float* __restrict__ ma,
                                                       const float* __restrict__ ra, const float* __restrict__ ga, const float* __restrict__ ba,
                                                       const float* __restrict__ b, int ldb, const float* __restrict__ mb, const float* __restrict__ rb,
                                                       const float* __restrict__ gb, const float* __restrict__ bb, float slope, int act,
                                                       float* __restrict__ out, int ldo) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * C) return;
    const int r = (int)(e / C), c = (int)(e % C), g = c / Cg;
    float v = (a[(size_t)r * lda + c] - ma[g]) * ra[g] * ga[c] + ba[c];
    if (b) {
        float u = b[(size_t)r * ldb + c];
        if (mb) u = (u - mb[g]) * rb[g] * gb[c] + bb[c];
        v += u;
    }
    if (act) v = v > 0.f ? v : v * slope;
    out[(size_t)r * ldo + c] = v;
}

size_t gn_workspace_bytes(int N, int C) { return (size_t)gn_slabs(N) * C * 2 * sizeof(double); }

int launch_gn_stats(int N, int C, int G, const float* x, int ldx, float eps, float* mean, float* rstd, void* ws, size_t ws_bytes, hipStream_t st) {
    if (N <= 0) return DR_OK;
    if (!ws || ws_bytes < gn_workspace_bytes(N, C)) return DR_EWORKSPACE;
    const int R = gn_slabs(N), rows_per = (N + R - 1) / R;
    hipLaunchKernelGGL(gn_partial_kernel, dim3((C + 31) / 32, R), dim3(256), 0, st, N, C, x, ldx, rows_per, (double*)ws);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gn_final_kernel, dim3((G + 255) / 256), dim3(256), 0, st, N, C, G, R, (const double*)ws, eps, mean, rstd);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// ---- GroupNorm backward ------------------------------------------------------------------------------------------------------------------
// g' = g act'(out).  Per column over the slabs: [sum g', sum g' xhat_a, sum g' xhat_b] (float64); then per column d beta = sum g', d gamma_a =
// sum g' xhat_a, d gamma_b = sum g' xhat_b, and per group the means of (gamma g') and (gamma g' xhat) over N x C/G entries.
__global__ __launch_bounds__(256) void gn_bwd_partial_kernel(int N, int C, int Cg, const float* __restrict__ gout, int ldg, const float* __restrict__ out,
                                                             int ldo, const float* __restrict__ a, int lda, const float* __restrict__ ma,
                                                             const float* __restrict__ ra, const float* __restrict__ b, int ldb,
                                                             const float* __restrict__ mb, const float* __restrict__ rb, float slope, int act,
                                                             int rows_per, double* __restrict__ part) {
    __shared__ double s0[8][32], s1[8][32], s2[8][32];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    const int r0 = blockIdx.y * rows_per, r1 = min(N, r0 + rows_per);
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    if (c < C) {
        const int g = c / Cg;
        const float m_a = ma[g], r_a = ra[g], m_b = mb ? mb[g] : 0.f, r_b = mb ? rb[g] : 0.f;
        for (int r = r0 + rl; r < r1; r += 8) {
            float gv = gout[(size_t)r * ldg + c];
            if (act && !(out[(size_t)r * ldo + c] > 0.f)) gv *= slope;
            t0 += (double)gv;
            t1 += (double)gv * (double)((a[(size_t)r * lda + c] - m_a) * r_a);
            if (mb) t2 += (double)gv * (double)((b[(size_t)r * ldb + c] - m_b) * r_b);
        }
    }
    s0[rl][cl] = t0; s1[rl][cl] = t1; s2[rl][cl] = t2;
    __syncthreads();
    if (rl == 0 && c < C) {
        for (int k = 1; k < 8; ++k) { t0 += s0[k][cl]; t1 += s1[k][cl]; t2 += s2[k][cl]; }
        double* p = part + ((size_t)blockIdx.y * C + c) * 3;
        p[0] = t0; p[1] = t1; p[2] = t2;
    }
}

// one block: the column totals (d gamma, d beta; float64 copies kept for the group pass), a barrier, then one thread per group.
// red[4 G] = per group: mean(gamma_a g'), mean(gamma_a g' xhat_a), mean(gamma_b g'), mean(gamma_b g' xhat_b)
__global__ __launch_bounds__(256) void gn_bwd_final_kernel(int N, int C, int G, int R, const double* __restrict__ part, const float* __restrict__ gam_a,
                                                           const float* __restrict__ gam_b, double* __restrict__ tot, float* __restrict__ red,
                                                           float* __restrict__ dgamma_a, float* __restrict__ dbeta_a, float* __restrict__ dgamma_b,
                                                           float* __restrict__ dbeta_b) {
    for (int c = threadIdx.x; c < C; c += 256) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        for (int r = 0; r < R; ++r) { const double* p = part + ((size_t)r * C + c) * 3; t0 += p[0]; t1 += p[1]; t2 += p[2]; }
        tot[c * 3] = t0; tot[c * 3 + 1] = t1; tot[c * 3 + 2] = t2;
        if (dbeta_a) dbeta_a[c] = (float)t0;
        if (dgamma_a) dgamma_a[c] = (float)t1;
        if (dbeta_b) dbeta_b[c] = (float)t0;
        if (dgamma_b) dgamma_b[c] = (float)t2;
    }
    __syncthreads();
    const int Cg = C / G;
    const double cnt = (double)N * Cg;
    for (int g = threadIdx.x; g < G; g += 256) {
        double u0 = 0.0, u1 = 0.0, v0 = 0.0, v1 = 0.0;
        for (int c = g * Cg; c < (g + 1) * Cg; ++c) {
            u0 += (double)gam_a[c] * tot[c * 3]; u1 += (double)gam_a[c] * tot[c * 3 + 1];
            if (gam_b) { v0 += (double)gam_b[c] * tot[c * 3]; v1 += (double)gam_b[c] * tot[c * 3 + 2]; }
        }
        red[g * 4] = (float)(u0 / cnt); red[g * 4 + 1] = (float)(u1 / cnt); red[g * 4 + 2] = (float)(v0 / cnt); red[g * 4 + 3] = (float)(v1 / cnt);
    }
}

// grad_a = rstd_a (gamma_a g' - mean(gamma_a g') - xhat_a mean(gamma_a g' xhat_a));  grad_b likewise with b's statistics | g' (identity shortcut)
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(int N, int C, int Cg, const float* __restrict__ gout, int ldg, const float* __restrict__ out,
                                                           int ldo, const float* __restrict__ a, int lda, const float* __restrict__ ma,
                                                           const float* __restrict__ ra, const float* __restrict__ gam_a, const float* __restrict__ b,
                                                           int ldb, const float* __restrict__ mb, const float* __restrict__ rb,
                                                           const float* __restrict__ gam_b, float slope, int act, const float* __restrict__ red,
                                                           float* __restrict__ ga, int ldga, float* __restrict__ gb, int ldgb) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)N * C) return;
    const int r = (int)(e / C), c = (int)(e % C), g = c / Cg;
    float gv = gout[(size_t)r * ldg + c];
    if (act && !(out[(size_t)r * ldo + c] > 0.f)) gv *= slope;
    if (ga) {
        const float xa = (a[(size_t)r * lda + c] - ma[g]) * ra[g];
        ga[(size_t)r * ldga + c] = ra[g] * (gam_a[c] * gv - red[g * 4] - xa * red[g * 4 + 1]);
    }
    if (gb) {
        if (mb) {
            const float xb = (b[(size_t)r * ldb + c] - mb[g]) * rb[g];
            gb[(size_t)r * ldgb + c] = rb[g] * (gam_b[c] * gv - red[g * 4 + 2] - xb * red[g * 4 + 3]);
        } else gb[(size_t)r * ldgb + c] = gv;
    }
}

size_t gn_backward_workspace_bytes(int N, int C, int G) {
    return (size_t)gn_slabs(N) * C * 3 * sizeof(double) + (size_t)C * 3 * sizeof(double) + (size_t)G * 4 * sizeof(float) + 64;
}

// ---- kNN interpolation ----------------------------------------------------------------------------------------------------------------------
// one wave per query; lane h < H computes neighbour h's weight, the wave sums them (fixed butterfly order), each lane then owns channels
// lane, lane + 64, ...
__device__ __forceinline__ void knn_weights(int q, int Ns, int H, const float* __restrict__ q_pts, const float* __restrict__ s_pts,
                                            const long long* __restrict__ nb, int lane, float* s_w, int* s_idx) {
    float wv = 0.f;
    int id = -1;
    if (lane < H) {
        const long long j = nb[(size_t)q * H + lane];
        if (j >= 0 && j < Ns) {                                     // the shadow index Ns is masked (knn_interpolate.py:72)
            id = (int)j;
            const float dx = q_pts[q * 3] - s_pts[j * 3], dy = q_pts[q * 3 + 1] - s_pts[j * 3 + 1], dz = q_pts[q * 3 + 2] - s_pts[j * 3 + 2];
            wv = 1.f / (dx * dx + dy * dy + dz * dz + 1e-8f);
        }
    }
    const float tot = wave_sum(wv);
    s_w[lane] = wv / (tot + 1e-8f);
    s_idx[lane] = id;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void knn_interp_kernel(int Nq, int Ns, int H, int C, const float* __restrict__ q_pts, const float* __restrict__ s_pts,
                                                         const long long* __restrict__ nb, const float* __restrict__ x, float* __restrict__ out, int ldo) {
    __shared__ float s_w[4][64];
    __shared__ int s_idx[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + w;
    if (q >= Nq) return;
    knn_weights(q, Ns, H, q_pts, s_pts, nb, lane, s_w[w], s_idx[w]);
    for (int c = lane; c < C; c += 64) {
        float acc = 0.f;
        for (int h = 0; h < H; ++h) {
            const int j = s_idx[w][h];
            if (j >= 0) acc = fmaf(s_w[w][h], x[(size_t)j * C + c], acc);
        }
        out[(size_t)q * ldo + c] = acc;
    }
}

__global__ __launch_bounds__(256) void knn_interp_bwd_kernel(int Nq, int Ns, int H, int C, const float* __restrict__ q_pts, const float* __restrict__ s_pts,
                                                             const long long* __restrict__ nb, const float* __restrict__ gout, int ldg,
                                                             float* __restrict__ gx) {
    __shared__ float s_w[4][64];
    __shared__ int s_idx[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + w;
    if (q >= Nq) return;
    knn_weights(q, Ns, H, q_pts, s_pts, nb, lane, s_w[w], s_idx[w]);
    for (int c = lane; c < C; c += 64) {
        const float gv = gout[(size_t)q * ldg + c];
        for (int h = 0; h < H; ++h) {
            const int j = s_idx[w][h];
            const float wt = s_w[w][h];
            if (j >= 0 && wt != 0.f && gv != 0.f) atomicAdd(gx + (size_t)j * C + c, wt * gv);
        }
    }
}

// ---- KPConv's neighbour count, summed exactly as kpconv_gather_kernel sums it ---------------------------------------------------------------
__global__ __launch_bounds__(256) void kp_count_kernel(int Nq, int Ns, int H, int Cin, int cpl, const long long* __restrict__ nb,
                                                       const float* __restrict__ x, int* __restrict__ counts) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + w;
    if (q >= Nq) return;
    int num = 0;
    for (int h = 0; h < H; ++h) {
        const long long id = nb[(size_t)q * H + h];
        if (id >= Ns || id < 0) continue;
        float part = 0.f;
        for (int c = 0; c < cpl; ++c) {
            const int ch = lane + 64 * c;
            part += ch < Cin ? x[(size_t)id * Cin + ch] : 0.f;
        }
        part = wave_sum(part);
        num += part > 0.f ? 1 : 0;
    }
    if (lane == 0) counts[q] = num;
}

}  // namespace dr

using namespace dr;

extern "C" {

size_t dr_group_norm_workspace_bytes(int N, int C) { return (N > 0 && C > 0) ? gn_workspace_bytes(N, C) : 0; }

int dr_group_norm_stats_f32(int N, int C, int G, const float* x, int ldx, float eps, float* mean, float* rstd, void* workspace, size_t workspace_bytes,
                            void* stream) {
    if (N < 1 || C < 1 || G < 1 || C % G || !x || !mean || !rstd || ldx < C || !(eps > 0.f)) return DR_EINVAL;
    return launch_gn_stats(N, C, G, x, ldx, eps, mean, rstd, workspace, workspace_bytes, (hipStream_t)stream);
}

int dr_group_norm_apply_f32(int N, int C, int G, const float* a, int lda, const float* mean_a, const float* rstd_a, const float* gamma_a, const float* beta_a,
                            const float* b, int ldb, const float* mean_b, const float* rstd_b, const float* gamma_b, const float* beta_b, float leaky_slope,
                            int activate, float* out, int ldo, void* stream) {
    if (N < 0 || C < 1 || G < 1 || C % G || !a || !mean_a || !rstd_a || !gamma_a || !beta_a || !out || lda < C || ldo < C) return DR_EINVAL;
    if (b && ldb < C) return DR_EINVAL;
    if (mean_b && (!b || !rstd_b || !gamma_b || !beta_b)) return DR_EINVAL;
    if (N == 0) return DR_OK;
    const size_t n = (size_t)N * C;
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, C, C / G, a, lda, mean_a, rstd_a, gamma_a,
                       beta_a, b, ldb, mean_b, rstd_b, gamma_b, beta_b, leaky_slope, activate, out, ldo);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_group_norm_backward_workspace_bytes(int N, int C, int G) { return (N > 0 && C > 0 && G > 0) ? gn_backward_workspace_bytes(N, C, G) : 0; }

int dr_group_norm_backward_f32(int N, int C, int G, const float* grad_out, int ldg, const float* out, int ldo, const float* a, int lda, const float* mean_a,
                               const float* rstd_a, const float* gamma_a, const float* b, int ldb, const float* mean_b, const float* rstd_b,
                               const float* gamma_b, float leaky_slope, int activate, float* grad_a, int ldga, float* grad_gamma_a, float* grad_beta_a,
                               float* grad_b, int ldgb, float* grad_gamma_b, float* grad_beta_b, void* workspace, size_t workspace_bytes, void* stream) {
    if (N < 1 || C < 1 || G < 1 || C % G || !grad_out || !a || !mean_a || !rstd_a || !gamma_a || ldg < C || lda < C || (activate && (!out || ldo < C)))
        return DR_EINVAL;
    if ((grad_a && ldga < C) || (grad_b && (!b || ldgb < C)) || (b && ldb < C)) return DR_EINVAL;
    if (mean_b && (!b || !rstd_b || !gamma_b)) return DR_EINVAL;
    if (!mean_b && (grad_gamma_b || grad_beta_b)) return DR_EINVAL;
    if (!workspace || workspace_bytes < gn_backward_workspace_bytes(N, C, G)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int R = gn_slabs(N), rows_per = (N + R - 1) / R;
    double* part = (double*)workspace;
    double* tot = part + (size_t)R * C * 3;
    float* red = (float*)(tot + (size_t)C * 3);
    hipLaunchKernelGGL(gn_bwd_partial_kernel, dim3((C + 31) / 32, R), dim3(256), 0, st, N, C, C / G, grad_out, ldg, out, ldo, a, lda, mean_a, rstd_a, b, ldb,
                       mean_b, rstd_b, leaky_slope, activate, rows_per, part);
    DR_LAUNCH_CHECK();
    hipLaunchKernelGGL(gn_bwd_final_kernel, dim3(1), dim3(256), 0, st, N, C, G, R, (const double*)part, gamma_a, mean_b ? gamma_b : nullptr, tot, red,
                       grad_gamma_a, grad_beta_a, grad_gamma_b, grad_beta_b);
    DR_LAUNCH_CHECK();
    if (grad_a || grad_b) {
        const size_t n = (size_t)N * C;
        hipLaunchKernelGGL(gn_bwd_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, N, C, C / G, grad_out, ldg, out, ldo, a, lda, mean_a,
                           rstd_a, gamma_a, b, ldb, mean_b, rstd_b, gamma_b, leaky_slope, activate, (const float*)red, grad_a, ldga, grad_b, ldgb);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

int dr_knn_interpolate_f32(int Nq, int Ns, int H, int C, const float* q_pts, const float* s_pts, const int64_t* neighb_inds, const float* x, float* out,
                           int ldo, void* stream) {
    if (Nq < 0 || Ns < 0 || H < 1 || C < 1 || ldo < C || !q_pts || !neighb_inds || !out || (Ns > 0 && (!s_pts || !x))) return DR_EINVAL;
    if (H > GN_MAXH) return DR_ENOSUP;
    if (Nq == 0) return DR_OK;
    hipLaunchKernelGGL(knn_interp_kernel, dim3((Nq + 3) / 4), dim3(256), 0, (hipStream_t)stream, Nq, Ns, H, C, q_pts, s_pts,
                       (const long long*)neighb_inds, x, out, ldo);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_knn_interpolate_backward_f32(int Nq, int Ns, int H, int C, const float* q_pts, const float* s_pts, const int64_t* neighb_inds, const float* grad_out,
                                    int ldg, float* grad_x, void* stream) {
    if (Nq < 0 || Ns < 0 || H < 1 || C < 1 || ldg < C || !q_pts || !neighb_inds || !grad_out || (Ns > 0 && (!s_pts || !grad_x))) return DR_EINVAL;
    if (H > GN_MAXH) return DR_ENOSUP;
    hipStream_t st = (hipStream_t)stream;
    if (Ns > 0) DR_HIP_CHECK(hipMemsetAsync(grad_x, 0, (size_t)Ns * C * sizeof(float), st));
    if (Nq == 0 || Ns == 0) return DR_OK;
    hipLaunchKernelGGL(knn_interp_bwd_kernel, dim3((Nq + 3) / 4), dim3(256), 0, st, Nq, Ns, H, C, q_pts, s_pts, (const long long*)neighb_inds, grad_out,
                       ldg, grad_x);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_kpconv_neighbor_count_f32(int Nq, int Ns, int H, int Cin, const int64_t* neighb_inds, const float* x, int32_t* counts, void* stream) {
    if (Nq < 0 || Ns < 1 || H < 1 || Cin < 1 || !neighb_inds || !x || !counts) return DR_EINVAL;
    if (H > GN_MAXH || Cin > 512) return DR_ENOSUP;
    if (Nq == 0) return DR_OK;
    const int cpl = Cin <= 64 ? 1 : Cin <= 128 ? 2 : Cin <= 256 ? 4 : 8;       // the lane's channels, as kpconv_gather_kernel<CPL>
    hipLaunchKernelGGL(kp_count_kernel, dim3((Nq + 3) / 4), dim3(256), 0, (hipStream_t)stream, Nq, Ns, H, Cin, cpl, (const long long*)neighb_inds, x,
                       (int*)counts);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
