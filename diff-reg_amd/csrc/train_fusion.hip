// train_fusion.hip -- the vision3d TransformerLayer of the 2D-3D CrossModalFusionModule (Diff-Reg-2d3d/vision3d/layers/transformer.py:58-301) for
// TRAINING, in the two entry points of train_layer.hip: the forward that keeps what its backward needs, and the whole backward.
//   q = x Wq^T + bq, k = y Wk^T + bk, v = y Wv^T + bv;  o = softmax(q k^T / sqrt(d)) v per head;  z = LN1(o Wl^T + bl + x)
//   out = LN2(relu(z We^T + be) Ws^T + bs + z)                                                         (post-LN; no dropout on the path)
// The projections and every weight gradient run on the library's f32-input MFMA GEMM (launch_gemm: bias and residual in its epilogue), the
// attention on dr_attention_f32 / dr_attention_backward_f32.  New kernels: the post-LN backward (the residual branch's gradient added to the
// upstream one in the same pass; the LayerNorm's gamma / beta AND the preceding linear's bias gradient as column partials of its row block), a
// column-sum family for the other biases (fused with the ReLU backward for expand), and one fixed-order reduction of all partials.  No atomics:
// every sum has one order, so the backward is bit-reproducible between launches.
#include "train_common.h"

namespace dr {
namespace {

constexpr int FB_RB = 16;          // token rows per partial-sum block

// g_pre = LayerNorm backward of (g + g_res) at x_pre (mean, rstd in stats); per block of FB_RB rows: sum (g + g_res) xhat -> part_gamma,
// sum (g + g_res) -> part_beta, sum g_pre -> part_bias (the bias of the linear that feeds the LayerNorm).  One wave per row, lane columns
// c = lane + 64 j; the four waves' partials are added in wave order.
template <int CPL>
__global__ __launch_bounds__(256) void postln_bwd_kernel(int rows, int C, const float* __restrict__ x, const float* __restrict__ gamma,
                                                         const float* __restrict__ stats, const float* __restrict__ g, const float* __restrict__ g_res,
                                                         float* __restrict__ g_pre, float* __restrict__ part_gamma, float* __restrict__ part_beta,
                                                         float* __restrict__ part_bias) {
    __shared__ float red[4][64 * CPL];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float ag[CPL], ab[CPL], ap[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) { ag[j] = 0.f; ab[j] = 0.f; ap[j] = 0.f; }
    for (int i = 0; i < FB_RB / 4; ++i) {
        const int row = blockIdx.x * FB_RB + w + 4 * i;
        if (row >= rows) break;
        const float mean = stats[2 * row], rstd = stats[2 * row + 1];
        const size_t o = (size_t)row * C;
        float gy[CPL], xh[CPL], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + 64 * j;
            gy[j] = 0.f; xh[j] = 0.f;
            if (c < C) {
                gy[j] = g_res ? g[o + c] + g_res[o + c] : g[o + c];
                xh[j] = (x[o + c] - mean) * rstd;
                const float d = gy[j] * gamma[c];
                s1 += d; s2 = fmaf(d, xh[j], s2);
            }
        }
        s1 = wave_sum(s1) / (float)C; s2 = wave_sum(s2) / (float)C;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const int c = lane + 64 * j;
            if (c < C) {
                const float gp = rstd * (gy[j] * gamma[c] - s1 - xh[j] * s2);
                g_pre[o + c] = gp;
                ag[j] = fmaf(gy[j], xh[j], ag[j]); ab[j] += gy[j]; ap[j] += gp;
            }
        }
    }
    float* parts[3] = {part_gamma, part_beta, part_bias};
#pragma unroll
    for (int s = 0; s < 3; ++s) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) red[w][lane + 64 * j] = s == 0 ? ag[j] : (s == 1 ? ab[j] : ap[j]);
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += 256) parts[s][(size_t)blockIdx.x * C + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
        __syncthreads();
    }
}

// column sums of up to 4 matrices by blocks of FB_RB rows -> part [row block][cols]; `act` given: the ReLU backward first (the gradient passes
// where the activation is > 0, torch's threshold_backward) and the masked gradient is written to `dst` (may be `src`)
struct CsProblem { const float* src; const float* act; float* dst; float* part; int rows, cols, tile0, tiles_c; };
struct CsBatch { CsProblem p[4]; int n; };
__global__ __launch_bounds__(256) void colsum_batch_kernel(CsBatch G) {
    int pi = 0;
    while (pi + 1 < G.n && (int)blockIdx.x >= G.p[pi + 1].tile0) ++pi;
    const CsProblem& P = G.p[pi];
    const int tl = blockIdx.x - P.tile0, tr = tl / P.tiles_c, c = (tl % P.tiles_c) * 256 + threadIdx.x;
    if (c >= P.cols) return;
    float acc = 0.f;
    const int r1 = min(P.rows, (tr + 1) * FB_RB);
    for (int r = tr * FB_RB; r < r1; ++r) {
        const size_t e = (size_t)r * P.cols + c;
        float v = P.src[e];
        if (P.act) {
            v = P.act[e] > 0.f ? v : 0.f;
            P.dst[e] = v;
        }
        acc += v;
    }
    P.part[(size_t)tr * P.cols + c] = acc;
}
struct ColSums {
    CsBatch g;
    int tiles;
    ColSums() { memset(&g, 0, sizeof(g)); tiles = 0; }
    void add(const float* src, int rows, int cols, float* part, const float* act = nullptr, float* dst = nullptr) {
        CsProblem& p = g.p[g.n++];
        p.src = src; p.act = act; p.dst = dst; p.part = part; p.rows = rows; p.cols = cols; p.tile0 = tiles; p.tiles_c = (cols + 255) / 256;
        tiles += ((rows + FB_RB - 1) / FB_RB) * p.tiles_c;
    }
    int launch(hipStream_t st) {
        hipLaunchKernelGGL(colsum_batch_kernel, dim3(tiles), dim3(256), 0, st, g);
        DR_LAUNCH_CHECK();
        memset(&g, 0, sizeof(g)); tiles = 0;
        return DR_OK;
    }
};

// out[c] = sum over the row blocks of part[b][c], in block order (double accumulator), for up to 10 targets in one launch
struct FinTarget { const float* part; float* out; int nblk, n, tile0; };
struct FinBatch { FinTarget t[10]; int n; };
__global__ __launch_bounds__(256) void colsum_final_kernel(FinBatch G) {
    int ti = 0;
    while (ti + 1 < G.n && (int)blockIdx.x >= G.t[ti + 1].tile0) ++ti;
    const FinTarget& T = G.t[ti];
    const int c = (blockIdx.x - T.tile0) * 256 + threadIdx.x;
    if (c >= T.n) return;
    double s = 0.0;
    for (int b = 0; b < T.nblk; ++b) s += (double)T.part[(size_t)b * T.n + c];
    T.out[c] = (float)s;
}

inline int nblk(int rows) { return (rows + FB_RB - 1) / FB_RB; }

int launch_postln_bwd(int rows, int C, const float* x, const float* gamma, const float* stats, const float* g, const float* g_res, float* g_pre,
                      float* pg, float* pb, float* pbias, hipStream_t st) {
    const dim3 grid(nblk(rows)), blk(256);
    if (C <= 256) hipLaunchKernelGGL(postln_bwd_kernel<4>, grid, blk, 0, st, rows, C, x, gamma, stats, g, g_res, g_pre, pg, pb, pbias);
    else if (C <= 512) hipLaunchKernelGGL(postln_bwd_kernel<8>, grid, blk, 0, st, rows, C, x, gamma, stats, g, g_res, g_pre, pg, pb, pbias);
    else hipLaunchKernelGGL(postln_bwd_kernel<16>, grid, blk, 0, st, rows, C, x, gamma, stats, g, g_res, g_pre, pg, pb, pbias);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// what the forward keeps (floats): q | k | v, the heads' output o, LN1's input a (= linear(o) + x) and output z, the ReLU activation e, LN2's
// input f (= squeeze(e) + z), both LayerNorms' (mean, rstd) rows, and an all-ones query mask (used when key masks are given)
struct FSaved {
    float *q, *k, *v, *o, *a, *z, *e, *f, *st1, *st2;
    uint8_t* ones;
    static size_t carve(void* buf, FSaved& s, size_t R, size_t Q, int C) {
        Carver c(buf);
        s.q = c.take<float>(R * C); s.k = c.take<float>(Q * C); s.v = c.take<float>(Q * C); s.o = c.take<float>(R * C); s.a = c.take<float>(R * C); s.z = c.take<float>(R * C);
        s.e = c.take<float>(R * 2 * C); s.f = c.take<float>(R * C); s.st1 = c.take<float>(2 * R); s.st2 = c.take<float>(2 * R);
        s.ones = reinterpret_cast<uint8_t*>(c.take<float>((R + 3) / 4));
        return c.off + 256;
    }
};

// the backward's workspace (floats): activation gradients, the transposed weights ([Wk^T | Wv^T] side by side), the transposed activations and
// gradients (token count padded to a multiple of 4: the GEMM's k extent), the column partials by blocks of FB_RB rows (LN2 and LN1: gamma, beta
// and the preceding linear's bias, one after the other), the attention backward's own workspace
struct FBwdWs {
    float *g_f, *g_e, *g_z, *g_a, *g_o, *g_q, *g_k, *g_v;
    float *TWs, *TWe, *TWl, *TWq, *TWkv;
    float *T_e, *T_z, *T_o, *T_x, *T_y, *T_gf, *T_ge, *T_ga, *T_gq, *T_gk, *T_gv;
    float *p_ln2, *p_exp, *p_ln1, *p_q, *p_k, *p_v;
    float* att_ws;
    size_t att_wsb;
    static size_t carve(void* buf, FBwdWs& s, int B, int H, int L, int S, size_t C) {
        const size_t R = (size_t)B * L, Q = (size_t)B * S, R4 = up4((int)R), Q4 = up4((int)Q), C2 = 2 * C, nR = nblk((int)R), nQ = nblk((int)Q);
        Carver c(buf);
        s.g_f = c.take<float>(R * C); s.g_e = c.take<float>(R * C2); s.g_z = c.take<float>(R * C); s.g_a = c.take<float>(R * C); s.g_o = c.take<float>(R * C);
        s.g_q = c.take<float>(R * C); s.g_k = c.take<float>(Q * C); s.g_v = c.take<float>(Q * C);
        s.TWs = c.take<float>(C2 * C); s.TWe = c.take<float>(C2 * C); s.TWl = c.take<float>(C * C); s.TWq = c.take<float>(C * C); s.TWkv = c.take<float>(C2 * C);
        s.T_e = c.take<float>(C2 * R4); s.T_z = c.take<float>(C * R4); s.T_o = c.take<float>(C * R4); s.T_x = c.take<float>(C * R4); s.T_y = c.take<float>(C * Q4);
        s.T_gf = c.take<float>(C * R4); s.T_ge = c.take<float>(C2 * R4); s.T_ga = c.take<float>(C * R4); s.T_gq = c.take<float>(C * R4);
        s.T_gk = c.take<float>(C * Q4); s.T_gv = c.take<float>(C * Q4);
        s.p_ln2 = c.take<float>(nR * C * 3); s.p_exp = c.take<float>(nR * C2); s.p_ln1 = c.take<float>(nR * C * 3); s.p_q = c.take<float>(nR * C);
        s.p_k = c.take<float>(nQ * C); s.p_v = c.take<float>(nQ * C);
        s.att_wsb = dr_attention_backward_workspace_bytes(B, H, L);
        s.att_ws = c.take<float>(s.att_wsb / sizeof(float) + 64);
        return c.off + 256;
    }
};

bool fusion_args_ok(int C, int H, int B, int L, int S) {
    return B >= 1 && L >= 1 && S >= 1 && H >= 1 && C >= 4 && C <= 1024 && C % H == 0 && (C / H) % 4 == 0 && C / H <= 160 && C % 4 == 0;
}

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" {

size_t dr_fusion_layer_train_saved_bytes(int B, int L, int S, int C) {
    if (B < 1 || L < 1 || S < 1 || C < 4) return 0;
    FSaved s;
    return FSaved::carve(nullptr, s, (size_t)B * L, (size_t)B * S, C);
}

int dr_fusion_layer_train_forward_f32(const dr_fusion_layer_weights* w, int C, int H, int B, int L, int S, const float* x, const float* y,
                                      const uint8_t* y_mask, float* out, void* saved, size_t saved_bytes, void* stream) {
    if (!w || !x || !y || !out || !saved || !fusion_args_ok(C, H, B, L, S)) return DR_EINVAL;
    if (saved_bytes < dr_fusion_layer_train_saved_bytes(B, L, S, C)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int R = B * L, Q = B * S, d = C / H, C2 = 2 * C;
    FSaved sv;
    FSaved::carve(saved, sv, R, Q, C);
    Gemms G;
    G.add(x, C, w->q_w, sv.q, C, R, C, C).bias = w->q_b;
    G.add(y, C, w->k_w, sv.k, C, Q, C, C).bias = w->k_b;
    G.add(y, C, w->v_w, sv.v, C, Q, C, C).bias = w->v_b;
    int rc = G.launch(st);
    if (rc) return rc;
    const uint8_t* qm = nullptr;
    if (y_mask) {
        DR_HIP_CHECK(hipMemsetAsync(sv.ones, 1, (size_t)R, st));
        qm = sv.ones;
    }
    rc = dr_attention_f32(B, H, L, S, d, sv.q, sv.k, sv.v, C, qm, y_mask, 1.0f / sqrtf((float)d), sv.o, stream);
    if (rc) return rc;
    G.add(sv.o, C, w->lin_w, sv.a, C, R, C, C, EPI_NONE, x).bias = w->lin_b;                               // linear(o) + x
    if ((rc = G.launch(st))) return rc;
    if ((rc = dr_layernorm_f32(R, C, sv.a, w->norm1_w, w->norm1_b, 1e-5f, sv.z, sv.st1, stream))) return rc;
    G.add(sv.z, C, w->expand_w, sv.e, C2, R, C2, C, EPI_RELU).bias = w->expand_b;                          // relu(expand(z))
    if ((rc = G.launch(st))) return rc;
    G.add(sv.e, C2, w->squeeze_w, sv.f, C, R, C, C2, EPI_NONE, sv.z).bias = w->squeeze_b;                   // squeeze(e) + z
    if ((rc = G.launch(st))) return rc;
    return dr_layernorm_f32(R, C, sv.f, w->norm2_w, w->norm2_b, 1e-5f, out, sv.st2, stream);
}

size_t dr_fusion_layer_backward_workspace_bytes(int B, int H, int L, int S, int C) {
    if (B < 1 || L < 1 || S < 1 || C < 4 || H < 1) return 0;
    FBwdWs ws;
    return FBwdWs::carve(nullptr, ws, B, H, L, S, C);
}

int dr_fusion_layer_backward_f32(const dr_fusion_layer_weights* w, int C, int H, int B, int L, int S, const float* x, const float* y,
                                 const uint8_t* y_mask, const void* saved, const float* grad_out, float* grad_x, float* grad_y,
                                 const dr_fusion_layer_grads* gw, void* workspace, size_t workspace_bytes, void* stream) {
    if (!w || !gw || !x || !y || !saved || !grad_out || !grad_x || !grad_y || !fusion_args_ok(C, H, B, L, S)) return DR_EINVAL;
    if (!workspace || workspace_bytes < dr_fusion_layer_backward_workspace_bytes(B, H, L, S, C)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int R = B * L, Q = B * S, d = C / H, R4 = up4(R), Q4 = up4(Q), C2 = 2 * C, nR = nblk(R), nQ = nblk(Q);
    FSaved sv;
    FSaved::carve(const_cast<void*>(saved), sv, R, Q, C);
    FBwdWs ws;
    FBwdWs::carve(workspace, ws, B, H, L, S, C);
    const size_t pRC = (size_t)nR * C;
    int rc;
    // ---- everything that only needs the forward's tensors is transposed first, in one launch
    Transposer T;
    T.add(w->squeeze_w, C, C2, C2, ws.TWs, C);         // Ws [C, 2C] -> [2C, C]
    T.add(w->expand_w, C2, C, C, ws.TWe, C2);          // We [2C, C] -> [C, 2C]
    T.add(w->lin_w, C, C, C, ws.TWl, C);
    T.add(w->q_w, C, C, C, ws.TWq, C);
    T.add(w->k_w, C, C, C, ws.TWkv, C2, C);            // [Wk^T | Wv^T]: row j = (Wk[:, j], Wv[:, j])
    T.add(w->v_w, C, C, C, ws.TWkv + C, C2, C);
    T.add(sv.e, R, C2, C2, ws.T_e, R4);
    T.add(sv.z, R, C, C, ws.T_z, R4);
    T.add(sv.o, R, C, C, ws.T_o, R4);
    T.add(x, R, C, C, ws.T_x, R4);
    if (y == x && Q == R) ws.T_y = ws.T_x;             // a self-attention call: y^T is x^T
    else T.add(y, Q, C, C, ws.T_y, Q4);
    if ((rc = T.launch(st))) return rc;
    // ---- LN2 -> squeeze -> ReLU -> expand
    if ((rc = launch_postln_bwd(R, C, sv.f, w->norm2_w, sv.st2, grad_out, nullptr, ws.g_f, ws.p_ln2, ws.p_ln2 + pRC, ws.p_ln2 + 2 * pRC, st))) return rc;
    Gemms G;
    G.add(ws.g_f, C, ws.TWs, ws.g_e, C2, R, C2, C);                                        // g_f Ws
    if ((rc = G.launch(st))) return rc;
    ColSums cs;
    cs.add(ws.g_e, R, C2, ws.p_exp, sv.e, ws.g_e);                                                              // ReLU backward + expand's bias
    if ((rc = cs.launch(st))) return rc;
    T.add(ws.g_f, R, C, C, ws.T_gf, R4);
    T.add(ws.g_e, R, C2, C2, ws.T_ge, R4);
    if ((rc = T.launch(st))) return rc;
    G.add(ws.g_e, C2, ws.TWe, ws.g_z, C, R, C, C2);                                        // g_e We
    G.add(ws.T_gf, R4, ws.T_e, gw->squeeze_w, C2, C, C2, R4);                              // g_f^T e
    G.add(ws.T_ge, R4, ws.T_z, gw->expand_w, C, C2, C, R4);                                // g_e^T z
    if ((rc = G.launch(st))) return rc;
    // ---- LN1 (its upstream: the feed-forward branch + the residual g_f) -> linear
    if ((rc = launch_postln_bwd(R, C, sv.a, w->norm1_w, sv.st1, ws.g_z, ws.g_f, ws.g_a, ws.p_ln1, ws.p_ln1 + pRC, ws.p_ln1 + 2 * pRC, st))) return rc;
    T.add(ws.g_a, R, C, C, ws.T_ga, R4);
    if ((rc = T.launch(st))) return rc;
    G.add(ws.g_a, C, ws.TWl, ws.g_o, C, R, C, C);
    G.add(ws.T_ga, R4, ws.T_o, gw->lin_w, C, C, C, R4);
    if ((rc = G.launch(st))) return rc;
    // ---- attention -> q | k | v projections
    const uint8_t* qm = y_mask ? sv.ones : nullptr;
    rc = dr_attention_backward_f32(B, H, L, S, d, sv.q, sv.k, sv.v, sv.o, ws.g_o, C, qm, y_mask, 1.0f / sqrtf((float)d), ws.g_q, ws.g_k, ws.g_v, ws.att_ws,
                                   ws.att_wsb, stream);
    if (rc) return rc;
    cs.add(ws.g_q, R, C, ws.p_q);
    cs.add(ws.g_k, Q, C, ws.p_k);
    cs.add(ws.g_v, Q, C, ws.p_v);
    if ((rc = cs.launch(st))) return rc;
    T.add(ws.g_q, R, C, C, ws.T_gq, R4);
    T.add(ws.g_k, Q, C, C, ws.T_gk, Q4);
    T.add(ws.g_v, Q, C, C, ws.T_gv, Q4);
    if ((rc = T.launch(st))) return rc;
    G.add(ws.g_q, C, ws.TWq, grad_x, C, R, C, C, EPI_NONE, ws.g_a);                        // g_q Wq + the residual
    G.add(ws.g_k, C, ws.g_v, C, C, ws.TWkv, grad_y, C, Q, C, C2);                          // g_k Wk + g_v Wv
    G.add(ws.T_gq, R4, ws.T_x, gw->q_w, C, C, C, R4);
    G.add(ws.T_gk, Q4, ws.T_y, gw->k_w, C, C, C, Q4);
    if ((rc = G.launch(st))) return rc;
    G.add(ws.T_gv, Q4, ws.T_y, gw->v_w, C, C, C, Q4);
    if ((rc = G.launch(st))) return rc;
    // ---- the ten vector gradients from their partials
    FinBatch fb;
    memset(&fb, 0, sizeof(fb));
    int tiles = 0;
    auto fin = [&](const float* part, int nb, int n, float* out) {
        FinTarget& t = fb.t[fb.n++];
        t.part = part; t.out = out; t.nblk = nb; t.n = n; t.tile0 = tiles;
        tiles += (n + 255) / 256;
    };
    fin(ws.p_q, nR, C, gw->q_b); fin(ws.p_k, nQ, C, gw->k_b); fin(ws.p_v, nQ, C, gw->v_b);
    fin(ws.p_ln1 + 2 * pRC, nR, C, gw->lin_b); fin(ws.p_ln1, nR, C, gw->norm1_w); fin(ws.p_ln1 + pRC, nR, C, gw->norm1_b);
    fin(ws.p_exp, nR, C2, gw->expand_b); fin(ws.p_ln2 + 2 * pRC, nR, C, gw->squeeze_b); fin(ws.p_ln2, nR, C, gw->norm2_w); fin(ws.p_ln2 + pRC, nR, C, gw->norm2_b);
    hipLaunchKernelGGL(colsum_final_kernel, dim3(tiles), dim3(256), 0, st, fb);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
