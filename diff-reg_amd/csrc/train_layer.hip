// train_layer.hip -- GeometryAttentionLayer (3D/models/transformero.py:43-96) for TRAINING as two entry points: the forward that keeps what its
// backward needs, and the whole backward -- every kernel of it launched from here.  Round 4 drove the same kernels one by one from Python
// (diffreg_hip/autograd.py: ~20 calls forward, ~55 backward per layer call, 20 layer calls per step); a training step was ~12 ms of kernels inside
// 28 ms of host time.  Nothing new is computed here: the projections and their gradients run on the library's f32-input MFMA GEMM (launch_gemm),
// the attention on dr_attention_f32 / dr_attention_backward_f32 (flash-style, no [B,H,L,S] matrix), LayerNorm / ReLU / rotary on the kernels of
// train.hip.  New kernels: a batched transposition (the GEMM contracts along contiguous k: x W for a gradient w.r.t. the input and g^T x for a weight
// gradient need the transposed operand) and a two-operand add, both in train_common.h.
#include <string.h>
#include "train_common.h"

namespace dr {
namespace {

// what the forward keeps (floats): q, k (rotary applied), v, the heads' output o, merge(o) before norm1, norm1's output m, the hidden
// activation h, mlp.2(h) before norm2, and the two LayerNorms' (mean, rstd) rows
struct Saved {
    float *qw, *kw, *vw, *o, *m_pre, *m, *h, *f_pre, *st1, *st2;
    static size_t carve(void* buf, Saved& s, size_t R, size_t Q, int C) {
        Carver c(buf);
        s.qw = c.take<float>(R * C); s.kw = c.take<float>(Q * C); s.vw = c.take<float>(Q * C); s.o = c.take<float>(R * C); s.m_pre = c.take<float>(R * C); s.m = c.take<float>(R * C);
        s.h = c.take<float>(R * 2 * C); s.f_pre = c.take<float>(R * C); s.st1 = c.take<float>(2 * R); s.st2 = c.take<float>(2 * R);
        return c.off + 256;
    }
};

// the backward's workspace (floats): activation gradients, the transposed weights ([Wk^T | Wv^T] side by side), the transposed activations and
// gradients (token count padded to a multiple of 4: the GEMM's k extent), the LayerNorm and attention backwards' own workspaces
struct BwdWs {
    float *g_fpre, *g_h, *g_x1, *g_m, *g_mpre, *g_o, *g_qw, *g_kw, *g_vw, *g_qpre, *g_kpre;
    float *TW2, *TW0, *TWm, *TWq, *TWkv;
    float *T_gf, *T_h, *T_gh, *T_cat, *T_gm, *T_o, *T_gq, *T_gk, *T_gv, *T_y;
    float *ln_ws, *att_ws;
    size_t att_wsb;
    static size_t carve(void* buf, BwdWs& s, int B, int H, int L, int S, size_t C) {
        const size_t R = (size_t)B * L, Q = (size_t)B * S, R4 = up4((int)R), Q4 = up4((int)Q), C2 = 2 * C;
        Carver c(buf);
        s.g_fpre = c.take<float>(R * C); s.g_h = c.take<float>(R * C2); s.g_x1 = c.take<float>(R * C); s.g_m = c.take<float>(R * C);
        s.g_mpre = c.take<float>(R * C); s.g_o = c.take<float>(R * C);
        s.g_qw = c.take<float>(R * C); s.g_kw = c.take<float>(Q * C); s.g_vw = c.take<float>(Q * C); s.g_qpre = c.take<float>(R * C); s.g_kpre = c.take<float>(Q * C);
        s.TW2 = c.take<float>(C2 * C); s.TW0 = c.take<float>(C2 * C2); s.TWm = c.take<float>(C * C); s.TWq = c.take<float>(C * C); s.TWkv = c.take<float>(C * C2);
        s.T_gf = c.take<float>(C * R4); s.T_h = c.take<float>(C2 * R4); s.T_gh = c.take<float>(C2 * R4); s.T_cat = c.take<float>(C2 * R4);
        s.T_gm = c.take<float>(C * R4); s.T_o = c.take<float>(C * R4); s.T_gq = c.take<float>(C * R4);
        s.T_gk = c.take<float>(C * Q4); s.T_gv = c.take<float>(C * Q4); s.T_y = c.take<float>(C * Q4);
        s.ln_ws = c.take<float>(dr_layernorm_backward_workspace_bytes((int)C) / sizeof(float));
        s.att_wsb = dr_attention_backward_workspace_bytes(B, H, L);
        s.att_ws = c.take<float>(s.att_wsb / sizeof(float) + 64);
        return c.off + 256;
    }
};

}  // namespace
}  // namespace dr

using namespace dr;

extern "C" {

size_t dr_attention_layer_train_saved_bytes(int B, int L, int S, int C) {
    if (B < 1 || L < 1 || S < 1 || C < 4) return 0;
    Saved s;
    return Saved::carve(nullptr, s, (size_t)B * L, (size_t)B * S, C);
}

int dr_attention_layer_train_forward_f32(const dr_layer_weights* w, int C, int H, int B, int L, int S, const float* x, const float* y,
                                         const float* cos_x, const float* sin_x, const float* cos_y, const float* sin_y,
                                         const uint8_t* x_mask, const uint8_t* y_mask, float* out, void* saved, size_t saved_bytes, void* stream) {
    if (!w || !x || !y || !cos_x || !sin_x || !cos_y || !sin_y || !out || !saved || B < 1 || L < 1 || S < 1 || C % H || (C / H) % 4 || C % 4) return DR_EINVAL;
    if ((x_mask == nullptr) != (y_mask == nullptr)) return DR_EINVAL;
    if (saved_bytes < dr_attention_layer_train_saved_bytes(B, L, S, C)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int R = B * L, Q = B * S, d = C / H;
    Saved sv;
    Saved::carve(saved, sv, R, Q, C);
    Gemms G;
    // q | k | v: one launch; the rotary code in the GEMM's epilogue (transformero.py:61-70)
    GemmProblem& pq = G.add(x, C, w->q_proj, sv.qw, C, R, C, C, EPI_ROTARY);
    pq.cosT = cos_x; pq.sinT = sin_x; pq.rot_C = C;
    GemmProblem& pk = G.add(y, C, w->k_proj, sv.kw, C, Q, C, C, EPI_ROTARY);
    pk.cosT = cos_y; pk.sinT = sin_y; pk.rot_C = C;
    G.add(y, C, w->v_proj, sv.vw, C, Q, C, C);
    int rc = G.launch(st);
    if (rc) return rc;
    rc = dr_attention_f32(B, H, L, S, d, sv.qw, sv.kw, sv.vw, C, x_mask, y_mask, 1.0f / sqrtf((float)d), sv.o, stream);
    if (rc) return rc;
    G.add(sv.o, C, w->merge, sv.m_pre, C, R, C, C);
    rc = G.launch(st);
    if (rc) return rc;
    rc = dr_layernorm_f32(R, C, sv.m_pre, w->norm1_w, w->norm1_b, 1e-5f, sv.m, sv.st1, stream);
    if (rc) return rc;
    G.add(x, C, sv.m, C, C, w->mlp0, sv.h, 2 * C, R, 2 * C, 2 * C, EPI_RELU);      // mlp.0(cat[x, message]) + ReLU
    rc = G.launch(st);
    if (rc) return rc;
    G.add(sv.h, 2 * C, w->mlp2, sv.f_pre, C, R, C, 2 * C);
    rc = G.launch(st);
    if (rc) return rc;
    // out = x + norm2(.)  (norm2's output is not needed again: it lands in `out` and the residual is added in place)
    rc = dr_layernorm_f32(R, C, sv.f_pre, w->norm2_w, w->norm2_b, 1e-5f, out, sv.st2, stream);
    if (rc) return rc;
    const long long n4 = (long long)R * C / 4;
    hipLaunchKernelGGL(add2_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, n4, (const float4*)out, (const float4*)x, (float4*)out);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_attention_layer_backward_workspace_bytes(int B, int H, int L, int S, int C) {
    if (B < 1 || L < 1 || S < 1 || C < 4 || H < 1) return 0;
    BwdWs ws;
    return BwdWs::carve(nullptr, ws, B, H, L, S, C);
}

int dr_attention_layer_backward_f32(const dr_layer_weights* w, int C, int H, int B, int L, int S, const float* x, const float* y,
                                    const float* cos_x, const float* sin_x, const float* cos_y, const float* sin_y, const uint8_t* x_mask,
                                    const uint8_t* y_mask, const void* saved, const float* grad_out, float* grad_x, float* grad_y,
                                    const dr_layer_grads* gw, void* workspace, size_t workspace_bytes, void* stream) {
    if (!w || !gw || !x || !y || !cos_x || !sin_x || !cos_y || !sin_y || !saved || !grad_out || !grad_x || !grad_y || B < 1 || L < 1 || S < 1 ||
        C % H || (C / H) % 4 || C % 4)
        return DR_EINVAL;
    if ((x_mask == nullptr) != (y_mask == nullptr)) return DR_EINVAL;
    if (!workspace || workspace_bytes < dr_attention_layer_backward_workspace_bytes(B, H, L, S, C)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int R = B * L, Q = B * S, d = C / H, R4 = up4(R), Q4 = up4(Q), C2 = 2 * C;
    Saved sv;
    Saved::carve(const_cast<void*>(saved), sv, R, Q, C);
    BwdWs ws;
    BwdWs::carve(workspace, ws, B, H, L, S, C);
    int rc;
    // ---- everything that only needs the forward's tensors is transposed first, in one launch
    Transposer T;
    T.add(w->mlp2, C, C2, C2, ws.TW2, C);              // W2 [C, 2C]  -> [2C, C]
    T.add(w->mlp0, C2, C2, C2, ws.TW0, C2);            // W0 [2C, 2C] -> its transpose
    T.add(w->merge, C, C, C, ws.TWm, C);
    T.add(w->q_proj, C, C, C, ws.TWq, C);
    T.add(w->k_proj, C, C, C, ws.TWkv, C2, C);         // [Wk^T | Wv^T]: row j = (Wk[:, j], Wv[:, j])
    T.add(w->v_proj, C, C, C, ws.TWkv + C, C2, C);
    T.add(sv.h, R, C2, C2, ws.T_h, R4);
    T.add(x, R, C, C, ws.T_cat, R4);                   // cat[x, m]^T = [x^T ; m^T]
    T.add(sv.m, R, C, C, ws.T_cat + (size_t)C * R4, R4);
    T.add(sv.o, R, C, C, ws.T_o, R4);
    // self-attention calls (y is x): y^T is x^T, already the first C rows of cat^T
    const bool y_is_x = y == x && Q == R;
    if (y_is_x) ws.T_y = ws.T_cat;
    else T.add(y, Q, C, C, ws.T_y, Q4);
    rc = T.launch(st);
    if (rc) return rc;
    // ---- norm2 -> mlp.2 -> ReLU -> mlp.0
    rc = dr_layernorm_backward_f32(R, C, sv.f_pre, w->norm2_w, sv.st2, grad_out, ws.g_fpre, gw->norm2_w, gw->norm2_b, ws.ln_ws, stream);
    if (rc) return rc;
    Gemms G;
    G.add(ws.g_fpre, C, ws.TW2, ws.g_h, C2, R, C2, C);                                     // g W2
    rc = G.launch(st);
    if (rc) return rc;
    rc = dr_relu_backward_f32((long long)R * C2, sv.h, ws.g_h, ws.g_h, stream);
    if (rc) return rc;
    T.add(ws.g_fpre, R, C, C, ws.T_gf, R4);
    T.add(ws.g_h, R, C2, C2, ws.T_gh, R4);
    rc = T.launch(st);
    if (rc) return rc;
    G.add(ws.g_h, C2, ws.TW0, ws.g_x1, C, R, C, C2, EPI_NONE, grad_out);                   // grad_out + (g_h W0)[:, :C]   (the residual + cat's x half)
    G.add(ws.g_h, C2, ws.TW0 + (size_t)C * C2, ws.g_m, C, R, C, C2);                       // (g_h W0)[:, C:]  -> norm1's output
    G.add(ws.T_gf, R4, ws.T_h, gw->mlp2, C2, C, C2, R4);                                      // g^T h
    G.add(ws.T_gh, R4, ws.T_cat, gw->mlp0, C2, C2, C2, R4);                                   // g_h^T cat[x, m]
    rc = G.launch(st);
    if (rc) return rc;
    // ---- norm1 -> merge
    rc = dr_layernorm_backward_f32(R, C, sv.m_pre, w->norm1_w, sv.st1, ws.g_m, ws.g_mpre, gw->norm1_w, gw->norm1_b, ws.ln_ws, stream);
    if (rc) return rc;
    T.add(ws.g_mpre, R, C, C, ws.T_gm, R4);
    rc = T.launch(st);
    if (rc) return rc;
    G.add(ws.g_mpre, C, ws.TWm, ws.g_o, C, R, C, C);
    G.add(ws.T_gm, R4, ws.T_o, gw->merge, C, C, C, R4);
    rc = G.launch(st);
    if (rc) return rc;
    // ---- attention, rotary code, projections
    rc = dr_attention_backward_f32(B, H, L, S, d, sv.qw, sv.kw, sv.vw, sv.o, ws.g_o, C, x_mask, y_mask, 1.0f / sqrtf((float)d), ws.g_qw, ws.g_kw, ws.g_vw,
                                   ws.att_ws, ws.att_wsb, stream);
    if (rc) return rc;
    rc = dr_rotary_f32(R, C, ws.g_qw, cos_x, sin_x, 1, 1.f, ws.g_qpre, stream);
    if (rc) return rc;
    rc = dr_rotary_f32(Q, C, ws.g_kw, cos_y, sin_y, 1, 1.f, ws.g_kpre, stream);
    if (rc) return rc;
    T.add(ws.g_qpre, R, C, C, ws.T_gq, R4);
    T.add(ws.g_kpre, Q, C, C, ws.T_gk, Q4);
    T.add(ws.g_vw, Q, C, C, ws.T_gv, Q4);
    rc = T.launch(st);
    if (rc) return rc;
    G.add(ws.g_qpre, C, ws.TWq, grad_x, C, R, C, C, EPI_NONE, ws.g_x1);                    // + the residual / mlp part
    G.add(ws.g_kpre, C, ws.g_vw, C, C, ws.TWkv, grad_y, C, Q, C, C2);                      // g_k Wk + g_v Wv
    rc = G.launch(st);
    if (rc) return rc;
    G.add(ws.T_gq, R4, ws.T_cat, gw->q_proj, C, C, C, R4);                                    // g_q^T x   (x^T = the first C rows of cat^T)
    G.add(ws.T_gk, Q4, ws.T_y, gw->k_proj, C, C, C, Q4);
    G.add(ws.T_gv, Q4, ws.T_y, gw->v_proj, C, C, C, Q4);
    return G.launch(st);
}

}  // extern "C"
