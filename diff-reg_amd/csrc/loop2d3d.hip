// loop2d3d.hip -- orchestration of the 2D-3D variant: CrossModalFusionModule denoiser,
// position-free matching head, reverse sampling of MATR2D3D.forward.  Same kernels as loop.hip
// (GEMM with bias / addend epilogues, attention with d_head = 64, post-LN LayerNorm, Sinkhorn,
// Procrustes, DDIM), enqueued on one stream without host synchronisation.  The steps are reverse_sampling() of loop_common.h, shared
// with loop.hip.
//
// Token layout: image patches of all P pairs (pair p at row p*M), then point nodes (P*M + p*N).
// In the terms of loop_common.h's Sides: side A = image patches (M rows per pair), side B = point nodes (N rows per pair).
//
// Round 4: calls of >= 4096 token rows (two cfg5 pairs or more) run the layer on fp16 hi / lo plane images (pgemm.h) like
// dr_denoise_loop: the biased q | k | v projections write the attention kernel's operand images, attention_planes_kernel (d = 64)
// writes the output projection's operand, z = LayerNorm(linear(h) + x) and out = LayerNorm(z + squeeze(relu(expand(z)))) are
// epilogue modes of the plane GEMM (bias, post-add LayerNorm, 256-column geometry) -- five launches per layer call instead of
// eight, no fp32 round trip of q / k / v / h / hidden.  The image half of layer 0 (a self layer on step-invariant tokens) is
// evaluated once per call.
#include "loop_common.h"

namespace dr {

// ---- plane path ---------------------------------------------------------------------------------------------------------------
struct P2Layer {
    PgW qkv, lin, expand, squeeze;          // q | k | v: 3 blocks of C rows; expand: 2 blocks
    const float *qkv_b;                     // [3 C] the three biases back to back (a PgProblem's bias is indexed nb * C + col)
    const float *qkv_bmax, *lin_bmax, *exp_bmax, *sq_bmax;   // [3] / [1] / [2] / [1]
    const float *lnB1, *lnB2;
};
struct Prepack2 {
    static constexpr int MAXL = 16;
    P2Layer L[MAXL];
    PgW out, head;
    const float* out_bmax;
    static bool supported(const dr_loop2d3d_config& cfg) {
        if (cfg.n_layers > MAXL || cfg.C % cfg.H) return false;
        const int d = cfg.C / cfg.H;
        // heads start at a k-chunk without padding (d = 64): biases and images then share the nn.Linear's column order
        return pgemm_shape_ok(cfg.C) && (d == 64 || d == 112 || d == 144) && cfg.C / 16 >= 4;
    }
    static size_t carve(void* buf, const dr_loop2d3d_config& cfg, Prepack2* pp) {
        Carver c(buf);
        const int C = cfg.C, nC = C / 16;
        for (int l = 0; l < cfg.n_layers; ++l) {
            P2Layer* L = pp ? &pp->L[l] : nullptr;
            take_weight(c, C, 3, nC, L ? &L->qkv : nullptr);
            take_weight(c, C, 1, nC, L ? &L->lin : nullptr);
            take_weight(c, C, 2, nC, L ? &L->expand : nullptr);
            take_weight(c, C, 1, 2 * nC, L ? &L->squeeze : nullptr);
            float* b = c.take<float>(3 * (size_t)C + 16);
            if (L && buf) {
                L->qkv_b = b; L->qkv_bmax = b + 3 * C; L->lin_bmax = b + 3 * C + 3; L->exp_bmax = b + 3 * C + 4; L->sq_bmax = b + 3 * C + 6;
                L->lnB1 = b + 3 * C + 7; L->lnB2 = b + 3 * C + 8;
            }
        }
        take_weight(c, C, 1, nC, pp ? &pp->out : nullptr);
        take_weight(c, C, 1, nC, pp ? &pp->head : nullptr);
        float* ob = c.take<float>(4);
        if (pp && buf) pp->out_bmax = ob;
        return c.off + 256;
    }
    static int fill(void* buf, const dr_loop2d3d_config& cfg, const dr_fusion_weights& W, hipStream_t st) {
        Prepack2 pp;
        carve(buf, cfg, &pp);
        const int C = cfg.C;
        for (int l = 0; l < cfg.n_layers; ++l) {
            const dr_fusion_layer_weights& w = W.layers[l];
            const P2Layer& L = pp.L[l];
            int rc = pgemm_pack_weights_block(w.q_w, C, C, C, C, L.qkv, 0, st);
            if (rc == DR_OK) rc = pgemm_pack_weights_block(w.k_w, C, C, C, C, L.qkv, 1, st);
            if (rc == DR_OK) rc = pgemm_pack_weights_block(w.v_w, C, C, C, C, L.qkv, 2, st);
            if (rc == DR_OK) rc = pgemm_pack_weights_block(w.lin_w, C, C, C, C, L.lin, 0, st);
            if (rc == DR_OK) rc = pgemm_pack_weights_block(w.expand_w, C, C, C, C, L.expand, 0, st);
            if (rc == DR_OK) rc = pgemm_pack_weights_block(w.expand_w + (size_t)C * C, C, C, C, C, L.expand, 1, st);
            if (rc == DR_OK) rc = pgemm_pack_weights_block(w.squeeze_w, C, 2 * C, 2 * C, 2 * C, L.squeeze, 0, st);
            if (rc) return rc;
            float* qb = const_cast<float*>(L.qkv_b);
            DR_HIP_CHECK(hipMemcpyAsync(qb, w.q_b, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
            DR_HIP_CHECK(hipMemcpyAsync(qb + C, w.k_b, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
            DR_HIP_CHECK(hipMemcpyAsync(qb + 2 * C, w.v_b, (size_t)C * 4, hipMemcpyDeviceToDevice, st));
            rc = launch_absmax_blocks(qb, 3, C, const_cast<float*>(L.qkv_bmax), st);
            if (rc == DR_OK) rc = launch_absmax_blocks(w.lin_b, 1, C, const_cast<float*>(L.lin_bmax), st);
            if (rc == DR_OK) rc = launch_absmax_blocks(w.expand_b, 2, C, const_cast<float*>(L.exp_bmax), st);
            if (rc == DR_OK) rc = launch_absmax_blocks(w.squeeze_b, 1, C, const_cast<float*>(L.sq_bmax), st);
            if (rc == DR_OK) rc = launch_ln_bound(w.norm1_w, w.norm1_b, C, const_cast<float*>(L.lnB1), st);
            if (rc == DR_OK) rc = launch_ln_bound(w.norm2_w, w.norm2_b, C, const_cast<float*>(L.lnB2), st);
            if (rc) return rc;
        }
        int rc = pgemm_pack_weights_block(W.out_w, C, C, C, C, pp.out, 0, st);
        if (rc == DR_OK) rc = pgemm_pack_weights_block(W.src_proj, C, C, C, C, pp.head, 0, st);
        if (rc == DR_OK) rc = launch_absmax_blocks(W.out_b, 1, C, const_cast<float*>(pp.out_bmax), st);
        return rc;
    }
};

struct Planes2 {
    bool on;
    Tok tok0, ta, tb, l0, z;
    char *qkv_img, *att_img, *hid_img, *feat_img;
    float *qkv_bnd, *att_bnd, *hid_bnd, *feat_bnd, *grp_x;
    size_t qkv_stride, side_C, side_hid;    // bytes from the q image to the k image; offset of the point part in an image of K = C / 2C
    void* own_pack;
    static size_t img_bytes(int PM, int PN, int K) { return plane_image_bytes(PM, K) + plane_image_bytes(PN, K); }
    static void carve(Carver& c, Planes2& w, const dr_loop2d3d_config& cfg, int P, int N, int M) {
        const int C = cfg.C, PM = P * M, PN = P * N, T = PM + PN;
        w.on = planes_wanted(cfg.flags, Prepack2::supported(cfg), T);
        if (!w.on) return;
        w.side_C = plane_image_bytes(PM, C); w.side_hid = plane_image_bytes(PM, 2 * C);
        Tok* toks[5] = {&w.tok0, &w.ta, &w.tb, &w.l0, &w.z};
        for (Tok* t : toks) { t->f32 = nullptr; t->img = c.take<char>(img_bytes(PM, PN, C)); t->bnd = c.take<float>(T); }
        w.l0.f32 = c.take<float>((size_t)T * C);
        w.qkv_stride = (img_bytes(PM, PN, C) + 255) & ~(size_t)255;
        w.qkv_img = c.take<char>(3 * w.qkv_stride); w.qkv_bnd = c.take<float>(3 * (size_t)T);
        w.att_img = c.take<char>(img_bytes(PM, PN, C)); w.att_bnd = c.take<float>(T);
        w.hid_img = c.take<char>(img_bytes(PM, PN, 2 * C)); w.hid_bnd = c.take<float>(T);
        w.feat_img = c.take<char>(img_bytes(PM, PN, C)); w.feat_bnd = c.take<float>(T);
        w.grp_x = c.take<float>(2 * (size_t)P);
        w.own_pack = c.take<char>(Prepack2::carve(nullptr, cfg, nullptr));
    }
};

struct F2Ws {
    float *tok0, *ta, *tb, *qkv, *att, *lin, *z, *hid, *f, *feat, *proj, *sim, *x0, *wconf, *cat, *emb2, *emb3, *warped;
    float *R, *t, *Rf, *tf;
    double *x, *cond;
    int* ok;
    void* skws; size_t skws_bytes;
    void* pws; size_t pws_bytes;
    Planes2 pl;
    unsigned* status;                        // the call's own sticky status word (dr_denoise_loop_status): zeroed when a call starts
    static size_t carve(Carver& c, F2Ws& w, const dr_loop2d3d_config& cfg, int P, int N, int M) {
        const size_t T = (size_t)P * (N + M), C = cfg.C, NM = (size_t)P * N * M, PM = (size_t)P * M, PN = (size_t)P * N;
        w.status = c.take<unsigned>(4);      // (first, as in the 3D / 4D loop's workspace: dr_denoise_loop_status reads either)
        w.tok0 = c.take<float>(T * C); w.ta = c.take<float>(T * C); w.tb = c.take<float>(T * C);
        w.qkv = c.take<float>(T * 3 * C); w.att = c.take<float>(T * C); w.lin = c.take<float>(T * C);
        w.z = c.take<float>(T * C); w.hid = c.take<float>(T * 2 * C); w.f = c.take<float>(T * C);
        w.feat = c.take<float>(T * C); w.proj = c.take<float>(T * C);
        w.sim = c.take<float>(NM); w.x0 = c.take<float>(NM); w.wconf = c.take<float>(NM);
        w.cat = c.take<float>(PM * 2 * C); w.emb2 = c.take<float>(PM * 44); w.emb3 = c.take<float>(PN * 64);
        w.warped = c.take<float>(PN * 3);
        w.R = c.take<float>((size_t)P * 9); w.t = c.take<float>((size_t)P * 3);
        w.Rf = c.take<float>((size_t)P * 9); w.tf = c.take<float>((size_t)P * 3);
        w.x = c.take<double>(NM); w.cond = c.take<double>(P); w.ok = c.take<int>(P);
        sampler_scratch(c, P, N, M, cfg.flags, w.skws, w.skws_bytes, w.pws, w.pws_bytes);
        Planes2::carve(c, w.pl, cfg, P, N, M);
        if (w.pl.on) { w.pl.tok0.f32 = w.tok0; w.pl.ta.f32 = w.ta; w.pl.tb.f32 = w.tb; w.pl.z.f32 = w.z; }
        return c.off + 256;
    }
};

// one vision3d TransformerLayer: x rows [xr0, +xrows) of xin attend y rows [yr0, +yrows) of yin
static int fusion_layer(const dr_fusion_layer_weights& W, int C, int H, int P, const float* xin, int xr0, int xrows, const float* yin, int yr0,
                        int yrows, const Family& f1, const Family* f2, const F2Ws& ws, float* out, hipStream_t st) {
    GemmBatch g;
    memset(&g, 0, sizeof(g));
    auto proj = [&](GemmProblem& p, const float* in, int r0, int rows, const float* Wm, const float* b, int coloff) {
        p.A = in + (size_t)r0 * C; p.W = Wm; p.bias = b; p.out = ws.qkv + (size_t)r0 * 3 * C + coloff;
        p.rows = rows; p.ncols = C; p.K = C; p.K1 = C; p.lda = C; p.ldo = 3 * C; p.epi = EPI_NONE; p.scale = 1.f;
    };
    proj(g.p[0], xin, xr0, xrows, W.q_w, W.q_b, 0);
    proj(g.p[1], yin, yr0, yrows, W.k_w, W.k_b, C);
    proj(g.p[2], yin, yr0, yrows, W.v_w, W.v_b, 2 * C);
    g.n = 3;
    int rc = launch_gemm(g, st);
    if (rc) return rc;
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.q = ws.qkv; a.k = ws.qkv + C; a.v = ws.qkv + 2 * C; a.out = ws.att;
    a.ldq = a.ldk = a.ldv = 3 * C; a.ldo = C; a.H = H; a.d = C / H;
    attn_families(a, P, f1, f2);
    a.scale = 1.0f / sqrtf((float)(C / H));
    rc = launch_attention(a, st);
    if (rc) return rc;
    // z = norm(linear(h) + x)
    rc = gemm1(ws.att + (size_t)xr0 * C, C, W.lin_w, W.lin_b, ws.lin + (size_t)xr0 * C, C, xrows, C, C, EPI_NONE, 1.f, nullptr, st);
    if (rc) return rc;
    rc = launch_layernorm_postadd(ws.lin + (size_t)xr0 * C, C, W.norm1_w, W.norm1_b, xin + (size_t)xr0 * C, C, ws.z + (size_t)xr0 * C, C, xrows, C, st);
    if (rc) return rc;
    // out = norm(z + squeeze(relu(expand(z))))
    rc = gemm1(ws.z + (size_t)xr0 * C, C, W.expand_w, W.expand_b, ws.hid + (size_t)xr0 * 2 * C, 2 * C, xrows, 2 * C, C, EPI_RELU, 1.f, nullptr, st);
    if (rc) return rc;
    rc = gemm1(ws.hid + (size_t)xr0 * 2 * C, 2 * C, W.squeeze_w, W.squeeze_b, ws.f + (size_t)xr0 * C, C, xrows, C, 2 * C, EPI_NONE, 1.f, nullptr, st);
    if (rc) return rc;
    return launch_layernorm_postadd(ws.f + (size_t)xr0 * C, C, W.norm2_w, W.norm2_b, ws.z + (size_t)xr0 * C, C, out + (size_t)xr0 * C, C, xrows, C, st);
}

// ---- one vision3d TransformerLayer call on plane images: five launches ---------------------------------------------------------
using P2Ctx = PlaneCtx<Prepack2, Planes2>;
// x rows of side(s) xs of `xin` attend the rows of side(s) ys of `yin`; out gets the x sides (fp32 rows + image + bounds)
static int fusion_layer_planes(const P2Ctx& X, const dr_fusion_layer_weights& W, int l, const Tok& xin, int xs, const Tok& yin, int ys,
                               const Tok& out, const Family& f1, const Family* f2, hipStream_t st) {
    const Sides& S = X.S;
    const int C = X.C, H = X.H, PM = S.rows_a, T = S.rows(SIDE_BOTH), nC = C / 16, d = C / H;
    const P2Layer& L = X.pp->L[l];
    const Planes2& pw = *X.pw;
    PgBatch g;
    auto reset = [&]() { memset(&g, 0, sizeof(g)); };
    auto add = [&]() -> PgProblem& { return g.p[g.n++]; };
    // bound of the keys' source rows per group (pair x side): all keys of a group share one scale in the k and v images
    // (taken inside the projection's kernel when a group is a whole number of workgroups: pgemm.h)
    const bool grp_inline = S.La % 128 == 0 && S.Lb % 128 == 0 && env_knob("DR_LOOP_GRP_INLINE", 1) != 0;
    int rc = grp_inline ? DR_OK : side_group_max(S, ys, yin.bnd, pw.grp_x, st);
    if (rc) return rc;
    // ---- q | k | v = x W^T + b -> three plane images (head h at k = h d), no rotary (vision3d/layers/transformer.py:96-104)
    auto proj = [&](const Tok& tin, int side, int b0, int nblk, int grpm) {
        PgProblem& p = add();
        p.A0 = S.at(tin.img, pw.side_C, side); p.bnd0 = tin.bnd + S.r0(side); p.nc0 = nC;
        p.W = pgw_blocks(L.qkv, b0, C); p.nblk = nblk; p.rows = S.rows(side); p.C = C; p.k_alg = C; p.mode = PG_PLANES; p.scale = 1.f;
        p.bias = L.qkv_b + (size_t)b0 * C; p.bias_max = L.qkv_bmax + b0;
        p.pimg = S.at(pw.qkv_img + (size_t)b0 * pw.qkv_stride, pw.side_C, side); p.p_nct = nC; p.pbnd = pw.qkv_bnd + (size_t)b0 * T + S.r0(side);
        p.pimg_blk_stride = (long long)pw.qkv_stride; p.pbnd_blk_stride = T;
        p.grp_bnd = grp_inline ? nullptr : pw.grp_x; p.grp_mask = grpm; p.grp_first = S.grp_first(side); p.grp_rows = S.per_pair(side);
    };
    reset();
    if (xs == ys && xin.img == yin.img) {
        S.for_sides(xs, [&](int side) { proj(xin, side, 0, 3, 6); });
    } else {
        S.for_sides(xs, [&](int side) { proj(xin, side, 0, 1, 0); });
        S.for_sides(ys, [&](int side) { proj(yin, side, 1, 2, 3); });
    }
    rc = launch_pgemm(g, st);
    if (rc) return rc;
    // ---- attention on the images -> image of the heads' outputs
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.H = H; a.d = d;
    attn_families(a, S.P, f1, f2);
    a.scale = 1.0f / sqrtf((float)d);
    a.pimg[0] = pw.att_img; a.pimg[1] = pw.att_img + pw.side_C; a.p_split = PM; a.p_nct = nC; a.p_dp = d; a.pbnd = pw.att_bnd;
    a.qimg[0] = pw.qkv_img; a.qimg[1] = pw.qkv_img + pw.side_C;
    a.kimg[0] = pw.qkv_img + pw.qkv_stride; a.kimg[1] = a.kimg[0] + pw.side_C;
    a.vimg[0] = pw.qkv_img + 2 * pw.qkv_stride; a.vimg[1] = a.vimg[0] + pw.side_C;
    a.qbnd = pw.qkv_bnd; a.kgb = pw.qkv_bnd + T; a.vgb = pw.qkv_bnd + 2 * (size_t)T;
    a.f16_single = X.attn_f16;
    rc = launch_attention(a, st);
    if (rc) return rc;
    // ---- z = LayerNorm(linear(h) + b + x)   (transformer.py:188-196)
    reset();
    S.for_sides(xs, [&](int side) {
        PgProblem& p = add();
        p.A0 = S.at(pw.att_img, pw.side_C, side); p.bnd0 = pw.att_bnd + S.r0(side); p.nc0 = nC;
        p.W = L.lin; p.nblk = 1; p.rows = S.rows(side); p.C = C; p.k_alg = C; p.mode = PG_LN; p.bias = W.lin_b;
        p.gamma = W.norm1_w; p.beta = W.norm1_b; p.lnB = L.lnB1;
        p.resid = xin.f32 + (size_t)S.r0(side) * C; p.ldr = C; p.ln_postadd = 1;
        p.out = pw.z.f32 + (size_t)S.r0(side) * C; p.ldo = C;
        p.pimg = S.at(pw.z.img, pw.side_C, side); p.p_nct = nC; p.pbnd = pw.z.bnd + S.r0(side);
    });
    rc = launch_pgemm(g, st);
    if (rc) return rc;
    // ---- hidden = relu(expand(z) + b)   (transformer.py:262-266)
    reset();
    S.for_sides(xs, [&](int side) {
        PgProblem& p = add();
        p.A0 = S.at(pw.z.img, pw.side_C, side); p.bnd0 = pw.z.bnd + S.r0(side); p.nc0 = nC;
        p.W = L.expand; p.nblk = 2; p.rows = S.rows(side); p.C = C; p.k_alg = C; p.mode = PG_PLANES; p.relu = 1; p.scale = 1.f;
        p.bias = W.expand_b; p.bias_max = L.exp_bmax;
        p.pimg = S.at(pw.hid_img, pw.side_hid, side); p.p_nct = 2 * nC; p.pbnd = pw.hid_bnd + S.r0(side);
    });
    rc = launch_pgemm(g, st);
    if (rc) return rc;
    // ---- out = LayerNorm(z + squeeze(hidden) + b)   (transformer.py:267-271)
    reset();
    S.for_sides(xs, [&](int side) {
        PgProblem& p = add();
        p.A0 = S.at(pw.hid_img, pw.side_hid, side); p.bnd0 = pw.hid_bnd + S.r0(side); p.nc0 = 2 * nC;
        p.W = L.squeeze; p.nblk = 1; p.rows = S.rows(side); p.C = C; p.k_alg = 2 * C; p.mode = PG_LN; p.bias = W.squeeze_b;
        p.gamma = W.norm2_w; p.beta = W.norm2_b; p.lnB = L.lnB2;
        p.resid = pw.z.f32 + (size_t)S.r0(side) * C; p.ldr = C; p.ln_postadd = 1;
        p.out = out.f32 + (size_t)S.r0(side) * C; p.ldo = C;
        p.pimg = S.at(out.img, pw.side_C, side); p.p_nct = nC; p.pbnd = out.bnd + S.r0(side);
    });
    return launch_pgemm(g, st);
}

}  // namespace dr

using namespace dr;

extern "C" {

size_t dr_loop2d3d_prepack_bytes(const dr_loop2d3d_config* cfg) {
    if (!cfg || cfg->C < 1 || cfg->H < 1 || !Prepack2::supported(*cfg)) return 0;
    return Prepack2::carve(nullptr, *cfg, nullptr);
}

int dr_loop2d3d_prepack(const dr_loop2d3d_config* cfg, const dr_fusion_weights* w, void* packed, size_t packed_bytes, void* stream) {
    if (!cfg || !w || !w->layers || !w->out_w || !w->out_b || !w->src_proj || !packed || ((uintptr_t)packed & 255)) return DR_EINVAL;
    if (cfg->C < 1 || cfg->H < 1 || !Prepack2::supported(*cfg)) return DR_ENOSUP;
    if (packed_bytes < Prepack2::carve(nullptr, *cfg, nullptr)) return DR_EWORKSPACE;
    return Prepack2::fill(packed, *cfg, *w, (hipStream_t)stream);
}

size_t dr_denoise_loop_2d3d_workspace_bytes(const dr_loop2d3d_config* cfg, int P, int N, int M) {
    if (!cfg || P < 1 || N < 1 || M < 1) return 0;
    Carver c(nullptr);
    F2Ws w;
    return F2Ws::carve(c, w, *cfg, P, N, M);
}

int dr_denoise_loop_2d3d(const dr_loop2d3d_config* cfg, const dr_fusion_weights* w, int P, int N, int M, const float* img_feats,
                         const float* img_dino, const float* img_pixels, const float* pcd_feats, const float* s_pcd,
                         const float* t_pcd_da, const uint8_t* src_mask, const uint8_t* tgt_mask, const uint8_t* tgt_mask_da,
                         const float* x_T, double* conf, double* x_final, int64_t* matches, int32_t* match_count, float* img_out,
                         float* pcd_out, const dr_loop_trace* trace, void* workspace, size_t workspace_bytes, void* stream) {
    if (!cfg || !w || P < 1 || N < 1 || M < 1 || !w->layers || !img_feats || !img_dino || !img_pixels || !pcd_feats || !s_pcd || !conf)
        return DR_EINVAL;
    if (cfg->C % cfg->H || (cfg->C / cfg->H) % 4 || cfg->img_dim % 4 || cfg->dino_dim % 4 || cfg->pcd_dim % 4 || cfg->steps < 0)
        return DR_EINVAL;
    const bool masked = src_mask != nullptr;
    if (masked != (tgt_mask != nullptr) || masked != (tgt_mask_da != nullptr)) return DR_EINVAL;
    if (cfg->steps > 0 && (!x_T || !t_pcd_da || !cfg->h_alphas_cumprod || !cfg->h_times)) return DR_EINVAL;
    if ((matches == nullptr) != (match_count == nullptr)) return DR_EINVAL;
    if (trace && (trace->force_R == nullptr) != (trace->force_t == nullptr)) return DR_EINVAL;
    if (!workspace || workspace_bytes < dr_denoise_loop_2d3d_workspace_bytes(cfg, P, N, M)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Carver c(workspace);
    F2Ws L;
    F2Ws::carve(c, L, *cfg, P, N, M);
    DR_HIP_CHECK(hipMemsetAsync(L.status, 0, 16, st));          // the status of THIS call (dr_denoise_loop_status)
    const Sides S(P, M, N);             // image patches, then point nodes
    const int C = cfg->C, H = cfg->H, PM = P * M, PN = P * N, T = PM + PN;
    const size_t NM = (size_t)P * N * M;
    const int strict = (cfg->flags & DR_LOOP_STRICT_F64) ? DR_SK_STRICT : 0;
    const int mflag = masked ? DR_SK_APPLY_MASK : 0;
    int rc;

    // ---- step-invariant tokens (fusion_module.py:84-92): image tokens incl. their 2-D embedding, point tokens w/o embedding
    rc = gemm1(img_feats, cfg->img_dim, w->img_in_w, w->img_in_b, L.cat, 2 * C, PM, C, cfg->img_dim, EPI_RELU, 1.f, nullptr, st);
    if (rc) return rc;
    rc = gemm1(img_dino, cfg->dino_dim, w->dino_w, w->dino_b, L.cat + C, 2 * C, PM, C, cfg->dino_dim, EPI_RELU, 1.f, nullptr, st);
    if (rc) return rc;
    rc = gemm1(L.cat, 2 * C, w->all_w, w->all_b, L.tok0, C, PM, C, 2 * C, EPI_NONE, 1.f, nullptr, st);
    if (rc) return rc;
    rc = launch_fourier2d(img_pixels, PM, 10, L.emb2, 44, st);
    if (rc) return rc;
    rc = gemm1(L.emb2, 44, w->img_emb_w, w->img_emb_b, L.tok0, C, PM, C, 44, EPI_NONE, 1.f, L.tok0, st);     // tokens += embedding
    if (rc) return rc;
    // point tokens WITHOUT their embedding are step-invariant too: parked in L.proj's point rows (the per-step
    // embedding projection adds them back through the GEMM's addend)
    rc = gemm1(pcd_feats, cfg->pcd_dim, w->pcd_in_w, w->pcd_in_b, L.proj + (size_t)PM * C, C, PN, C, cfg->pcd_dim, EPI_NONE, 1.f, nullptr, st);
    if (rc) return rc;

    // ---- plane path, once per call: packed weights (the caller's, or packed now into the workspace), the image tokens' plane image
    // and the image half of layer 0 (a self layer: image tokens attend image tokens only -- step-invariant)
    Prepack2 pp;
    const bool want_feat = cfg->steps == 0;
    const Planes2& pw = L.pl;
    const P2Ctx X{&pp, &pw, S, C, H, (cfg->flags & DR_LOOP_ATTN_F16) ? 1 : 0};
    if (pw.on) {
        rc = packed_or_own(*cfg, *w, pw.own_pack, pp, st);
        if (rc == DR_OK) rc = side_planes_from_f32(S, SIDE_A, pw.tok0, C, pw.side_C, st);
        if (rc == DR_OK) rc = fusion_layer_planes(X, w->layers[0], 0, pw.tok0, SIDE_A, pw.tok0, SIDE_A, pw.l0, S.self_a(), nullptr, st);
        if (rc) return rc;
    }

    auto evaluate = [&](const float* Rf, const float* tf) -> int {
        // point tokens = base + pcd_emb_proj(Fourier(warped - mean))  (fusion_module.py:55-59, 93-94)
        int r = launch_fourier3d(s_pcd, P, N, Rf, tf, 10, L.emb3, 64, L.warped, st);
        if (r) return r;
        r = gemm1(L.emb3, 64, w->pcd_emb_w, w->pcd_emb_b, L.tok0 + (size_t)PM * C, C, PN, C, 64, EPI_NONE, 1.f, L.proj + (size_t)PM * C, st);
        if (r) return r;
        if (pw.on) {
            // the point tokens of this step -> their part of the token image (row maxima as bounds)
            r = side_planes_from_f32(S, SIDE_B, pw.tok0, C, pw.side_C, st);
            if (r) return r;
            // layer 0 (self): the image half is step-invariant and sits in pw.l0 already (evaluated once per call, above); the point half joins it there
            r = fusion_layer_planes(X, w->layers[0], 0, pw.tok0, SIDE_B, pw.tok0, SIDE_B, pw.l0, S.self_b(), nullptr, st);
            if (r) return r;
            const Tok* cur = &pw.l0;
            r = layer_schedule(S, 1, cfg->n_layers, cur, &pw.ta, &pw.tb,
                               [&](int l, int xs, const Tok* x, int ys, const Tok* y, const Tok* out, const Family& f1, const Family* f2) {
                return fusion_layer_planes(X, w->layers[l], l, *x, xs, *y, ys, *out, f1, f2, st);
            });
            if (r) return r;
            // out_proj (+ bias) -> image (+ fp32 rows when the caller wants the features), then the matching head's src_proj on both
            // sides (Q1) / sqrt(C) -> fp32 rows for the similarity
            PgBatch g;
            memset(&g, 0, sizeof(g));
            S.for_sides(SIDE_BOTH, [&](int side) {
                PgProblem& p = g.p[g.n++];
                const int r0 = S.r0(side);
                p.A0 = S.at(cur->img, pw.side_C, side); p.bnd0 = cur->bnd + r0; p.nc0 = C / 16;
                p.W = pp.out; p.nblk = 1; p.rows = S.rows(side); p.C = C; p.k_alg = C; p.mode = PG_PLANES; p.scale = 1.f;
                p.bias = w->out_b; p.bias_max = pp.out_bmax;
                p.pimg = S.at(pw.feat_img, pw.side_C, side); p.p_nct = C / 16; p.pbnd = pw.feat_bnd + r0;
                if (want_feat) { p.out = L.feat + (size_t)r0 * C; p.ldo = C; }
            });
            r = launch_pgemm(g, st);
            if (r) return r;
            memset(&g, 0, sizeof(g));
            S.for_sides(SIDE_BOTH, [&](int side) {
                PgProblem& p = g.p[g.n++];
                const int r0 = S.r0(side);
                p.A0 = S.at(pw.feat_img, pw.side_C, side); p.bnd0 = pw.feat_bnd + r0; p.nc0 = C / 16;
                p.W = pp.head; p.nblk = 1; p.rows = S.rows(side); p.C = C; p.k_alg = C; p.mode = PG_F32;
                p.out = L.z + (size_t)r0 * C; p.ldo = C; p.scale = 1.0f / sqrtf((float)C);
            });
            r = launch_pgemm(g, st);
            if (r) return r;
            r = gemm1(L.z + (size_t)PM * C, C, L.z, nullptr, L.sim, M, N, M, C, EPI_NONE, 1.f, nullptr, st, nullptr, nullptr, 0, P, (long long)N * C,
                      (long long)M * C, (long long)N * M);
            if (r) return r;
            return sinkhorn_f32(P, N, M, L.sim, src_mask, tgt_mask, w->bin_score, cfg->sk_iters, DR_SK_OUT_CONF | mflag, L.x0, L.skws,
                                L.skws_bytes, st, L.status);
        }
        const float* cur = L.tok0;
        r = layer_schedule(S, 0, cfg->n_layers, cur, L.ta, L.tb,
                           [&](int l, int xs, const float* x, int ys, const float* y, float* out, const Family& f1, const Family* f2) {
            return fusion_layer(w->layers[l], C, H, P, x, S.r0(xs), S.rows(xs), y, S.r0(ys), S.rows(ys), f1, f2, L, out, st);
        });
        if (r) return r;
        r = gemm1(cur, C, w->out_w, w->out_b, L.feat, C, T, C, C, EPI_NONE, 1.f, nullptr, st);
        if (r) return r;
        // matching head: src_proj on both sides (Q1), / sqrt(C), sim[p] = pcd_p img_p^T  (EXP/matching.py:100-125)
        r = gemm1(L.feat, C, w->src_proj, nullptr, L.z, C, T, C, C, EPI_NONE, 1.0f / sqrtf((float)C), nullptr, st);
        if (r) return r;
        for (int p0 = 0; p0 < P; p0 += 4) {
            GemmBatch g;
            memset(&g, 0, sizeof(g));
            g.n = (P - p0) < 4 ? (P - p0) : 4;
            for (int i = 0; i < g.n; ++i) {
                GemmProblem& q = g.p[i];
                const int pr = p0 + i;
                q.A = L.z + ((size_t)PM + (size_t)pr * N) * C; q.W = L.z + (size_t)pr * M * C;
                q.out = L.sim + (size_t)pr * N * M; q.rows = N; q.ncols = M; q.K = C; q.K1 = C; q.lda = C; q.ldo = M;
                q.epi = EPI_NONE; q.scale = 1.f;
            }
            r = launch_gemm(g, st);
            if (r) return r;
        }
        return sinkhorn_f32(P, N, M, L.sim, src_mask, tgt_mask, w->bin_score, cfg->sk_iters, DR_SK_OUT_CONF | mflag, L.x0, L.skws,
                            L.skws_bytes, st, L.status);
    };
    if (cfg->steps == 0) {          // component mode: one evaluation on the points as given
        rc = evaluate(nullptr, nullptr);
        if (rc) return rc;
        if (img_out) DR_HIP_CHECK(hipMemcpyAsync(img_out, L.feat, (size_t)PM * C * 4, hipMemcpyDeviceToDevice, st));
        if (pcd_out) DR_HIP_CHECK(hipMemcpyAsync(pcd_out, L.feat + (size_t)PM * C, (size_t)PN * C * 4, hipMemcpyDeviceToDevice, st));
        return launch_f32_to_f64(L.x0, conf, NM, st);
    }

    rc = launch_f32_to_f64(x_T, L.x, NM, st);
    if (rc) return rc;
    // -- the steps: the warp uses the masks (src, tgt_da) and no min-shift (EXP/model.py:830-846); the in-place fill of :832-834 with
    // tgt_mask_da persists in x
    SamplerArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.P = P; sa.N = N; sa.M = M; sa.steps = cfg->steps; sa.alphas_cumprod = cfg->h_alphas_cumprod; sa.times = cfg->h_times;
    sa.sample_rate = cfg->sample_rate; sa.max_condition_num = cfg->max_condition_num; sa.sk_iters = cfg->sk_iters; sa.strict = strict;
    sa.s_pcd = s_pcd; sa.warp_tgt_pcd = t_pcd_da; sa.src_mask = src_mask; sa.warp_tgt_mask = tgt_mask_da;
    sa.warp_mflag = mflag; sa.use_mask_len = 1; sa.bin_score = w->bin_score; sa.trace = trace;
    sa.x = L.x; sa.x_final = x_final; sa.x0 = L.x0; sa.wconf = L.wconf; sa.R = L.R; sa.t = L.t; sa.Rf = L.Rf; sa.tf = L.tf; sa.cond = L.cond; sa.ok = L.ok;
    sa.skws = L.skws; sa.skws_bytes = L.skws_bytes; sa.pws = L.pws; sa.pws_bytes = L.pws_bytes; sa.status = L.status;
    rc = reverse_sampling(sa, evaluate, st);
    if (rc) return rc;
    // read-out: no min-shift, masks (src, tgt) (EXP/model.py:681-694)
    rc = sinkhorn_f64(P, N, M, L.x, nullptr, src_mask, tgt_mask, w->bin_score, cfg->sk_iters, DR_SK_OUT_CONF | mflag | strict, conf,
                      L.skws, L.skws_bytes, st, L.status);
    if (rc) return rc;
    // (the steps' x0 tile is free by now; the row-block arg-maxima need < N M floats)
    if (matches) rc = launch_top1_union<double>(conf, P, N, M, (long long*)matches, match_count, st, nullptr, nullptr, L.x0, NM * 4);
    return rc;
}

}  // extern "C"
