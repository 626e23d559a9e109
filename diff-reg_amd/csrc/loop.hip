// loop.hip -- host-side orchestration of the 3D / 4D reverse-diffusion matching loop: the attention layer on both GEMM paths, the
// denoiser + matching head, and the entries that need them (dr_attention_layer_*, dr_loop_prepack*, dr_denoiser_match_f32,
// dr_denoise_loop*).  The steps themselves are reverse_sampling() of loop_common.h, shared with loop2d3d.hip; the entries of the
// individual ops live in api.hip.  Everything is enqueued on the caller's stream; there is no host synchronisation anywhere, so the
// whole loop can be captured in a HIP graph.
//
// Token layout: all src superpoints of all P pairs, then all tgt superpoints:
//   rows [0, P*N) = src (pair p at p*N), rows [P*N, P*(N+M)) = tgt (pair p at P*N + p*M).
// In the terms of loop_common.h's Sides: side A = src (N rows per pair), side B = tgt (M rows per pair).
// Linear layers / LayerNorm / rotary are row-wise, so the P pairs simply widen the GEMMs; only the
// attention, the N x M matrices and the Procrustes fit know about pair boundaries.
#include "loop_common.h"

namespace dr {

// buffers of one attention-layer evaluation over `T` token rows
struct LayerWs {
    float *qkv, *att, *mrg, *msg, *hid, *g2;
    size_t T;
    static size_t carve(Carver& c, LayerWs& w, size_t T, int C) {
        w.T = T;
        w.qkv = c.take<float>(T * 3 * C);
        w.att = c.take<float>(T * C);
        w.mrg = c.take<float>(T * C);
        w.msg = c.take<float>(T * C);
        w.hid = c.take<float>(T * 2 * C);
        w.g2 = c.take<float>(T * C);
        return c.off;
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// Plane-image path of the layer GEMMs (pgemm.h): every activation that feeds a GEMM lives as an fp16 hi / lo plane image
// written by its producer; LayerNorm happens in the epilogue of the GEMM in front of it; weights are packed once.
// ---------------------------------------------------------------------------------------------------------------------
struct PrepackLayer {
    PgW qkv, merge, mlp0, mlp2;     // q|k|v: 3 blocks; merge: k order padded per head; mlp0: 2 blocks
    const float *lnB1, *lnB2;       // device scalars: bound of norm1 / norm2 outputs
};
struct Prepack {
    static constexpr int MAXL = 16;
    PrepackLayer L[MAXL];
    PgW head;                        // src_proj
    int dp;                          // head dim rounded up to 16
    static bool supported(const dr_loop_config& cfg) {
        if (!(cfg.n_layers <= MAXL && pgemm_shape_ok(cfg.C) && cfg.C % cfg.H == 0 && (cfg.C / cfg.H) % 4 == 0)) return false;
        const int dp = (cfg.C / cfg.H + 15) / 16 * 16;                 // the head-padded q | k | v block must fit the column block too
        return pgemm_shape_ok(cfg.H * dp) && pgemm_bn(cfg.H * dp) == pgemm_bn(cfg.C) && (dp == 64 || dp == 112 || dp == 144);
    }
    static bool wide_layout(const dr_loop_config& cfg) { return pgemm_bn(cfg.C) > 448 && env_knob("DR_PG_WIDE", 1) != 0; }
    // lays the images out in `buf` (nullptr: size only) and returns the byte count
    static size_t carve(void* buf, const dr_loop_config& cfg, Prepack* pp) {
        Carver c(buf);
        const int C = cfg.C, d = C / cfg.H, dp = (d + 15) / 16 * 16, nC = C / 16;
        if (pp) pp->dp = dp;
        // the launches without LayerNorm of the 576-column geometry (4DMatch) run on the wide-wave kernel: their weights in its layout
        const bool wide = wide_layout(cfg);
        for (int l = 0; l < cfg.n_layers; ++l) {
            PrepackLayer* L = pp ? &pp->L[l] : nullptr;
            take_weight(c, C, 3, nC, L ? &L->qkv : nullptr, wide);           // (C' = H dp output columns per block: same image size, C' <= BN)
            take_weight(c, C, 1, cfg.H * dp / 16, L ? &L->merge : nullptr);
            take_weight(c, C, 2, 2 * nC, L ? &L->mlp0 : nullptr, wide);
            take_weight(c, C, 1, 2 * nC, L ? &L->mlp2 : nullptr);
            float* b = c.take<float>(2);
            if (L && buf) { L->lnB1 = b; L->lnB2 = b + 1; }
        }
        take_weight(c, C, 1, nC, pp ? &pp->head : nullptr, wide);
        return c.off + 256;
    }
    static int fill(void* buf, const dr_loop_config& cfg, const dr_loop_weights& W, hipStream_t st) {
        Prepack pp;
        carve(buf, cfg, &pp);
        const int C = cfg.C, d = C / cfg.H;
        // q|k|v are three separate [C, C] tensors: pack them as three one-block images laid out back to back (the block stride
        // of a 3-block image is exactly one 1-block image minus its tail, so pack block by block into the 3-block view)
        for (int l = 0; l < cfg.n_layers; ++l) {
            const dr_layer_weights& w = W.layers[l];
            const PrepackLayer& L = pp.L[l];
            // q | k | v: output columns padded per head (d -> dp) so that the images the GEMM writes start every head at a k-chunk
            const int Cq = cfg.H * pp.dp;
            int rc = pack_weight_block(w.q_proj, Cq, C, C, C, L.qkv, 0, st, d, pp.dp);
            if (rc == DR_OK) rc = pack_weight_block(w.k_proj, Cq, C, C, C, L.qkv, 1, st, d, pp.dp);
            if (rc == DR_OK) rc = pack_weight_block(w.v_proj, Cq, C, C, C, L.qkv, 2, st, d, pp.dp);
            if (rc == DR_OK) rc = pack_weight_block(w.merge, C, C, d, pp.dp, L.merge, 0, st);
            if (rc == DR_OK) rc = pack_weight_block(w.mlp0, C, 2 * C, 2 * C, 2 * C, L.mlp0, 0, st);
            if (rc == DR_OK) rc = pack_weight_block(w.mlp0 + (size_t)C * 2 * C, C, 2 * C, 2 * C, 2 * C, L.mlp0, 1, st);
            if (rc == DR_OK) rc = pack_weight_block(w.mlp2, C, 2 * C, 2 * C, 2 * C, L.mlp2, 0, st);
            if (rc == DR_OK) rc = launch_ln_bound(w.norm1_w, w.norm1_b, C, (float*)L.lnB1, st);
            if (rc == DR_OK) rc = launch_ln_bound(w.norm2_w, w.norm2_b, C, (float*)L.lnB2, st);
            if (rc) return rc;
        }
        return pack_weight_block(W.src_proj, C, C, C, C, pp.head, 0, st);
    }
};

struct PlanesWs {
    bool on;
    Tok feat0, fa, fb, tgt_l0;
    char *att_img, *msg_img, *hid_img;
    float *att_bnd, *msg_bnd, *hid_bnd;
    char *qkv_img, *kvc_img;                 // q | k | v images (three images of H dp columns, back to back); cached k | v of layer 1
    float *qkv_bnd, *kvc_bnd;                // [3][T] / [2][T]
    float* grp_x;                            // [2 P] bound of x per key group (src groups, then tgt groups)
    // step-invariant projections, evaluated once per call (fill_step_invariants; `hoist`: diagnostics knob DR_LOOP_HOIST, default on):
    bool hoist;
    float* pre0;                             // [PN][2 H dp] layer 0, src rows: q | k in front of the rotary step (the src code moves, feat0 does not)
    char* v0_img; float *v0_bnd, *grp0;      // layer 0, src rows: the V image, its bounds [PN]; [P] bound of feat0 per src group
    char* q1_img; float* q1_bnd;             // layer 1, second cross call: q image of the tgt rows (PM rows), its row bounds [T] (token-indexed)
    // ... and the x half of mlp0 where x stays (`hoist_mlp0`: knob DR_LOOP_HOIST_MLP0, default on, off with DR_LOOP_HOIST=0): the accumulator slabs
    // (pgemm.h: acc_store / acc_load) of layer 0's src rows [0] and of layer 1's second cross call, tgt rows [1]; their room in floats; the form and
    // tiling that stored (launch_pgemm's tag: a host word -- the launches of one call are enqueued by one thread, in order)
    bool hoist_mlp0;
    float* x0_acc[2]; size_t x0_cap[2]; mutable unsigned long long x0_tag[2];
    float* csT;                              // [T][C/2][2] the rotary tables interleaved (cos, sin)
    size_t qkv_stride;                       // bytes from the q image to the k image (= to the next: v)
    size_t side_C, side_att, side_hid;      // byte offset of the tgt part inside an image of K = C / H dp / 2C
    void* own_pack;                         // packed weights inside the workspace (used when the caller passed none)
    // KSPLIT exchange of the LayerNorm launches (pgemm.h): partial sums + arrival flags (zeroed by planes_begin), the launches counted since then
    float* xk_buf; unsigned* xk_flags; mutable unsigned xk_epoch; unsigned* status;
    static size_t img_bytes(int PN, int PM, int K) { return plane_image_bytes(PN, K) + plane_image_bytes(PM, K); }
    static void carve(Carver& c, PlanesWs& w, const dr_loop_config& cfg, int P, int N, int M) {
        const int C = cfg.C, PN = P * N, PM = P * M, T = PN + PM;
        w.on = planes_wanted(cfg.flags, Prepack::supported(cfg), T);
        if (!w.on) return;
        const int dp = (C / cfg.H + 15) / 16 * 16;
        w.side_C = plane_image_bytes(PN, C); w.side_att = plane_image_bytes(PN, cfg.H * dp); w.side_hid = plane_image_bytes(PN, 2 * C);
        Tok* toks[4] = {&w.feat0, &w.fa, &w.fb, &w.tgt_l0};
        for (Tok* t : toks) { t->f32 = nullptr; t->img = c.take<char>(img_bytes(PN, PM, C)); t->bnd = c.take<float>(T); }
        w.att_img = c.take<char>(img_bytes(PN, PM, cfg.H * dp)); w.att_bnd = c.take<float>(T);
        w.msg_img = c.take<char>(img_bytes(PN, PM, C)); w.msg_bnd = c.take<float>(T);
        w.hid_img = c.take<char>(img_bytes(PN, PM, 2 * C)); w.hid_bnd = c.take<float>(T);
        w.qkv_stride = (img_bytes(PN, PM, cfg.H * dp) + 255) & ~(size_t)255;
        w.qkv_img = c.take<char>(3 * w.qkv_stride); w.qkv_bnd = c.take<float>(3 * (size_t)T);
        w.kvc_img = c.take<char>(2 * w.qkv_stride); w.kvc_bnd = c.take<float>(2 * (size_t)T);
        w.grp_x = c.take<float>(2 * (size_t)P);
        w.hoist = w.hoist_mlp0 = false;          // (carve_hoist: the buffers live in memory the plane path leaves idle)
        w.csT = c.take<float>((size_t)T * C);
        w.own_pack = c.take<char>(Prepack::carve(nullptr, cfg, nullptr));
        // (only launches of at most half a chip of 64-row workgroups are split: 128 row blocks on 256 CUs)
        const bool xk = (T + 63) / 64 + 2 <= PG_XK_MAX_RB;
        w.xk_buf = xk ? c.take<float>(pgemm_xk_buf_bytes(pgemm_bn(C)) / 4) : nullptr;
        w.xk_flags = xk ? c.take<unsigned>(pgemm_xk_flag_bytes() / 4) : nullptr;
        w.xk_epoch = 0; w.status = nullptr;
    }
    // The buffers of the once-per-call projections take no workspace of their own (the sizes the callers keep do not move): they are laid into
    // `bytes` at `mem` (nullptr: a size query), memory that no launch of the plane path touches.  Where they do not fit -- forced plane paths of
    // a few rows, whose images are mostly padding -- the loop keeps the per-step projections.
    static void carve_hoist(PlanesWs& w, char* mem, size_t bytes, const dr_loop_config& cfg, int P, int N, int M) {
        const int PN = P * N, PM = P * M, T = PN + PM, Cq = cfg.H * ((cfg.C / cfg.H + 15) / 16 * 16);
        Carver c(mem);
        w.pre0 = c.take<float>((size_t)PN * 2 * Cq);
        w.v0_img = c.take<char>(plane_image_bytes(PN, Cq)); w.v0_bnd = c.take<float>(PN); w.grp0 = c.take<float>(P);
        w.q1_img = c.take<char>(plane_image_bytes(PM, Cq)); w.q1_bnd = c.take<float>(T);
        w.hoist = c.off <= bytes && env_knob("DR_LOOP_HOIST", 1) != 0;
        // the slabs of mlp0's x half behind them, where the kernel form that runs mlp0 keeps accumulators between launches and the room is there
        const int side_rows[2] = {PN, PM};
        for (int i = 0; i < 2; ++i) {
            w.x0_cap[i] = pgemm_acc_cache_floats(side_rows[i], cfg.C, 2);
            w.x0_acc[i] = c.take<float>(w.x0_cap[i]);
            w.x0_tag[i] = 0;
        }
        w.hoist_mlp0 = w.hoist && c.off <= bytes && env_knob("DR_LOOP_HOIST_MLP0", 1) != 0 &&
                       pgemm_acc_cache_ok(cfg.C, cfg.C / 16, cfg.C / 16, Prepack::wide_layout(cfg) ? 2 : 0);
    }
};

// One GeometryAttentionLayer call (transformero.py:43-96) on token buffers.
//   xin rows [xr0, xr0 + xrows) are the queries/residual stream, yin rows [yr0, yr0 + yrows) the
//   source; out gets rows [xr0, xr0 + xrows).  fam2 may be null.
static int layer_call(const dr_layer_weights& W, int C, int H, int P, const float* xin, int xr0, int xrows,
                      const float* yin, int yr0, int yrows, const float* cosT, const float* sinT,
                      const uint8_t* tokmask, const Family& f1, const Family* f2, const LayerWs& ws, float* out,
                      hipStream_t st, const float* kv_cached = nullptr, float* kv_store = nullptr, const float* xq_in = nullptr,
                      const float* yk_in = nullptr) {
    // kv_cached: K|V of the source rows were projected earlier ([tokens, 2C], rotary applied to K): skip them.
    // kv_store : project ONLY K|V of the source rows into this buffer and return (used to fill the cache).
    // xq_in / yk_in: the inputs of the q / k projections where they are not x / y themselves (pe_type 'sinusoidal', transformero.py:50-57:
    //   q = W_q (x + pe_x), k = W_k (y + pe_y), v = W_v y); cosT == nullptr: no rotary code on q and k (sinusoidal, or the entangled form whose
    //   layers are called without a position code, transformero.py:246-252)
    const int halfC = C / 2, d = C / H;
    const bool rotary = cosT != nullptr;
    const float* const qin = xq_in ? xq_in : xin;
    const float* const kin = yk_in ? yk_in : yin;
    GemmBatch g;
    memset(&g, 0, sizeof(g));
    auto proj = [&](GemmProblem& p, const float* in, int r0, int rows, const float* Wm, int coloff, bool rot) {
        p.A = in + (size_t)r0 * C; p.A2 = nullptr; p.W = Wm; p.out = ws.qkv + (size_t)r0 * 3 * C + coloff;
        p.rows = rows; p.ncols = C; p.K = C; p.K1 = C; p.lda = C; p.lda2 = 0; p.ldo = 3 * C;
        p.epi = (rot && rotary) ? EPI_ROTARY : EPI_NONE; p.rot_C = C; p.scale = 1.f;
        p.cosT = rotary ? cosT + (size_t)r0 * halfC : nullptr; p.sinT = rotary ? sinT + (size_t)r0 * halfC : nullptr;
    };
    int rc;
    if (kv_store) {
        proj(g.p[0], kin, yr0, yrows, W.k_proj, 0, true);
        proj(g.p[1], yin, yr0, yrows, W.v_proj, 0, false);
        g.p[0].out = kv_store + (size_t)yr0 * 2 * C; g.p[0].ldo = 2 * C;
        g.p[1].out = kv_store + (size_t)yr0 * 2 * C + C; g.p[1].ldo = 2 * C;
        g.n = 2;
        return launch_gemm(g, st);
    }
    proj(g.p[0], qin, xr0, xrows, W.q_proj, 0, true);
    g.n = 1;
    if (!kv_cached) {
        proj(g.p[1], kin, yr0, yrows, W.k_proj, C, true);
        proj(g.p[2], yin, yr0, yrows, W.v_proj, 2 * C, false);
        g.n = 3;
    }
    rc = launch_gemm(g, st);
    if (rc) return rc;

    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.q = ws.qkv; a.k = ws.qkv + C; a.v = ws.qkv + 2 * C; a.out = ws.att;
    a.ldq = a.ldk = a.ldv = 3 * C; a.ldo = C; a.H = H; a.d = d;
    if (kv_cached) { a.k = kv_cached; a.v = kv_cached + C; a.ldk = a.ldv = 2 * C; }
    a.qmask = tokmask; a.kmask = tokmask;
    attn_families(a, P, f1, f2);
    a.scale = 1.0f / sqrtf((float)d);
    rc = launch_attention(a, st);
    if (rc) return rc;

    // message = norm1(merge(o))
    memset(&g, 0, sizeof(g));
    GemmProblem& m = g.p[0];
    m.A = ws.att + (size_t)xr0 * C; m.W = W.merge; m.out = ws.mrg + (size_t)xr0 * C;
    m.rows = xrows; m.ncols = C; m.K = C; m.K1 = C; m.lda = C; m.ldo = C; m.epi = EPI_NONE; m.scale = 1.f;
    g.n = 1;
    rc = launch_gemm(g, st);
    if (rc) return rc;
    rc = launch_layernorm(ws.mrg + (size_t)xr0 * C, C, W.norm1_w, W.norm1_b, nullptr, 0, ws.msg + (size_t)xr0 * C, C, xrows, C, st);
    if (rc) return rc;
    // message = norm2(mlp(cat[x, message]))
    memset(&g, 0, sizeof(g));
    GemmProblem& h = g.p[0];
    h.A = xin + (size_t)xr0 * C; h.A2 = ws.msg + (size_t)xr0 * C; h.W = W.mlp0; h.out = ws.hid + (size_t)xr0 * 2 * C;
    h.rows = xrows; h.ncols = 2 * C; h.K = 2 * C; h.K1 = C; h.lda = C; h.lda2 = C; h.ldo = 2 * C; h.epi = EPI_RELU; h.scale = 1.f;
    g.n = 1;
    rc = launch_gemm(g, st);
    if (rc) return rc;
    memset(&g, 0, sizeof(g));
    GemmProblem& o = g.p[0];
    o.A = ws.hid + (size_t)xr0 * 2 * C; o.W = W.mlp2; o.out = ws.g2 + (size_t)xr0 * C;
    o.rows = xrows; o.ncols = C; o.K = 2 * C; o.K1 = 2 * C; o.lda = 2 * C; o.ldo = C; o.epi = EPI_NONE; o.scale = 1.f;
    g.n = 1;
    rc = launch_gemm(g, st);
    if (rc) return rc;
    // e = x + message
    return launch_layernorm(ws.g2 + (size_t)xr0 * C, C, W.norm2_w, W.norm2_b, xin + (size_t)xr0 * C, C, out + (size_t)xr0 * C, C,
                            xrows, C, st);
}


// ---- the plane path of one GeometryAttentionLayer call (transformero.py:43-96): five launches ---------------------------------
using PlCtx = PlaneCtx<Prepack, PlanesWs>;
// exchange region of a problem whose launch may split its k range over two workgroups (pgemm.h: xk_buf).  The buffer holds PG_XK_MAX_RB units --
// one per 64-row block of a LayerNorm launch / per 128 x 288 tile of a wide-wave launch; the problems of a launch take consecutive regions
// (`next`: units handed out so far in this launch); the caller advances pw.xk_epoch once per launch that got regions.
static void xk_assign(const PlanesWs& pw, int C, PgProblem& p, size_t& next, size_t units) {
    if (!pw.xk_buf || next + units > (size_t)PG_XK_MAX_RB) return;
    p.xk_buf = pw.xk_buf + next * (pgemm_xk_buf_bytes(pgemm_bn(C)) / 4 / PG_XK_MAX_RB); p.xk_flags = pw.xk_flags + next * 2; p.xk_cap = (int)units;
    p.xk_epoch = pw.xk_epoch + 1; p.xk_status = pw.status;
    next += units;
}
static size_t xk_wide_units(const PgProblem& p) { return (size_t)(p.rows + 127) / 128 * p.nblk * 2; }

// what a call leaves in / takes from the once-per-call buffers of fill_step_invariants (PlanesWs: pre0, v0_*, q1_*)
struct PlHoist {
    bool l0_fill = false;   // layer 0, src rows: project q | k up to the rotary step (-> pre0) and V in its final form (-> v0_img) and return
    bool l0_use = false;    // layer 0, src rows: no projection launch -- q | k images by rot_images from pre0, V is v0_img
    bool q1_fill = false;   // project ONLY q of the x rows (tgt) into q1_img / q1_bnd and return
    bool q1_use = false;    // q of the x rows (tgt) is q1_img / q1_bnd: the projection launch carries K | V of the y rows only
    // one-sided calls whose x rows stay during a loop call (x0_slab: PlanesWs::x0_acc 0 / 1): mlp0 contracts [x | message], x first --
    bool x0_store = false;  // the first evaluation of a call: mlp0's launch leaves the accumulators of its x half in the slabs
    bool x0_use = false;    // every later one: mlp0's launch starts from them and contracts the message half only
    int x0_slab = 0;
    bool no_f32_out = false;   // nobody reads the fp32 rows of this call's result (the loop's last layer: the head takes the image): image only
};
static int layer_call_planes(const PlCtx& X, const dr_layer_weights& W, int l, const Tok& xin, int xs, const Tok& yin, int ys,
                             const Tok& out, const Family& f1, const Family* f2, hipStream_t st, const float* kv_cached = nullptr,
                             float* kv_store = nullptr, const PlHoist& hz = PlHoist()) {
    const Sides& S = X.S;
    const int C = X.C, H = X.H, PN = S.rows_a, PM = S.rows_b, halfC = C / 2, d = C / H, nC = C / 16, dp = X.pp->dp;
    const PrepackLayer& L = X.pp->L[l];
    const PlanesWs& pw = *X.pw;
    PgBatch g;
    size_t xk_next = 0;                   // exchange units handed to the problems of the launch being assembled
    auto reset = [&]() { memset(&g, 0, sizeof(g)); xk_next = 0; };
    auto add = [&]() -> PgProblem& { return g.p[g.n++]; };
    // KSPLIT exchange region of a LayerNorm problem (launch_pgemm decides whether the launch is split): the tgt side's row blocks behind the src side's
    auto xk = [&](PgProblem& p, size_t units) { xk_assign(pw, C, p, xk_next, units); };
    int rc;

    // ---- q | k | v projections + rotary -> three plane images of H dp columns (head h at k = h dp): the attention kernel's
    // operands.  q keeps a scale per row; all keys of a pair's side share ONE scale (k, v blocks take the bound of the row's group).
    const int T = PN + PM, Cq = H * dp, nq = Cq / 16;
    const bool cached = kv_cached != nullptr;            // (the plane path keeps the cached K | V as images: kvc_img / kvc_bnd)
    char* const kv_img = kv_store ? pw.kvc_img : pw.qkv_img + pw.qkv_stride;
    float* const kv_bnd = kv_store ? pw.kvc_bnd : pw.qkv_bnd + T;
    // bound of the keys' source rows per group (pair x side): taken inside the projection's own kernel when a group is a whole number of
    // workgroups (the 480 five-microsecond launches of a 20-step loop were 2 - 4 % of it), by a kernel of its own otherwise
    const bool grp_inline = S.La % 128 == 0 && S.Lb % 128 == 0 && env_knob("DR_LOOP_GRP_INLINE", 1) != 0;
    if (!cached && !grp_inline && !hz.l0_fill && !hz.l0_use && !hz.q1_fill) {
        rc = side_group_max(S, ys, yin.bnd, pw.grp_x, st);
        if (rc) return rc;
    }
    auto proj = [&](const Tok& tin, int side, int b0, int nblk, char* img, float* bnd, int rotm, int grpm) {
        PgProblem& p = add();
        p.A0 = S.at(tin.img, pw.side_C, side); p.bnd0 = tin.bnd + S.r0(side); p.nc0 = nC;
        p.W = pgw_blocks(L.qkv, b0, C); p.nblk = nblk; p.rows = S.rows(side); p.C = Cq; p.k_alg = C; p.mode = PG_PLANES;
        p.rot_mask = rotm; p.rot_C = C; p.rot_piece_len = d; p.rot_piece_pad = dp; p.scale = 1.f;
        p.cosT = X.cosT + (size_t)S.r0(side) * halfC; p.sinT = X.sinT + (size_t)S.r0(side) * halfC;
        p.csT = X.pw->csT + (size_t)S.r0(side) * halfC * 2;
        p.pimg = S.at(img, pw.side_att, side); p.p_nct = nq; p.pbnd = bnd + S.r0(side);
        p.pimg_blk_stride = (long long)pw.qkv_stride; p.pbnd_blk_stride = T;
        p.grp_bnd = grp_inline ? nullptr : pw.grp_x; p.grp_mask = grpm; p.grp_first = S.grp_first(side); p.grp_rows = S.per_pair(side);
        if (p.W.sub == 2) xk(p, xk_wide_units(p));
    };
    reset();
    if (kv_store) {
        S.for_sides(ys, [&](int side) { proj(yin, side, 1, 2, kv_img, kv_bnd, 1, 3); });
        ++pw.xk_epoch;
        return launch_pgemm(g, st);
    }
    // The once-per-call launches stand in for problems of a per-step launch: they take that launch's geometry (PgBatch::wg_as), so that the
    // accumulators are summed in its order and the images come out bit for bit as the per-step launch writes them.
    const int rbS = (PN + 127) / 128, rbT = (PM + 127) / 128;
    if (hz.l0_fill) {
        rc = launch_group_max(xin.bnd, S.P, S.La, pw.grp0, st);
        if (rc) return rc;
        // q | k: the value in front of the rotary step (the fp32 epilogue without rotary: the same accumulators, column and row scales)
        proj(xin, SIDE_A, 0, 2, pw.qkv_img, pw.qkv_bnd, 0, 0);
        g.p[0].mode = PG_F32; g.p[0].pimg = nullptr; g.p[0].pbnd = nullptr;
        g.p[0].out = pw.pre0; g.p[0].ldo = 2 * Cq; g.p[0].blk_stride = Cq;
        g.wg_as = 3 * rbS;
        ++pw.xk_epoch;
        rc = launch_pgemm(g, st);
        if (rc) return rc;
        reset();
        proj(xin, SIDE_A, 2, 1, pw.v0_img, pw.v0_bnd, 0, 1);
        g.p[0].grp_bnd = pw.grp0; g.p[0].grp_first = 0;
        g.wg_as = 3 * rbS;
        ++pw.xk_epoch;
        return launch_pgemm(g, st);
    }
    if (hz.q1_fill) {
        proj(xin, SIDE_B, 0, 1, pw.qkv_img, pw.qkv_bnd, 1, 0);
        g.p[0].pimg = pw.q1_img; g.p[0].pbnd = pw.q1_bnd + PN;
        g.wg_as = rbT + 2 * rbS;
        ++pw.xk_epoch;
        return launch_pgemm(g, st);
    }
    const bool self = xs == ys && xin.img == yin.img && !cached;
    if (hz.l0_use) {
        RotImgArgs r;
        memset(&r, 0, sizeof(r));
        r.x = pw.pre0; r.ldx = 2 * Cq; r.x_blk = Cq; r.rows = PN; r.C = Cq; r.nblk = 2;
        r.csT = pw.csT; r.rot_mask = 3; r.rot_C = C; r.rot_piece_len = d; r.rot_piece_pad = dp; r.scale = 1.f;
        r.bnd0 = xin.bnd; r.wnorm = L.qkv.wnorm; r.wide_form = L.qkv.sub == 2; r.grp_bnd = pw.grp0; r.grp_mask = 2; r.grp_first = 0; r.grp_rows = S.La;
        r.pimg = pw.qkv_img; r.p_nct = nq; r.pbnd = pw.qkv_bnd; r.pimg_blk_stride = (long long)pw.qkv_stride; r.pbnd_blk_stride = T;
        rc = launch_rot_images(r, st);
        if (rc) return rc;
    } else {
        if (self) {
            S.for_sides(xs, [&](int side) { proj(xin, side, 0, 3, pw.qkv_img, pw.qkv_bnd, 3, 6); });
        } else {
            if (!hz.q1_use) S.for_sides(xs, [&](int side) { proj(xin, side, 0, 1, pw.qkv_img, pw.qkv_bnd, 1, 0); });
            else g.wg_as = rbT + 2 * rbS;
            if (!cached) S.for_sides(ys, [&](int side) { proj(yin, side, 1, 2, kv_img, kv_bnd, 1, 3); });
        }
        ++pw.xk_epoch;
        rc = launch_pgemm(g, st);
        if (rc) return rc;
    }

    // ---- attention on the images -> plane image of the heads' outputs (head h at k = h dp)
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.H = H; a.d = d;
    a.qmask = X.tokmask; a.kmask = X.tokmask;
    attn_families(a, S.P, f1, f2);
    a.scale = 1.0f / sqrtf((float)d);
    a.pimg[0] = pw.att_img; a.pimg[1] = pw.att_img + pw.side_att; a.p_split = PN; a.p_nct = nq; a.p_dp = dp;
    a.pbnd = pw.att_bnd;
    {
        const char* kimg = cached ? pw.kvc_img : pw.qkv_img + pw.qkv_stride;
        const float* kb = cached ? pw.kvc_bnd : pw.qkv_bnd + T;
        a.qimg[0] = pw.qkv_img; a.qimg[1] = pw.qkv_img + pw.side_att;
        a.kimg[0] = kimg; a.kimg[1] = kimg + pw.side_att;
        a.vimg[0] = kimg + pw.qkv_stride; a.vimg[1] = kimg + pw.qkv_stride + pw.side_att;
        a.qbnd = pw.qkv_bnd; a.kgb = kb; a.vgb = kb + T;
        if (hz.l0_use) { a.vimg[0] = pw.v0_img; a.vgb = pw.v0_bnd; }          // (src keys only: rows below PN)
        if (hz.q1_use) { a.qimg[1] = pw.q1_img; a.qbnd = pw.q1_bnd; }          // (tgt queries only: rows from PN)
        a.f16_single = X.attn_f16;
    }
    rc = launch_attention(a, st);
    if (rc) return rc;

    // ---- message = norm1(merge(o)) -> plane image
    reset();
    S.for_sides(xs, [&](int side) {
        PgProblem& p = add();
        p.A0 = S.at(pw.att_img, pw.side_att, side); p.bnd0 = pw.att_bnd + S.r0(side); p.nc0 = H * dp / 16;
        p.W = L.merge; p.nblk = 1; p.rows = S.rows(side); p.C = C; p.mode = PG_LN; p.k_alg = C;
        p.gamma = W.norm1_w; p.beta = W.norm1_b; p.lnB = L.lnB1;
        p.pimg = S.at(pw.msg_img, pw.side_C, side); p.p_nct = nC; p.pbnd = pw.msg_bnd + S.r0(side);
        xk(p, (size_t)(p.rows + 63) / 64);
    });
    ++pw.xk_epoch;
    rc = launch_pgemm(g, st);
    if (rc) return rc;
    // ---- hidden = relu(mlp0([x | message])) -> plane image
    reset();
    S.for_sides(xs, [&](int side) {
        PgProblem& p = add();
        p.A0 = S.at(xin.img, pw.side_C, side); p.bnd0 = xin.bnd + S.r0(side); p.nc0 = nC;
        p.A1 = S.at(pw.msg_img, pw.side_C, side); p.bnd1 = pw.msg_bnd + S.r0(side); p.nc1 = nC;
        p.W = L.mlp0; p.nblk = 2; p.rows = S.rows(side); p.C = C; p.mode = PG_PLANES; p.relu = 1; p.scale = 1.f;
        p.pimg = S.at(pw.hid_img, pw.side_hid, side); p.p_nct = 2 * nC; p.pbnd = pw.hid_bnd + S.r0(side);
        if (p.W.sub == 2) xk(p, xk_wide_units(p));
        if (hz.x0_store || hz.x0_use) {
            if (hz.x0_store) p.acc_store = pw.x0_acc[hz.x0_slab];
            else p.acc_load = pw.x0_acc[hz.x0_slab];
            p.acc_cap = pw.x0_cap[hz.x0_slab]; p.acc_tag = &pw.x0_tag[hz.x0_slab];
        }
    });
    ++pw.xk_epoch;
    rc = launch_pgemm(g, st);
    if (rc) return rc;
    // ---- out = x + norm2(mlp2(hidden)) -> fp32 rows (the residual stream) + plane image (the next GEMMs' operand)
    reset();
    S.for_sides(xs, [&](int side) {
        PgProblem& p = add();
        p.A0 = S.at(pw.hid_img, pw.side_hid, side); p.bnd0 = pw.hid_bnd + S.r0(side); p.nc0 = 2 * nC;
        p.W = L.mlp2; p.nblk = 1; p.rows = S.rows(side); p.C = C; p.mode = PG_LN;
        p.gamma = W.norm2_w; p.beta = W.norm2_b; p.lnB = L.lnB2;
        p.resid = xin.f32 + (size_t)S.r0(side) * C; p.ldr = C; p.bnd_res = xin.bnd + S.r0(side);
        p.out = hz.no_f32_out ? nullptr : out.f32 + (size_t)S.r0(side) * C; p.ldo = C;
        p.pimg = S.at(out.img, pw.side_C, side); p.p_nct = nC; p.pbnd = out.bnd + S.r0(side);
        xk(p, (size_t)(p.rows + 63) / 64);
    });
    ++pw.xk_epoch;
    return launch_pgemm(g, st);
}

// workspace of one denoiser + matching-head evaluation
struct DenoiseWs {
    LayerWs lw;
    float *fa, *fb, *cosT, *sinT, *proj, *sim;
    float *tgt_l0, *kv_l1;      // step-invariant: layer-0 output of the tgt rows, layer-1 K|V of those rows
    PlanesWs pl;
    const Prepack* pp;          // packed weights of the plane path (set per call)
    Sides S;                    // src rows, then tgt rows
    static void carve(Carver& c, DenoiseWs& w, const dr_loop_config& cfg, int P, int N, int M) {
        const int C = cfg.C;
        w.S = Sides(P, N, M);
        const size_t T = (size_t)P * (N + M);
        const size_t lw_begin = align256(c.off);
        LayerWs::carve(c, w.lw, T, C);
        const size_t lw_end = c.off;
        PlanesWs::carve(c, w.pl, cfg, P, N, M);
        // (the activations of the f32-input layers: layer_call's alone -- a call on the plane path never reads or writes them)
        if (w.pl.on) PlanesWs::carve_hoist(w.pl, c.base ? c.base + lw_begin : nullptr, lw_end - lw_begin, cfg, P, N, M);
        w.tgt_l0 = c.take<float>(T * C);
        w.kv_l1 = c.take<float>(T * 2 * C);
        w.fa = c.take<float>(T * C);
        w.fb = c.take<float>(T * C);
        w.cosT = c.take<float>(T * (C / 2));
        w.sinT = c.take<float>(T * (C / 2));
        w.proj = c.take<float>(T * C);
        w.sim = c.take<float>((size_t)P * N * M);
        if (w.pl.on) { w.pl.fa.f32 = w.fa; w.pl.fb.f32 = w.fb; w.pl.tgt_l0.f32 = w.tgt_l0; }
    }
};

// six layers self, cross, ... (pipeline.py:142; transformero.py:170-186) starting from feat0,
// then the matching head's projection + N x M similarity (matching.py:173-207).  PE tables must be
// filled.  On return *final points at the buffer holding the refined features and ws.sim holds sim.
// The tgt cloud never moves and layer 0 is a self layer, so the tgt half of layer 0 and the K|V projections of
// layer 1's first cross call do not depend on the step (the reference recomputes them 20 times): fill_step_invariants
// evaluates them once per loop, denoiser_and_sim(use_cache) reuses them.  Results are bit-identical.
// On the plane path two more pieces stay from step to step (PlanesWs::hoist): layer 0's q | k | v projections of the SRC rows up to the rotary
// step (their input is the caller's feat0; only the src position code moves: a row-wise kernel applies it per step, V is final), and the q image of
// layer 1's second cross call (tgt_l0 and the tgt code).
static PlCtx plane_ctx(const dr_loop_config& cfg, const DenoiseWs& ws, const uint8_t* tokmask) {
    return PlCtx{ws.pp, &ws.pl, ws.S, cfg.C, cfg.H, (cfg.flags & DR_LOOP_ATTN_F16) ? 1 : 0, ws.cosT, ws.sinT, tokmask};
}
// layer_call on the rows of side(s) xs of x and ys of y
static int layer_call_sides(const dr_loop_config& cfg, const dr_layer_weights& W, const float* x, int xs, const float* y, int ys, const uint8_t* tokmask,
                            const Family& f1, const Family* f2, const DenoiseWs& ws, float* out, hipStream_t st, const float* kv_cached = nullptr,
                            float* kv_store = nullptr) {
    const Sides& S = ws.S;
    return layer_call(W, cfg.C, cfg.H, S.P, x, S.r0(xs), S.rows(xs), y, S.r0(ys), S.rows(ys), ws.cosT, ws.sinT, tokmask, f1, f2, ws.lw, out, st,
                      kv_cached, kv_store);
}

static int fill_step_invariants(const dr_loop_config& cfg, const dr_loop_weights& w, const float* feat0, const uint8_t* tokmask, DenoiseWs& ws,
                                hipStream_t st) {
    const Family self_s = ws.S.self_a(), self_t = ws.S.self_b();
    if (ws.pl.on) {
        const PlCtx X = plane_ctx(cfg, ws, tokmask);
        int rc = layer_call_planes(X, w.layers[0], 0, ws.pl.feat0, SIDE_B, ws.pl.feat0, SIDE_B, ws.pl.tgt_l0, self_t, nullptr, st);
        if (rc == DR_OK && ws.pl.hoist) {
            PlHoist hz; hz.l0_fill = true;
            rc = layer_call_planes(X, w.layers[0], 0, ws.pl.feat0, SIDE_A, ws.pl.feat0, SIDE_A, ws.pl.tgt_l0, self_s, nullptr, st, nullptr, nullptr, hz);
        }
        if (rc || cfg.n_layers < 2) return rc;
        rc = layer_call_planes(X, w.layers[1], 1, ws.pl.tgt_l0, 0, ws.pl.tgt_l0, SIDE_B, ws.pl.tgt_l0, self_t, nullptr, st, nullptr, ws.kv_l1);
        if (rc || !ws.pl.hoist) return rc;
        PlHoist hz; hz.q1_fill = true;
        return layer_call_planes(X, w.layers[1], 1, ws.pl.tgt_l0, SIDE_B, ws.pl.tgt_l0, 0, ws.pl.tgt_l0, self_t, nullptr, st, nullptr, nullptr, hz);
    }
    int rc = layer_call_sides(cfg, w.layers[0], feat0, SIDE_B, feat0, SIDE_B, tokmask, self_t, nullptr, ws, ws.tgt_l0, st);
    if (rc || cfg.n_layers < 2) return rc;
    return layer_call_sides(cfg, w.layers[1], nullptr, 0, ws.tgt_l0, SIDE_B, tokmask, self_t, nullptr, ws, nullptr, st, nullptr, ws.kv_l1);
}

static int denoiser_and_sim(const dr_loop_config& cfg, const dr_loop_weights& w, const float* feat0, const uint8_t* tokmask, DenoiseWs& ws,
                            const float** final_feats, hipStream_t st, bool use_cache = false, bool first_eval = true, bool final_f32 = true) {
    // first_eval (with use_cache): the first evaluation since fill_step_invariants -- it leaves mlp0's x half of the two calls whose x stays
    // (layer 0 on the src rows: x = feat0; layer 1's second cross call: x = the tgt rows of tgt_l0) for the later ones (PlanesWs::hoist_mlp0).
    // final_f32 = false: the caller reads no fp32 rows of the last layer (*final_feats is then null on the plane path: the head takes the image).
    const Sides& S = ws.S;
    const int C = cfg.C, P = S.P, N = S.La, M = S.Lb, PN = S.rows_a;
    // the matching head on the f32-input GEMM: src_proj on BOTH sides (quirk Q1), rotary, / sqrt(C) ...
    auto head = [&](const float* feats) {
        return gemm1(feats, C, w.src_proj, nullptr, ws.proj, C, S.rows(SIDE_BOTH), C, C, EPI_ROTARY, 1.0f / sqrtf((float)C), nullptr, st, ws.cosT, ws.sinT, C);
    };
    // ... and sim[p] = a_p b_p^T : one NT GEMM per pair, all P pairs as one strided batch
    auto sim = [&]() {
        return gemm1(ws.proj, C, ws.proj + (size_t)PN * C, nullptr, ws.sim, M, N, M, C, EPI_NONE, 1.f, nullptr, st, nullptr, nullptr, 0, P,
                     (long long)N * C, (long long)M * C, (long long)N * M);
    };
    // with the cache, layer 0 runs on the src half only, written beside the cached tgt half into the cache's own token buffer (rows, plane image,
    // bounds): layer 1 reads both halves there and nothing later writes to it (no copy of the cached half).  The schedule then starts at layer 1,
    // whose first cross call takes the cached K | V of the tgt rows (and, on the plane path, whose second takes the q image projected once per call).
    const int l_begin = use_cache ? 1 : 0;
    if (ws.pl.on) {
        const PlCtx X = plane_ctx(cfg, ws, tokmask);
        const Tok* cur = &ws.pl.feat0;
        int rc = DR_OK;
        const bool x0 = use_cache && ws.pl.hoist_mlp0;
        const bool head_f32 = env_knob("DR_HEAD_F32", 0) != 0;
        const bool drop_f32 = !final_f32 && !head_f32;      // the last layer's fp32 rows have no reader
        if (use_cache) {
            PlHoist hz; hz.l0_use = ws.pl.hoist;
            hz.x0_store = x0 && first_eval; hz.x0_use = x0 && !first_eval; hz.x0_slab = 0;
            hz.no_f32_out = drop_f32 && cfg.n_layers == 1;
            rc = layer_call_planes(X, w.layers[0], 0, *cur, SIDE_A, *cur, SIDE_A, ws.pl.tgt_l0, S.self_a(), nullptr, st, nullptr, nullptr, hz);
            cur = &ws.pl.tgt_l0;
        }
        if (rc == DR_OK)
            rc = layer_schedule(S, l_begin, cfg.n_layers, cur, (const Tok*)&ws.pl.fa, (const Tok*)&ws.pl.fb,
                                [&](int l, int xs, const Tok* x, int ys, const Tok* y, const Tok* out, const Family& f1, const Family* f2) {
                const bool l1 = use_cache && l == 1;
                PlHoist hz; hz.q1_use = l1 && xs == SIDE_B && ws.pl.hoist;
                const bool x1 = x0 && l1 && xs == SIDE_B;
                hz.x0_store = x1 && first_eval; hz.x0_use = x1 && !first_eval; hz.x0_slab = 1;
                hz.no_f32_out = drop_f32 && l == cfg.n_layers - 1;
                return layer_call_planes(X, w.layers[l], l, *x, xs, *y, ys, *out, f1, f2, st, (l1 && xs == SIDE_A) ? ws.kv_l1 : nullptr, nullptr, hz);
            });
        if (rc) return rc;
        *final_feats = drop_f32 ? nullptr : cur->f32;
        if (head_f32) {
            // (experiment: the head's projection on the f32-input MFMA GEMM, 24-bit operands, from the fp32 rows of the last layer)
            rc = head(cur->f32);
            return rc ? rc : sim();
        }
        // matching head: src_proj on BOTH sides (quirk Q1), rotary, / sqrt(C)
        PgBatch g;
        memset(&g, 0, sizeof(g));
        size_t xk_next = 0;
        S.for_sides(SIDE_BOTH, [&](int side) {
            PgProblem& p = g.p[g.n++];
            const int r0 = S.r0(side);
            p.A0 = S.at(cur->img, ws.pl.side_C, side); p.bnd0 = cur->bnd + r0; p.nc0 = C / 16;
            p.W = ws.pp->head; p.nblk = 1; p.rows = S.rows(side); p.C = C; p.mode = PG_F32;
            p.out = ws.proj + (size_t)r0 * C; p.ldo = C; p.blk_stride = 0; p.rot_mask = 1; p.rot_C = C; p.scale = 1.0f / sqrtf((float)C);
            p.cosT = ws.cosT + (size_t)r0 * (C / 2); p.sinT = ws.sinT + (size_t)r0 * (C / 2);
            p.csT = ws.pl.csT + (size_t)r0 * C;
            if (p.W.sub == 2) xk_assign(ws.pl, C, p, xk_next, xk_wide_units(p));
        });
        ++ws.pl.xk_epoch;
        rc = launch_pgemm(g, st);
        return rc ? rc : sim();
    }
    const float* cur = feat0;
    int rc = DR_OK;
    if (use_cache) {
        rc = layer_call_sides(cfg, w.layers[0], cur, SIDE_A, cur, SIDE_A, tokmask, S.self_a(), nullptr, ws, ws.tgt_l0, st);
        cur = ws.tgt_l0;
    }
    if (rc == DR_OK)
        rc = layer_schedule(S, l_begin, cfg.n_layers, cur, ws.fa, ws.fb,
                            [&](int l, int xs, const float* x, int ys, const float* y, float* out, const Family& f1, const Family* f2) {
            return layer_call_sides(cfg, w.layers[l], x, xs, y, ys, tokmask, f1, f2, ws, out, st, (use_cache && l == 1 && xs == SIDE_A) ? ws.kv_l1 : nullptr);
        });
    if (rc) return rc;
    *final_feats = cur;
    rc = head(cur);
    return rc ? rc : sim();
}

static int fill_pe(const dr_loop_config& cfg, const dr_loop_weights& w, int P, int N, int M, const float* s_pcd,
                   const float* Rf, const float* tf, const float* t_pcd, bool do_src, bool do_tgt, DenoiseWs& ws,
                   hipStream_t st) {
    const int halfC = cfg.C / 2;
    int rc = DR_OK;
    if (do_src)
        rc = launch_vol_pe(s_pcd, P * N, N, Rf, tf, cfg.C, cfg.origin[0], cfg.origin[1], cfg.origin[2], cfg.voxel, w.pe_freq,
                           ws.cosT, ws.sinT, st, ws.pl.on ? ws.pl.csT : nullptr);
    if (rc == DR_OK && do_tgt)
        rc = launch_vol_pe(t_pcd, P * M, M, nullptr, nullptr, cfg.C, cfg.origin[0], cfg.origin[1], cfg.origin[2], cfg.voxel,
                           w.pe_freq, ws.cosT + (size_t)P * N * halfC, ws.sinT + (size_t)P * N * halfC, st,
                           ws.pl.on ? ws.pl.csT + (size_t)P * N * halfC * 2 : nullptr);
    return rc;
}

struct LoopWs {
    DenoiseWs dw;
    float *feat0, *wconf, *x0, *R, *t, *Rf, *tf, *conf32;
    double *x, *dmin, *cond;
    void* pmin;                              // pair_min_scratch_bytes(P): slice minima + arrival counters of the multi-workgroup minimum
    int* ok;
    uint8_t* tokmask;
    void* skws;
    size_t skws_bytes;
    void* pws;
    size_t pws_bytes;
    unsigned* status;                        // the call's own sticky status word (dr_denoise_loop_status): zeroed when a call starts
    static size_t carve(Carver& c, LoopWs& w, const dr_loop_config& cfg, int P, int N, int M) {
        const size_t T = (size_t)P * (N + M), NM = (size_t)P * N * M;
        w.status = c.take<unsigned>(4);      // (first: its place does not depend on the configuration)
        DenoiseWs::carve(c, w.dw, cfg, P, N, M);
        w.feat0 = c.take<float>(T * cfg.C);
        if (w.dw.pl.on) w.dw.pl.feat0.f32 = w.feat0;
        w.wconf = c.take<float>(NM);
        w.x0 = c.take<float>(NM);
        w.conf32 = c.take<float>(NM);
        w.x = c.take<double>(NM);
        w.dmin = c.take<double>(P);
        w.cond = c.take<double>(P);
        w.pmin = (void*)c.take<char>(pair_min_scratch_bytes(P));
        w.R = c.take<float>((size_t)P * 9);
        w.t = c.take<float>((size_t)P * 3);
        w.Rf = c.take<float>((size_t)P * 9);
        w.tf = c.take<float>((size_t)P * 3);
        w.ok = c.take<int>(P);
        w.tokmask = c.take<uint8_t>(T);
        sampler_scratch(c, P, N, M, cfg.flags, w.skws, w.skws_bytes, w.pws, w.pws_bytes);
        return c.off + 256;
    }
};

// plane path, once per call: the packed weights (the caller's, or packed now into the workspace) and the plane image of the
// external features with their row maxima as bounds
static int planes_begin(const dr_loop_config& cfg, const dr_loop_weights& w, DenoiseWs& ws, Prepack& pp, hipStream_t st) {
    if (!ws.pl.on) return DR_OK;
    int rc = packed_or_own(cfg, w, ws.pl.own_pack, pp, st);
    if (rc) return rc;
    ws.pp = &pp;
    if (ws.pl.xk_flags) {
        DR_HIP_CHECK(hipMemsetAsync(ws.pl.xk_flags, 0, pgemm_xk_flag_bytes(), st));
        ws.pl.xk_epoch = 0;
    }
    ws.S.for_sides(SIDE_BOTH, [&](int side) { if (rc == DR_OK) rc = side_planes_from_f32(ws.S, side, ws.pl.feat0, cfg.C, ws.pl.side_C, st); });
    return rc;
}

// what both loop entries do first: lay out the workspace, zero the call's status word, gather the features and the masks in token order
static int loop_begin(const dr_loop_config& cfg, int P, int N, int M, const float* src_feats, const float* tgt_feats, const uint8_t* src_mask,
                      const uint8_t* tgt_mask, void* workspace, LoopWs& L, hipStream_t st) {
    Carver c(workspace);
    LoopWs::carve(c, L, cfg, P, N, M);
    DR_HIP_CHECK(hipMemsetAsync(L.status, 0, 16, st));          // the status of THIS call (one 16-byte fill per call)
    L.dw.pl.status = L.status;
    const size_t PN = (size_t)P * N, PM = (size_t)P * M;
    DR_HIP_CHECK(hipMemcpyAsync(L.feat0, src_feats, PN * cfg.C * 4, hipMemcpyDeviceToDevice, st));
    DR_HIP_CHECK(hipMemcpyAsync(L.feat0 + PN * cfg.C, tgt_feats, PM * cfg.C * 4, hipMemcpyDeviceToDevice, st));
    if (src_mask) {
        DR_HIP_CHECK(hipMemcpyAsync(L.tokmask, src_mask, PN, hipMemcpyDeviceToDevice, st));
        DR_HIP_CHECK(hipMemcpyAsync(L.tokmask + PN, tgt_mask, PM, hipMemcpyDeviceToDevice, st));
    }
    return DR_OK;
}

}  // namespace dr

using namespace dr;

extern "C" {

size_t dr_attention_layer_workspace_bytes(int P, int Lx, int Ly, int C) {
    Carver c(nullptr);
    LayerWs w;
    const size_t T = (size_t)P * (Lx + Ly);
    LayerWs::carve(c, w, T, C);
    c.take<float>(T * C);          // x|y token buffer
    c.take<float>(T * C);          // output token buffer
    c.take<float>(T * (C / 2));    // cos
    c.take<float>(T * (C / 2));    // sin
    c.take<uint8_t>(T);
    c.take<float>(T * C);          // q | k inputs of the additive (sinusoidal) form
    return c.off + 256;
}

int dr_attention_layer_f32(const dr_layer_weights* w, int C, int H, int P, int Lx, int Ly, const float* x, const float* y,
                           const float* cos_x, const float* sin_x, const float* cos_y, const float* sin_y,
                           const uint8_t* x_mask, const uint8_t* y_mask, float* out, void* workspace,
                           size_t workspace_bytes, void* stream) {
    if (!cos_x || !sin_x || !cos_y || !sin_y) return DR_EINVAL;
    return dr_attention_layer_pe_f32(w, C, H, P, Lx, Ly, x, y, nullptr, nullptr, cos_x, sin_x, cos_y, sin_y, x_mask, y_mask, out, workspace,
                                     workspace_bytes, stream);
}

int dr_attention_layer_pe_f32(const dr_layer_weights* w, int C, int H, int P, int Lx, int Ly, const float* x, const float* y,
                              const float* xq, const float* yk, const float* cos_x, const float* sin_x, const float* cos_y, const float* sin_y,
                              const uint8_t* x_mask, const uint8_t* y_mask, float* out, void* workspace,
                              size_t workspace_bytes, void* stream) {
    if (!w || !x || !y || !out || P < 1 || Lx < 1 || Ly < 1 || C % H || (C / H) % 4 || C % 4) return DR_EINVAL;
    if ((x_mask == nullptr) != (y_mask == nullptr)) return DR_EINVAL;
    const bool rotary = cos_x != nullptr;
    if ((sin_x != nullptr) != rotary || (cos_y != nullptr) != rotary || (sin_y != nullptr) != rotary) return DR_EINVAL;
    if ((xq == nullptr) != (yk == nullptr) || (xq && rotary)) return DR_EINVAL;   // additive code and rotary code exclude each other (pe_type)
    if (workspace_bytes < dr_attention_layer_workspace_bytes(P, Lx, Ly, C) || !workspace) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    Carver c(workspace);
    LayerWs lw;
    const size_t T = (size_t)P * (Lx + Ly), PX = (size_t)P * Lx, PY = (size_t)P * Ly;
    const int halfC = C / 2;
    LayerWs::carve(c, lw, T, C);
    float* tok = c.take<float>(T * C);
    float* otok = c.take<float>(T * C);
    float* cosT = c.take<float>(T * halfC);
    float* sinT = c.take<float>(T * halfC);
    uint8_t* mask = c.take<uint8_t>(T);
    float* qk_buf = c.take<float>(T * C);
    DR_HIP_CHECK(hipMemcpyAsync(tok, x, PX * C * 4, hipMemcpyDeviceToDevice, st));
    DR_HIP_CHECK(hipMemcpyAsync(tok + PX * C, y, PY * C * 4, hipMemcpyDeviceToDevice, st));
    float* qk_tok = nullptr;                       // q | k inputs of the additive form
    if (rotary) {
        DR_HIP_CHECK(hipMemcpyAsync(cosT, cos_x, PX * halfC * 4, hipMemcpyDeviceToDevice, st));
        DR_HIP_CHECK(hipMemcpyAsync(cosT + PX * halfC, cos_y, PY * halfC * 4, hipMemcpyDeviceToDevice, st));
        DR_HIP_CHECK(hipMemcpyAsync(sinT, sin_x, PX * halfC * 4, hipMemcpyDeviceToDevice, st));
        DR_HIP_CHECK(hipMemcpyAsync(sinT + PX * halfC, sin_y, PY * halfC * 4, hipMemcpyDeviceToDevice, st));
    } else if (xq) {
        qk_tok = qk_buf;
        DR_HIP_CHECK(hipMemcpyAsync(qk_tok, xq, PX * C * 4, hipMemcpyDeviceToDevice, st));
        DR_HIP_CHECK(hipMemcpyAsync(qk_tok + PX * C, yk, PY * C * 4, hipMemcpyDeviceToDevice, st));
    }
    if (x_mask) {
        DR_HIP_CHECK(hipMemcpyAsync(mask, x_mask, PX, hipMemcpyDeviceToDevice, st));
        DR_HIP_CHECK(hipMemcpyAsync(mask + PX, y_mask, PY, hipMemcpyDeviceToDevice, st));
    }
    const Family f{0, Lx, (int)PX, Ly};
    int rc = layer_call(*w, C, H, P, tok, 0, (int)PX, tok, (int)PX, (int)PY, rotary ? cosT : nullptr, rotary ? sinT : nullptr,
                        x_mask ? mask : nullptr, f, nullptr, lw, otok, st, nullptr, nullptr, qk_tok, qk_tok);
    if (rc) return rc;
    DR_HIP_CHECK(hipMemcpyAsync(out, otok, PX * C * 4, hipMemcpyDeviceToDevice, st));
    return DR_OK;
}

static int check_cfg(const dr_loop_config* cfg, const dr_loop_weights* w, int P, int N, int M) {
    if (!cfg || !w || P < 1 || N < 1 || M < 1) return DR_EINVAL;
    if (cfg->C % cfg->H || (cfg->C / cfg->H) % 4 || cfg->C % 6 || cfg->n_layers < 1 || cfg->sk_iters < 1) return DR_EINVAL;
    if (!w->layers || !w->src_proj || !w->bin_score || !w->pe_freq) return DR_EINVAL;
    if (cfg->variant != DR_VARIANT_3DMATCH && cfg->variant != DR_VARIANT_4DMATCH) return DR_EINVAL;
    return DR_OK;
}

size_t dr_loop_prepack_bytes(const dr_loop_config* cfg) {
    if (!cfg || !Prepack::supported(*cfg)) return 0;
    return Prepack::carve(nullptr, *cfg, nullptr);
}

int dr_loop_prepack(const dr_loop_config* cfg, const dr_loop_weights* w, void* packed, size_t packed_bytes, void* stream) {
    if (!cfg || !w || !w->layers || !w->src_proj || !packed || ((uintptr_t)packed & 255)) return DR_EINVAL;
    if (!Prepack::supported(*cfg)) return DR_ENOSUP;
    if (packed_bytes < Prepack::carve(nullptr, *cfg, nullptr)) return DR_EWORKSPACE;
    return Prepack::fill(packed, *cfg, *w, (hipStream_t)stream);
}

size_t dr_denoise_loop_workspace_bytes(const dr_loop_config* cfg, int P, int N, int M) {
    if (!cfg || P < 1 || N < 1 || M < 1) return 0;
    Carver c(nullptr);
    LoopWs w;
    return LoopWs::carve(c, w, *cfg, P, N, M);
}

int dr_denoise_loop_status(void* workspace, void* stream, int clear) {
    if (!workspace) return DR_EINVAL;
    Carver c(workspace);
    return sinkhorn_call_status(c.take<unsigned>(4), (hipStream_t)stream, clear != 0);
}

int dr_denoiser_match_f32(const dr_loop_config* cfg, const dr_loop_weights* w, int P, int N, int M, const float* src_feats,
                          const float* tgt_feats, const float* s_pcd_warped, const float* t_pcd, const uint8_t* src_mask,
                          const uint8_t* tgt_mask, float* src_out, float* tgt_out, float* conf, void* workspace,
                          size_t workspace_bytes, void* stream) {
    int rc = check_cfg(cfg, w, P, N, M);
    if (rc) return rc;
    if (!src_feats || !tgt_feats || !s_pcd_warped || !t_pcd || !conf) return DR_EINVAL;
    if ((src_mask == nullptr) != (tgt_mask == nullptr)) return DR_EINVAL;
    if (!workspace || workspace_bytes < dr_denoise_loop_workspace_bytes(cfg, P, N, M)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    LoopWs L;
    rc = loop_begin(*cfg, P, N, M, src_feats, tgt_feats, src_mask, tgt_mask, workspace, L, st);
    if (rc) return rc;
    const int C = cfg->C;
    const size_t PN = (size_t)P * N, PM = (size_t)P * M;
    Prepack pp;
    rc = planes_begin(*cfg, *w, L.dw, pp, st);
    if (rc) return rc;
    rc = fill_pe(*cfg, *w, P, N, M, s_pcd_warped, nullptr, nullptr, t_pcd, true, true, L.dw, st);
    if (rc) return rc;
    const float* fin = nullptr;
    rc = denoiser_and_sim(*cfg, *w, L.feat0, src_mask ? L.tokmask : nullptr, L.dw, &fin, st);
    if (rc) return rc;
    if (src_out) DR_HIP_CHECK(hipMemcpyAsync(src_out, fin, PN * C * 4, hipMemcpyDeviceToDevice, st));
    if (tgt_out) DR_HIP_CHECK(hipMemcpyAsync(tgt_out, fin + PN * C, PM * C * 4, hipMemcpyDeviceToDevice, st));
    return sinkhorn_f32(P, N, M, L.dw.sim, src_mask, tgt_mask, w->bin_score, cfg->sk_iters,
                        DR_SK_OUT_CONF | (src_mask ? DR_SK_APPLY_MASK : 0), conf, L.skws, L.skws_bytes, st, L.status);
}

int dr_denoise_loop(const dr_loop_config* cfg, const dr_loop_weights* w, int P, int N, int M, const float* src_feats,
                    const float* tgt_feats, const float* s_pcd, const float* t_pcd, const uint8_t* src_mask,
                    const uint8_t* tgt_mask, const float* x_T, const float* noise, double* conf, double* x_final,
                    int64_t* matches, int32_t* match_count, float* R_final, float* t_final, const dr_loop_trace* trace,
                    void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_cfg(cfg, w, P, N, M);
    if (rc) return rc;
    if (!src_feats || !tgt_feats || !s_pcd || !t_pcd || !x_T || !conf || cfg->steps < 1 || !cfg->h_alphas_cumprod || !cfg->h_times)
        return DR_EINVAL;
    if ((src_mask == nullptr) != (tgt_mask == nullptr)) return DR_EINVAL;
    const bool v4d = cfg->variant == DR_VARIANT_4DMATCH;
    if (v4d && !noise) return DR_EINVAL;
    if ((matches == nullptr) != (match_count == nullptr) || (R_final == nullptr) != (t_final == nullptr)) return DR_EINVAL;
    if (trace && (trace->force_R == nullptr) != (trace->force_t == nullptr)) return DR_EINVAL;
    if (!workspace || workspace_bytes < dr_denoise_loop_workspace_bytes(cfg, P, N, M)) return DR_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    LoopWs L;
    rc = loop_begin(*cfg, P, N, M, src_feats, tgt_feats, src_mask, tgt_mask, workspace, L, st);
    if (rc) return rc;
    const int C = cfg->C;
    const size_t PN = (size_t)P * N, PM = (size_t)P * M, NM = (size_t)P * N * M;
    const uint8_t* tokmask = src_mask ? L.tokmask : nullptr;
    const int strict = (cfg->flags & DR_LOOP_STRICT_F64) ? DR_SK_STRICT : 0;
    // DR_LOOP_RAGGED: the masks are the true extents of pairs padded to (N, M); every pair gets its unpadded result
    const bool ragged = (cfg->flags & DR_LOOP_RAGGED) && src_mask;
    const int mflag = src_mask ? (DR_SK_APPLY_MASK | (ragged ? DR_SK_RAGGED : 0)) : 0;
    const uint8_t* rsm = ragged ? src_mask : nullptr;
    const uint8_t* rtm = ragged ? tgt_mask : nullptr;

    rc = launch_f32_to_f64(x_T, L.x, NM, st);     // exact widening; step 1 keeps float32 semantics
    if (rc) return rc;
    if (!v4d && P <= 32)                          // arrival counters of the multi-workgroup minimum (few pairs: stateops.hip)
        DR_HIP_CHECK(hipMemsetAsync((char*)L.pmin + pair_min_scratch_bytes(P) - 64 * (size_t)P, 0, 64 * (size_t)P, st));
    Prepack pp;
    rc = planes_begin(*cfg, *w, L.dw, pp, st);
    if (rc) return rc;
    // the target cloud never moves: its position code is computed once (the reference recomputes it
    // every step, transformero.py:166)
    rc = fill_pe(*cfg, *w, P, N, M, s_pcd, nullptr, nullptr, t_pcd, false, true, L.dw, st);
    if (rc) return rc;
    rc = fill_step_invariants(*cfg, *w, L.feat0, tokmask, L.dw, st);
    if (rc) return rc;

    // -- the steps: x <- x - x.min() first (3D only), per-step noise (4D only); the denoiser of a step is the position code of the warped
    // source (pipeline.py:306, transformero.py:165), denoising_transformer + denoising_coarse_matching (pipeline.py:243-244) and the
    // float32 Sinkhorn of the similarity
    const float* fin = nullptr;
    SamplerArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.P = P; sa.N = N; sa.M = M; sa.steps = cfg->steps; sa.alphas_cumprod = cfg->h_alphas_cumprod; sa.times = cfg->h_times;
    sa.sample_rate = cfg->sample_rate; sa.max_condition_num = cfg->max_condition_num; sa.sk_iters = cfg->sk_iters; sa.strict = strict;
    sa.s_pcd = s_pcd; sa.warp_tgt_pcd = t_pcd; sa.src_mask = src_mask; sa.warp_tgt_mask = tgt_mask;
    sa.warp_mflag = mflag; sa.use_mask_len = (v4d || ragged) ? 1 : 0;
    sa.min_shift = !v4d; sa.rsm = rsm; sa.rtm = rtm; sa.dmin = L.dmin; sa.pmin = P <= 32 ? L.pmin : nullptr;
    sa.noise = v4d ? noise : nullptr; sa.bin_score = w->bin_score; sa.trace = trace;
    sa.x = L.x; sa.x_final = x_final; sa.x0 = L.x0; sa.wconf = L.wconf; sa.R = L.R; sa.t = L.t; sa.Rf = L.Rf; sa.tf = L.tf; sa.cond = L.cond; sa.ok = L.ok;
    sa.skws = L.skws; sa.skws_bytes = L.skws_bytes; sa.pws = L.pws; sa.pws_bytes = L.pws_bytes; sa.status = L.status;
    // (the fp32 rows of the last layer are read by the trace's feature outputs alone: the matching head takes the plane image)
    const bool final_f32 = trace && (trace->feats_nopos || trace->feats_pos);
    int evals = 0;                                // evaluations since fill_step_invariants
    rc = reverse_sampling(sa, [&](const float* Rf, const float* tf) -> int {
        int r = fill_pe(*cfg, *w, P, N, M, s_pcd, Rf, tf, t_pcd, true, false, L.dw, st);
        if (r == DR_OK) r = denoiser_and_sim(*cfg, *w, L.feat0, tokmask, L.dw, &fin, st, true, evals++ == 0, final_f32);
        if (r) return r;
        return sinkhorn_f32(P, N, M, L.dw.sim, src_mask, tgt_mask, w->bin_score, cfg->sk_iters, DR_SK_OUT_CONF | mflag, L.x0, L.skws, L.skws_bytes, st,
                            L.status);
    }, st);
    if (rc) return rc;
    if (trace && (trace->feats_nopos || trace->feats_pos) && fin) {
        // data["src_feats_nopos"] / ["src_feats"] (+ tgt) of the last Matching.forward (matching.py:177-187): src_proj on both
        // sides (quirk Q1), without and with the rotary embedding of the last step's position code
        for (int pos = 0; pos < 2; ++pos) {
            float* dst = pos ? trace->feats_pos : trace->feats_nopos;
            if (!dst) continue;
            rc = gemm1(fin, C, w->src_proj, nullptr, dst, C, (int)(PN + PM), C, C, pos ? EPI_ROTARY : EPI_NONE, 1.f, nullptr, st, L.dw.cosT, L.dw.sinT, C);
            if (rc) return rc;
        }
    }

    // -- read-out
    if (v4d) {
        rc = launch_sigmoid(L.x, conf, NM, st);                       // 4D/models/pipeline.py:192
        if (rc) return rc;
    } else {
        rc = launch_pair_min(L.x, P, N * M, L.dmin, st, M, rsm, rtm, P <= 32 ? L.pmin : nullptr);  // pipeline.py:264-272
        if (rc) return rc;
        rc = sinkhorn_f64(P, N, M, L.x, L.dmin, src_mask, tgt_mask, w->bin_score, cfg->sk_iters, DR_SK_OUT_CONF | mflag | strict,
                          conf, L.skws, L.skws_bytes, st, L.status);
        if (rc) return rc;
        if (matches) {
            // (the steps' x0 tile is free by now; the row-block arg-maxima need < N M floats)
            rc = launch_top1_union<double>(conf, P, N, M, (long long*)matches, match_count, st, rsm, rtm, L.x0, NM * 4);
            if (rc) return rc;
        }
    }
    if (R_final) {
        // soft_procrustes on float32(conf): the well-defined value of pipeline.py:282 (quirk Q3)
        rc = launch_f64_to_f32(conf, L.conf32, NM, st);
        if (rc) return rc;
        rc = launch_procrustes(L.conf32, s_pcd, t_pcd, src_mask, tgt_mask, P, N, M, (v4d || ragged) ? 1 : 0, cfg->sample_rate,
                               cfg->max_condition_num, R_final, t_final, L.Rf, L.tf, L.cond, L.ok, nullptr, st, L.pws, L.pws_bytes);
        if (rc) return rc;
    }
    return DR_OK;
}

}  // extern "C"
