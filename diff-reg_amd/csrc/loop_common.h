// loop_common.h -- host helpers shared by the two denoise loops (loop.hip, loop2d3d.hip), the single-op entries (api.hip) and the training
// entry points: the carving of caller memory (carve.h), the two-sided token view (Sides) and the ONE layer schedule of both denoisers, the plane
// path's small types, its packed-weight plumbing and its on / off rule, a one-problem GEMM launch, and reverse_sampling(), the ONE driver of
// the reverse-diffusion steps -- both loops honour the dr_loop_trace / teacher-forcing contract through it.
#pragma once
#include <math.h>
#include <string.h>
#include "kernels.h"
#include "pgemm.h"

namespace dr {

// a token tensor of the plane path: fp32 rows [T, C] (the residual stream; may be null), plane image (first side, then second side, each
// padded to 128 rows) and per-row bounds [T]
struct Tok { float* f32; char* img; float* bnd; };
struct Family {   // P segments: queries rows q0 + p*Lq (+Lq) attend keys rows k0 + p*Lk (+Lk)
    int q0, Lq, k0, Lk;
};
// the one or two families of an attention launch
static inline void attn_families(AttnArgs& a, int P, const Family& f1, const Family* f2) {
    a.nseg = P; a.q0 = f1.q0; a.qstride = f1.Lq; a.Lq = f1.Lq; a.k0 = f1.k0; a.kstride = f1.Lk; a.Lk = f1.Lk;
    if (f2) { a.nseg2 = P; a.q0b = f2->q0; a.qstrideb = f2->Lq; a.Lqb = f2->Lq; a.k0b = f2->k0; a.kstrideb = f2->Lk; a.Lkb = f2->Lk; }
}

// The two token sides of a call: all rows of side A (pair p at p * La), then all rows of side B (pair p at rows_a + p * Lb).  Which side is
// which is the loop's business (the header comment of loop.hip / loop2d3d.hip says).  A `side` argument is SIDE_A or SIDE_B (r0 takes SIDE_BOTH too:
// the whole token range starts at row 0); a mask is any of the three, or 0.
enum { SIDE_A = 1, SIDE_B = 2, SIDE_BOTH = 3 };
struct Sides {
    int P, La, Lb, rows_a, rows_b;           // pairs; rows per pair of each side; rows of each side (side B starts at row rows_a)
    Sides() = default;
    Sides(int P_, int La_, int Lb_) : P(P_), La(La_), Lb(Lb_), rows_a(P_ * La_), rows_b(P_ * Lb_) {}
    int r0(int side) const { return side == SIDE_B ? rows_a : 0; }
    int rows(int mask) const { return (mask & SIDE_A ? rows_a : 0) + (mask & SIDE_B ? rows_b : 0); }
    int per_pair(int side) const { return side == SIDE_B ? Lb : La; }
    int grp_first(int side) const { return side == SIDE_B ? P : 0; }        // first of the side's P groups in a [2 P] per-group array
    // the side's part of a two-sided plane image whose side B starts `side_off` bytes in
    template <class T> T* at(T* img, size_t side_off, int side) const { return img + (side == SIDE_B ? side_off : 0); }
    template <class F> void for_sides(int mask, F&& fn) const { for (int side = SIDE_A; side <= SIDE_B; ++side) if (mask & side) fn(side); }
    // the attention families: a side attends itself / side A attends side B / side B attends side A
    Family self_a() const { return {0, La, 0, La}; }
    Family self_b() const { return {rows_a, Lb, rows_a, Lb}; }
    Family cross_a() const { return {0, La, rows_a, Lb}; }
    Family cross_b() const { return {rows_a, Lb, 0, La}; }
};

// The layer schedule of both denoisers (pipeline.py:142, transformero.py:170-186; fusion_module.py:96-102): even layers are self layers on both
// sides; odd layers are cross layers -- side A attends side B, then side B attends the UPDATED side A (quirk Q11).  Walks layers
// [l_begin, n_layers) from the tokens in `cur`, writing buf0 and buf1 in turn, and leaves the last written buffer in `cur`.
// call(l, xs, x_tok, ys, y_tok, out_tok, f1, f2) evaluates layer l: the rows of side(s) xs of x_tok attend those of side(s) ys of y_tok.
template <class H, class B, class Call>
static int layer_schedule(const Sides& S, int l_begin, int n_layers, H& cur, B buf0, B buf1, Call&& call) {
    const Family self_a = S.self_a(), self_b = S.self_b(), cross_a = S.cross_a(), cross_b = S.cross_b();
    B bufs[2] = {buf0, buf1};
    for (int l = l_begin, which = 0; l < n_layers; ++l, which ^= 1) {
        B nxt = bufs[which];
        int rc;
        if (l % 2 == 0) {
            rc = call(l, SIDE_BOTH, cur, SIDE_BOTH, cur, nxt, self_a, &self_b);
        } else {
            rc = call(l, SIDE_A, cur, SIDE_B, cur, nxt, cross_a, nullptr);
            if (rc == DR_OK) rc = call(l, SIDE_B, cur, SIDE_A, H(nxt), nxt, cross_b, nullptr);
        }
        if (rc) return rc;
        cur = nxt;
    }
    return DR_OK;
}

// what a plane-path layer call needs besides its tokens (Pack / Ws: the loop's packed weights and plane buffers; the rotary tables and the
// token mask stay null in the 2D-3D loop)
template <class Pack, class Ws> struct PlaneCtx {
    const Pack* pp; const Ws* pw; Sides S;
    int C, H, attn_f16;                      // attn_f16: DR_LOOP_ATTN_F16
    const float *cosT, *sinT; const uint8_t* tokmask;
};
// bound of the keys' source rows per group (pair x side) for the sides in `mask`: bnd [T] -> grp_x [2 P]
static inline int side_group_max(const Sides& S, int mask, const float* bnd, float* grp_x, hipStream_t st) {
    int rc = DR_OK;
    S.for_sides(mask, [&](int side) { if (rc == DR_OK) rc = launch_group_max(bnd + S.r0(side), S.P, S.per_pair(side), grp_x + S.grp_first(side), st); });
    return rc;
}
// the fp32 rows of one side of a token buffer -> that side's part of its plane image, row maxima as bounds
static inline int side_planes_from_f32(const Sides& S, int side, const Tok& t, int C, size_t side_C, hipStream_t st) {
    return launch_planes_from_f32(t.f32 + (size_t)S.r0(side) * C, C, S.rows(side), C, S.at(t.img, side_C, side), t.bnd + S.r0(side), st);
}

// ---- packed weights of the plane path --------------------------------------------------------------------------------------------------
// room for one packed weight of nblk blocks x nct k-chunks (wide: in the wide-wave kernel's layout); viewed through *v where the carve is real
static inline void take_weight(Carver& c, int C, int nblk, int nct, PgW* v, bool wide = false) {
    char* p = c.take<char>(wide ? pgemm16w_weight_bytes(nblk, nct) : pgemm_weight_bytes(C, nblk, nct));
    if (!v || !p) return;
    if (wide) pgemm16w_weight_view(p, nblk, nct, v);
    else pgemm_weight_view(p, C, nblk, nct, v);
}
// packs one block of a weight in the layout of its view
static inline int pack_weight_block(const float* Wm, int Cc, int K, int plen, int ppad, const PgW& v, int nb, hipStream_t st, int olen = 0, int opad = 0) {
    return v.sub == 2 ? pgemm16w_pack_weights_block(Wm, Cc, K, plen, ppad, v, nb, st, olen, opad)
                      : pgemm_pack_weights_block(Wm, Cc, K, plen, ppad, v, nb, st, olen, opad);
}
// the views of a call's packed weights: the caller's buffer, or the workspace's own, packed now (Pack: Prepack / Prepack2)
template <class Pack, class Cfg, class W>
static int packed_or_own(const Cfg& cfg, const W& w, void* own_pack, Pack& pp, hipStream_t st) {
    void* buf = const_cast<void*>(w.prepacked);
    if (!buf) {
        buf = own_pack;
        const int rc = Pack::fill(buf, cfg, w, st);
        if (rc) return rc;
    }
    Pack::carve(buf, cfg, &pp);
    return DR_OK;
}

// blocks b0.. of a packed weight.  (The 2D-3D loop had a copy without the wide-wave branch: its weights are never packed in that layout,
// PgW::sub == 0, where the two bodies are the same function.)
static inline PgW pgw_blocks(const PgW& v, int b0, int C) {
    PgW r = v;
    if (v.sub == 2) { r.img += (size_t)b0 * v.nct * 576 * 64; r.cinv += (size_t)b0 * 576; r.wnorm += b0; return r; }   // (two sub-blocks of 288 rows per block)
    r.img += (size_t)b0 * v.nct * pgemm_bn(C) * 64; r.cinv += (size_t)b0 * pgemm_bn(C); r.wnorm += b0;
    return r;
}
// whether a loop call of `token_rows` rows runs its layers on plane images
// (crossover re-measured with the 64-row plane workgroups, tools/bench_planes_threshold.py: 256-point pairs 24.5 / 37.7 ms on the
//  f32 kernels against 31.6 / 31.9 ms on the plane path at 2048 / 4096 token rows; 512-point 4D pairs 60.9 vs 62.0 ms at 4096)
static inline bool planes_wanted(int flags, bool supported, int token_rows) {
    bool on = env_knob("DR_PLANES", 1) && supported && token_rows >= env_knob("DR_PLANES_MIN_ROWS", 4096);
    if (flags & DR_LOOP_PLANES_FORCE) on = supported;
    if (flags & DR_LOOP_PLANES_OFF) on = false;
    return on;
}

// launch_gemm of ONE problem on contiguous-k operands: bias / addend / rotary tables / strided batch as in GemmProblem (null or 0: none)
static inline int gemm1(const float* A, int lda, const float* W, const float* bias, float* out, int ldo, int rows, int ncols, int K, int epi,
                        float scale, const float* addend, hipStream_t st, const float* cosT = nullptr, const float* sinT = nullptr, int rot_C = 0,
                        int nbatch = 0, long long sA = 0, long long sW = 0, long long sO = 0) {
    GemmBatch g;
    memset(&g, 0, sizeof(g));
    GemmProblem& p = g.p[0];
    p.A = A; p.W = W; p.out = out; p.rows = rows; p.ncols = ncols; p.K = K; p.K1 = K; p.lda = lda; p.ldo = ldo;
    p.epi = epi; p.scale = scale; p.bias = bias; p.addend = addend; p.cosT = cosT; p.sinT = sinT; p.rot_C = rot_C;
    p.nbatch = nbatch; p.sA = sA; p.sW = sW; p.sO = sO;
    g.n = 1;
    return launch_gemm(g, st);
}

// the five DDIM coefficients of a step from alpha_cumprod[t] = a to alpha_cumprod[t_next] = an, eta = 1 (pipeline.py:246-256)
static inline void ddim_coefficients(double a, double an, DdimArgs& d) {
    d.sra = sqrt(1.0 / a); d.srm1 = sqrt(1.0 / a - 1.0);
    d.sigma = 1.0 * sqrt((1.0 - a / an) * (1.0 - an) / (1.0 - a));
    d.c = sqrt(1.0 - an - d.sigma * d.sigma);
    d.sqrt_an = (float)sqrt(an);
}

// scratch of a loop's Sinkhorn calls (the larger of the fp64-state and the fp32 form) and of its Procrustes fits; null where none is needed
static inline void sampler_scratch(Carver& c, int P, int N, int M, int flags, void*& skws, size_t& skws_bytes, void*& pws, size_t& pws_bytes) {
    const size_t a = dr_sinkhorn_workspace_bytes(P, N, M, 8, (flags & DR_LOOP_STRICT_F64) ? DR_SK_STRICT : 0);
    const size_t b = dr_sinkhorn_workspace_bytes(P, N, M, 4, 0);
    skws_bytes = a > b ? a : b;
    skws = skws_bytes ? (void*)c.take<char>(skws_bytes) : nullptr;
    pws_bytes = procrustes_workspace_bytes(P, N, M);
    pws = pws_bytes ? (void*)c.take<char>(pws_bytes) : nullptr;
}

// ---- the reverse-diffusion steps ----------------------------------------------------------------------------------------------------
// What differs between the 3D / 4D loop and the 2D-3D loop is data: filled on the stack per call, nothing is kept.
struct SamplerArgs {
    int P, N, M, steps;
    const double* alphas_cumprod; const int* times;             // host: alpha_cumprod table, the steps + 1 time indices
    float sample_rate, max_condition_num; int sk_iters, strict; // strict: DR_SK_STRICT or 0 (applies to the warp of steps k > 0)
    const float *s_pcd, *warp_tgt_pcd;                          // the warp fits s_pcd onto this target cloud ...
    const uint8_t *src_mask, *warp_tgt_mask;                    // ... under these masks (nullable), which the DDIM update fills in place too
    int warp_mflag, use_mask_len;                               // DR_SK_APPLY_MASK | DR_SK_RAGGED bits of the warp; launch_procrustes' use_mask_len
    bool min_shift; const uint8_t *rsm, *rtm; double* dmin; void* pmin;   // 3DMatch only: x - x.min() per pair first (ragged masks, [P] minima, scratch)
    const float* noise;                                         // 4DMatch only: [steps, P, N*M]
    const float* bin_score; const dr_loop_trace* trace;         // trace: nullable
    double *x, *x_final;                                        // the state (workspace); x_final (nullable): the caller's copy after the last step
    float *x0, *wconf, *R, *t, *Rf, *tf; double* cond; int* ok; // workspace
    void *skws, *pws; size_t skws_bytes, pws_bytes; unsigned* status;
};

// Runs a.steps steps on a.x.  evaluate(Rf, tf) is the denoiser: it leaves this step's float32 x0 in a.x0 for the source warped by (Rf, tf).
template <class Eval>
static int reverse_sampling(const SamplerArgs& a, Eval&& evaluate, hipStream_t st) {
    const int P = a.P, N = a.N, M = a.M;
    const size_t NM = (size_t)P * N * M;
    const dr_loop_trace* trace = a.trace;
    int rc;
    for (int k = 0; k < a.steps; ++k) {
        const int tcur = a.times[k], tnext = a.times[k + 1];
        // teacher forcing (parity tests): this step starts from the caller's state, not from the loop's own
        if (trace && trace->force_x) DR_HIP_CHECK(hipMemcpyAsync(a.x, trace->force_x + (size_t)k * NM, NM * 8, hipMemcpyDeviceToDevice, st));
        // -- [x <- x - x.min() (pipeline.py:239)]; mask; Sinkhorn; exp; slice; float32 (pipeline.py:293-302, EXP/model.py:830-846)
        const double* shift = nullptr;
        if (a.min_shift) {
            rc = launch_pair_min(a.x, P, N * M, a.dmin, st, M, a.rsm, a.rtm, a.pmin);
            if (rc) return rc;
            shift = a.dmin;
        }
        rc = sinkhorn_f64(P, N, M, a.x, shift, a.src_mask, a.warp_tgt_mask, a.bin_score, a.sk_iters,
                          DR_SK_OUT_CONF | DR_SK_OUT_F32 | a.warp_mflag | (k > 0 ? a.strict : 0), a.wconf, a.skws, a.skws_bytes, st, a.status);
        if (rc) return rc;
        // -- denoising_soft_procrustes (pipeline.py:304)
        int* tk = nullptr;
        if (trace && trace->topk_idx) {
            const size_t Kf = (size_t)(int)((float)(N > M ? N : M) * a.sample_rate);
            tk = trace->topk_idx + (size_t)k * P * Kf;
            DR_HIP_CHECK(hipMemsetAsync(tk, 0xff, (size_t)P * Kf * 4, st));
        }
        if (trace && trace->wconf) DR_HIP_CHECK(hipMemcpyAsync(trace->wconf + (size_t)k * NM, a.wconf, NM * 4, hipMemcpyDeviceToDevice, st));
        rc = launch_procrustes(a.wconf, a.s_pcd, a.warp_tgt_pcd, a.src_mask, a.warp_tgt_mask, P, N, M, a.use_mask_len, a.sample_rate,
                               a.max_condition_num, a.R, a.t, a.Rf, a.tf, a.cond, a.ok, tk, st, a.pws, a.pws_bytes);
        if (rc) return rc;
        if (trace && trace->R_forwd) DR_HIP_CHECK(hipMemcpyAsync(trace->R_forwd + (size_t)k * P * 9, a.Rf, (size_t)P * 36, hipMemcpyDeviceToDevice, st));
        if (trace && trace->t_forwd) DR_HIP_CHECK(hipMemcpyAsync(trace->t_forwd + (size_t)k * P * 3, a.tf, (size_t)P * 12, hipMemcpyDeviceToDevice, st));
        if (trace && trace->cond) DR_HIP_CHECK(hipMemcpyAsync(trace->cond + (size_t)k * P, a.cond, (size_t)P * 8, hipMemcpyDeviceToDevice, st));
        if (trace && trace->force_R) {           // teacher forcing: warp with the caller's pose (the fit above is traced all the same)
            DR_HIP_CHECK(hipMemcpyAsync(a.Rf, trace->force_R + (size_t)k * P * 9, (size_t)P * 36, hipMemcpyDeviceToDevice, st));
            DR_HIP_CHECK(hipMemcpyAsync(a.tf, trace->force_t + (size_t)k * P * 3, (size_t)P * 12, hipMemcpyDeviceToDevice, st));
        }
        // -- the denoiser on the source warped by this pose (pipeline.py:243-244, 306)
        rc = evaluate(a.Rf, a.tf);
        if (rc) return rc;
        if (trace && trace->x0) DR_HIP_CHECK(hipMemcpyAsync(trace->x0 + (size_t)k * NM, a.x0, NM * 4, hipMemcpyDeviceToDevice, st));
        // -- DDIM update (pipeline.py:246-256); the masks' in-place fill persists in x (EXP/model.py:832-834)
        DdimArgs d;
        d.x = a.x; d.x0 = a.x0; d.shift = shift; d.noise = a.noise ? a.noise + (size_t)k * NM : nullptr;
        d.src_mask = a.src_mask; d.tgt_mask = a.warp_tgt_mask; d.N = N; d.M = M; d.first_step = (k == 0);
        ddim_coefficients(a.alphas_cumprod[tcur], a.alphas_cumprod[tnext], d);
        rc = launch_ddim(d, P, st);
        if (rc) return rc;
        if (trace && trace->x_next) DR_HIP_CHECK(hipMemcpyAsync(trace->x_next + (size_t)k * NM, a.x, NM * 8, hipMemcpyDeviceToDevice, st));
    }
    if (a.x_final) DR_HIP_CHECK(hipMemcpyAsync(a.x_final, a.x, NM * 8, hipMemcpyDeviceToDevice, st));
    return DR_OK;
}

}  // namespace dr
