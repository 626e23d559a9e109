// loop_common.h -- host helpers shared by the two denoise loops (loop.hip, loop2d3d.hip), the single-op entries (api.hip) and the training
// entry points: the carving of caller memory, the plane path's small types and its on / off rule, a one-problem GEMM launch, and
// reverse_sampling(), the ONE driver of the reverse-diffusion steps -- both loops honour the dr_loop_trace / teacher-forcing contract
// through it.
#pragma once
#include <math.h>
#include <string.h>
#include "kernels.h"
#include "pgemm.h"

namespace dr {

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// hands out consecutive arrays of caller memory, each starting at a multiple of 256 bytes; a null base only counts (`off` = bytes so far)
struct Carver {
    char* base; size_t off;
    explicit Carver(void* p) : base((char*)p), off(0) {}
    template <typename T> T* take(size_t n) {
        off = align256(off);
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return r;
    }
};

// a token tensor of the plane path: fp32 rows [T, C] (the residual stream; may be null), plane image (first side, then second side, each
// padded to 128 rows) and per-row bounds [T]
struct Tok { float* f32; char* img; float* bnd; };
struct Family {   // P segments: queries rows q0 + p*Lq (+Lq) attend keys rows k0 + p*Lk (+Lk)
    int q0, Lq, k0, Lk;
};
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
