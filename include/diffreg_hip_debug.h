/* diffreg_hip_debug.h -- diagnostics of libdiffreg_hip.so for tools/ and for the kernel-forcing test fixtures.
 * NOT part of the drop-in boundary (include/diffreg_hip.h): nothing a deployment calls is declared here.
 *
 * The library reads no environment variable unless dr_debug_enable_env(1) was called: the DR_* tuning variables of tools/
 * (DR_GEMM_*, DR_ATTN_*, DR_PLANES*, DR_PG_*, DR_SK_PERSIST_GRID) cannot change which kernels a deployment runs.  Once enabled they are
 * re-read on every launch (nothing is latched).  The plane GEMM's: DR_PG_HALF (0 / 2: never / always 64-row workgroups), DR_PG_HALF_PCT (the
 * 64-row rule's threshold in percent of the CU count), DR_PG_M16 (0: the 32x32x16 main loop instead of the 16x16x32 one), DR_PG_NOEPI (timing
 * ablations, WRONG results: bit 0 return behind the main loop, 2 no fp32 row stores, 3 no image stores, 4 no residual loads, 5 no rotary tables).  Per-call choices of the product path are arguments: dr_loop_config.flags
 * (DR_LOOP_PLANES_FORCE / _OFF, DR_LOOP_STRICT_F64, DR_LOOP_RAGGED), DR_SK_* flags.  The setters below are process-wide and meant
 * for single-threaded tools and tests only. */
#ifndef DIFFREG_HIP_DEBUG_H
#define DIFFREG_HIP_DEBUG_H
#include "diffreg_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

void dr_debug_enable_env(int on);
/* force the f32-input GEMM configuration: -1 auto, 0 / 9 LDS-staged 32 x 32 / 64 x 64 single-buffer tiles, 11 / 12 the latency
 * form with 8 / 16 waves (K <= 448 / 896: a launch beyond that returns DR_ENOSUP); any other value makes every launch DR_EINVAL */
void dr_debug_gemm_config(int c);
/* one grouped launch of the f32-input GEMM in its internal problem form (what the ABI's dr_linear_f32 / dr_linear_ex_f32 /
 * dr_gemm_nt_batched_f32 cannot express: a two-segment A, an addend, bias with rotary, a column offset of `out`, 2..4 different problems in one
 * grid), for the per-geometry tests.  Problem i:
 *   acc[r][c] = sum_{k < K1} A[r lda + k] W[c K + k] + sum_{K1 <= k < K} A2[r lda2 + k - K1] W[c K + k]    (A2 == NULL: K1 is ignored)
 *   out[r ldo + c] = scale * relu(rot(acc)[r][c] + bias[c]) + addend[r ldo + c]    for r < rows, c < ncols
 * rot (epilogue & 2): with h = c % rot_C / 2, rot(acc)[r][2j] = acc[r][2j] cos_t[r rot_C/2 + h] - acc[r][2j+1] sin_t[..], rot(acc)[r][2j+1] =
 * acc[r][2j+1] cos_t[..] + acc[r][2j] sin_t[..]; relu (epilogue & 1); bias / addend NULL: none.  nbatch > 1: instance z reads A + z stride_a,
 * W + z stride_w and writes out + z stride_o (floats); A2, bias, addend and the rotary tables are shared by all instances.
 * K, K1, lda, lda2 multiples of 4 and A, A2, W 16-byte aligned (else DR_ENOSUP, as inside the library).  The geometry is the automatic one
 * or the one dr_debug_gemm_config forced; n outside 1..4 or a malformed problem -> DR_EINVAL. */
typedef struct dr_debug_gemm_problem {
    const float* A;
    const float* A2;
    const float* W;
    float* out;
    const float* cos_t;
    const float* sin_t;
    const float* bias;
    const float* addend;
    int rows, ncols, K, K1, lda, lda2, ldo;
    int epilogue;
    int rot_C;
    float scale;
    int nbatch;
    long long stride_a, stride_w, stride_o;
} dr_debug_gemm_problem;
int dr_debug_gemm_f32(const dr_debug_gemm_problem* problems, int n, void* stream);
/* attention: use the 128-query (flash) kernel from this many workgroups on; -1 = default rule (256) */
void dr_debug_attention_config(int flash_min_workgroups);
/* flash attention arithmetic: 1 = split-operand bf16 MFMA products (default), 0 = f32-input MFMA, -1 = default */
void dr_debug_attention_split(int on);
/* which kernel form the last attention launch of the calling thread chose (dr_attention_f32, dr_attention_planes[_f16], the attention launches
 * inside a layer or loop call): set on the host just before the kernel launch, 0 before any launch and after a call that launched nothing
 * (an argument the dispatcher refused, zero segments).
 *   bits 0..3   the form: 1 the 32-query kernel with 4 waves, 2 the 32-query kernel with 8 waves, 3 the 128-query flash kernel on the f32-input
 *               MFMA, 4 the flash kernel on split bf16 operands, 5 the plane-image kernel with one key group, 6 the one with two key groups
 *   bit 4       plane-image forms: ONE fp16 product per contraction (dr_attention_planes_f16)
 *   bit 5       plane-image forms: the XCD dealing of the workgroups is on
 *   bits 8..15  the head-dim geometry's count of 8-column groups: 8 (d <= 64), 14 (d <= 112), 17 (d <= 136), 20 (d <= 160) */
#define DR_ATTN_FORM_Q32_W4 1
#define DR_ATTN_FORM_Q32_W8 2
#define DR_ATTN_FORM_FLASH_F32 3
#define DR_ATTN_FORM_FLASH_SPLIT 4
#define DR_ATTN_FORM_PLANES_KG1 5
#define DR_ATTN_FORM_PLANES_KG2 6
#define DR_ATTN_FORM_MASK 0xf
#define DR_ATTN_FORM_F16 0x10
#define DR_ATTN_FORM_XCD 0x20
#define DR_ATTN_FORM_GEOM_SHIFT 8
int dr_debug_attention_last_form(void);
/* which launch form the last dr_procrustes_f32 of the calling thread (or the fit inside a loop call) took: set on the host just before the
 * launches, -1 before any call and after a call that launched nothing (P = 0, DR_ENOSUP).
 *   0  one workgroup per pair on a register-resident tile (N M <= 65536)
 *   1  whole-chip sliced selection, the take pass keeps its slice's keys in registers (slices of at most 32768 entries)
 *   2  whole-chip sliced selection, the take pass re-reads its keys (longer slices) */
#define DR_PROC_FORM_REG 0
#define DR_PROC_FORM_SLICED 1
#define DR_PROC_FORM_SLICED_REREAD 2
int dr_debug_procrustes_last_form(void);
/* which plane-GEMM forms kept or took up the accumulators of a step-invariant first operand segment (the x half of mlp0 in the 3D / 4D loop)
 * in the launches the calling thread has enqueued since the last call with clear != 0; 0: none did (the feature is off, or the geometry has
 * no such form).  Bit f - 1: form f stored, bit 4 + f - 1: form f loaded;
 *   f = 1  128-row workgroups, the 16x16x32 main loop     2  128-row workgroups, the generic main loop     3  64-row workgroups */
#define DR_PGEMM_ACC_FORM_M16 1
#define DR_PGEMM_ACC_FORM_ROWS128 2
#define DR_PGEMM_ACC_FORM_ROWS64 3
int dr_debug_pgemm_acc_forms(int clear);
/* polls before a workgroup of the single-launch Sinkhorn gives up waiting for the others (0 = the default, 2^22); the timeout test
 * sets 1 so that the first failed poll already gives up (tests/test_errors_gpu.py) */
void dr_debug_sinkhorn_spin_limit(unsigned polls);
/* the workgroup tile of dr_gemm_rows_f16 (and of the GEMMs inside dr_vit_forward_f16): -1 the automatic rule (the largest tile that still gives
 * every CU a workgroup), 0 / 1 / 2 force 64 x 64 / 128 x 64 / 128 x 128; any other value makes every launch DR_EINVAL */
void dr_debug_gemm_rows_tile(int c);
/* the workgroup tile of dr_gemm_rows_f32 (and of the GEMMs inside dr_vit_forward_f32): -1 the automatic rule of the shape (64 x 64, with
 * two k-groups of waves reduced through LDS when K >= 1024; the 128 x 128 tile is never chosen by it), 0 / 1 / 2 force 64 x 64 with 4 waves /
 * 128 x 128 with 4 waves / 64 x 64 with 8 waves and the k split; any other value makes every launch DR_EINVAL */
void dr_debug_gemm_rows_f32_tile(int c);
/* furthest-point sampling (dr_fps_nodes_f32, dr_fps_batch_f32): on != 0 makes every cloud take the streaming instantiation, whatever its
 * size, and dr_fps_workspace_bytes size the workspace for it; 0 restores the rule (on chip up to dr_fps_onchip_capacity() points) */
void dr_debug_fps_force_streaming(int on);
/* n dependent launches of an empty kernel (tools/launch_floor.py) */
int dr_debug_launch_chain(int n, int workgroups, int threads, void* stream);

/* The row and state kernels the denoise loops launch between their GEMMs (csrc/rowops.hip, csrc/stateops.hip), one launch each, for the
 * per-kernel edge tests.  Every entry checks its arguments BEFORE it launches: a refused call (DR_EINVAL / DR_ENOSUP) runs no kernel and
 * writes nothing.  All pointers are device pointers; leading dimensions and strides are in elements. */
/* out[r][c] = LayerNorm(x[r])[c] gamma[c] + beta[c] (+ res[r][c] with res != NULL, postadd == 0), or LayerNorm(x[r] + res[r]) gamma + beta with
 * postadd != 0 (res required); eps = 1e-5, r < rows, c < C <= 1024 (beyond: DR_ENOSUP).  rowmax (nullable, [rows]): max_c |out[r][c]|; with
 * postadd it must be NULL (DR_EINVAL).  C % 4 == 0 up to 768 with leading dimensions that are multiples of 4 and 16-byte aligned pointers
 * takes the float4 form, everything else the scalar one. */
int dr_debug_layernorm_f32(int rows, int C, const float* x, int ldx, const float* gamma, const float* beta, const float* res, int ldres,
                           int postadd, float* out, int ldo, float* rowmax, void* stream);
/* Fourier embedding [p | sin(2^l p), cos(2^l p) for l < L] of width (2L+1) D, zero-padded to ldo (below that width: DR_EINVAL).
 * D == 3: pts [P, rows_per_pair, 3], warped by R [P, 3, 3], t [P, 3] (both NULL: not warped) and centred on the mean of each pair's rows;
 *         warped_ws [P, rows_per_pair, 3] receives the warped, centred points and is required.
 * D == 2: pts [P rows_per_pair, 2] as they are; R, t, warped_ws are ignored.  Any other D: DR_EINVAL.  L in 0..30. */
int dr_debug_fourier_f32(int D, int P, int rows_per_pair, const float* pts, const float* R, const float* t, int L, float* emb, int ldo,
                         float* warped_ws, void* stream);
/* out[p] = min of x[p][:, :] (float64, [P, N, M]) over the entries inside both masks (uint8 [P, N] / [P, M], both NULL: all of them; a pair
 * with no such entry gives +inf).  scratch == NULL: one workgroup per pair.  scratch of dr_debug_pair_min_scratch_bytes(P) bytes whose last
 * 64 P bytes (the arrival counters) are zero: the sliced form wherever the library's rule chooses it (P <= 32 and N M >= 16384), which
 * leaves the counters zero again. */
size_t dr_debug_pair_min_scratch_bytes(int P);
int dr_debug_pair_min_f64(int P, int N, int M, const double* x, const uint8_t* src_mask, const uint8_t* tgt_mask, double* out, void* scratch,
                          void* stream);
/* one DDIM update of the state in place (the launch argument of csrc/kernels.h, field for field):
 *   x <- x0 * sqrt_an + c * ((sra * xs - x0) / srm1) [+ sigma * noise],  xs = x - shift[pair] (shift != NULL) or x
 * with the reference's dtype bookkeeping: on the first step x - shift and sigma * noise are float32 operations, x0 * sqrt_an is a float32
 * product on every step, the rest is float64.  Entries outside the masks (both NULL: none) become -inf. */
typedef struct dr_debug_ddim_args {
    double* x;
    const float* x0;
    const double* shift;
    const float* noise;
    const uint8_t* src_mask;
    const uint8_t* tgt_mask;
    int N, M, first_step;
    double sra, srm1, c, sigma;
    float sqrt_an;
} dr_debug_ddim_args;
int dr_debug_ddim_f64(const dr_debug_ddim_args* args, int P, void* stream);
/* element-wise maps of the state, n elements: kind 0 float32 -> float64 (exact), 1 float64 -> float32 (round to nearest even),
 * 2 float64 -> float64 1 / (1 + exp(-x)); any other kind: DR_EINVAL */
int dr_debug_state_map(int kind, const void* in, void* out, long long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
