// kernels.h -- internal launch interface between the .hip translation units of libdiffreg_hip.
#pragma once
#include "carve.h"
#include "common.h"

namespace dr {

// ---------------------------------------------------------------------------------------------
// optional per-kernel-family timing with HIP events on the launch stream (dr_prof_* in the C ABI);
// costs one branch per launch when disabled.  Never enable inside a stream capture.
// ---------------------------------------------------------------------------------------------
enum ProfKind { PK_GEMM = 0, PK_ATTN, PK_LN, PK_PE, PK_SINKHORN, PK_PROCRUSTES, PK_STATE, PK_GEMM_SPLIT, PK_COUNT };
extern bool g_prof_on;
void prof_begin(int kind, double work, hipStream_t st);
void prof_end(int kind, hipStream_t st);
struct ProfScope {
    int kind; hipStream_t st; bool on;
    ProfScope(int k, double work, hipStream_t s) : kind(k), st(s), on(g_prof_on) { if (on) prof_begin(k, work, s); }
    ~ProfScope() { if (on) prof_end(kind, st); }
};

// ---------------------------------------------------------------------------------------------
// grouped "NT" GEMM:  out[r][c] = epi( sum_k A[r][k] * W[c][k] )   (nn.Linear without bias)
// A may be the concatenation [A | A2] along k (torch.cat([x, msg], 2) of transformero.py:91).
// ---------------------------------------------------------------------------------------------
enum { EPI_NONE = 0, EPI_RELU = 1, EPI_ROTARY = 2 };

struct GemmProblem {
    const float* A;     // [rows, K1] row-major, leading dimension lda
    const float* A2;    // [rows, K - K1] or nullptr
    const float* W;     // [ncols, K] row-major (the nn.Linear weight)
    float* out;         // [rows, ldo]
    const float* cosT;  // rotary tables [rows, C/2] (EPI_ROTARY)
    const float* sinT;
    const float* bias;  // [ncols] added before the activation (nn.Linear with bias) or nullptr
    const float* addend; // [rows, ldo] added last (e.g. tokens + embedding projection) or nullptr
    int rows, ncols, K, K1, lda, lda2, ldo;
    int epi;
    int rot_C;          // rotary: column c uses table index (c % rot_C) / 2
    float scale;        // applied last (1/sqrt(C) of matching.py:190)
    // strided batch (f32-MFMA kernels only): instance z = blockIdx.z uses A + z sA, W + z sW, out + z sO (floats)
    int nbatch;         // 0 or 1 = a single instance
    long long sA, sW, sO;
};

struct GemmBatch {
    GemmProblem p[4];
    int n;
};

int launch_gemm(const GemmBatch& g, hipStream_t st);
int gemm_configure();
int vit_f32_configure();      // vit_f32.hip: the dynamic LDS of the float32 rows GEMM's tiles
int nonrigid_configure();     // nonrigid.hip: the dynamic LDS of the non-rigid ICP solver up to its node capacity
int geo_graph_configure();    // geo_graph.hip: the dynamic LDS of the geodesic relaxation up to its on-chip capacity
void gemm_force_config(int c);
void fps_force_streaming(int on);   // fps.hip: every cloud takes the streaming instantiation (tests compare the two forms at a small size)

// ---------------------------------------------------------------------------------------------
// attention (transformero.py:79-85): segments of queries attending segments of keys
// ---------------------------------------------------------------------------------------------
struct AttnArgs {
    const float* q;       // [q_rows_total, ldq]   (rotary already applied)
    const float* k;       // [k_rows_total, ldk]
    const float* v;
    float* out;           // [q_rows_total, ldo]
    const uint8_t* qmask; // per q row (nullable = all valid)
    const uint8_t* kmask; // per k row
    int ldq, ldk, ldv, ldo;
    int H, d;             // heads, head dim (C = H*d)
    int nseg;             // number of segments
    // segment g: queries rows [q0 + g*qstride, +Lq), keys rows [k0 + g*kstride, +Lk)
    int q0, qstride, Lq, k0, kstride, Lk;
    // second family of segments (self attention over src AND tgt in one launch); nseg2 may be 0
    int nseg2, q0b, qstrideb, Lqb, k0b, kstrideb, Lkb;
    float scale;          // 1/sqrt(d)
    // plane-image output (pgemm.h) instead of `out`: rows < p_split go to pimg[0], the others (minus p_split) to pimg[1]; head h
    // occupies the k range [h p_dp, h p_dp + d) of the image (p_dp = d rounded up to 16, the pad is written as zeros);
    // bound of a query row = max over the segment's key rows of kbnd[row] * vnorm[0]  (|softmax V| <= max |V|), written to
    // pbnd[row] by the head-0 workgroups
    char* pimg[2]; int p_split, p_nct, p_dp; float* pbnd; const float* kbnd; const float* vnorm;
    // plane-image INPUT (attention_planes_kernel): q / k / v as images of p_nct chunks (head h at k = h p_dp), written by the
    // q|k|v GEMM's epilogue with the rotary embedding applied; same side split as pimg.  qbnd, kgb, vgb: bounds per token row;
    // all key rows of a segment carry ONE bound (the GEMM wrote the bound of the row's group: a pair's side), read at the
    // segment's first key row
    const char* qimg[2]; const char* kimg[2]; const char* vimg[2];
    const float* qbnd; const float* kgb; const float* vgb;
    int f16_single;       // plane-image form only: ONE fp16 product per contraction (hi planes only) -- the opt-in DR_LOOP_ATTN_F16 mode
    int xcd_groups;       // plane-image form only (set by the launcher): the query blocks of one (head, segment) run on ONE XCD -- they share its K / V
};
int launch_attention(const AttnArgs& a, hipStream_t st);
int attention_configure();
void attention_force_flash_min(int n);
void attention_force_split(int on);
// which kernel form the last launch_attention of this thread launched (host bookkeeping for the tests; DR_ATTN_FORM_* of diffreg_hip_debug.h)
int attention_last_form();

// ---------------------------------------------------------------------------------------------
// the steps both ViT encoders launch (vit.hip; the schedule is vit_forward.h): no argument checks in here, the entries make them
// ---------------------------------------------------------------------------------------------
// nn.LayerNorm of fp32 rows [rows, C] -> fp16 rows, or fp32 rows with out_f32
int launch_layernorm_rows(int rows, int C, const float* x, int ldx, const float* gamma, const float* beta, float eps, int out_f32, void* out,
                          int ldo, hipStream_t st);
// [3, H, W] image (fp16, or fp32 with img_f32) -> patch rows [(H / p)(W / p), ldo] (fp16, or fp32 with out_f32: then the image is fp32 too)
int launch_patch_rows(int H, int W, int p, const void* img, int img_f32, void* out, int out_f32, int ldo, hipStream_t st);
// the domain of dr_patch_rows_f16, and with out_f32 that of dr_patch_rows_f32
int patch_rows_check(int H, int W, int p, const void* img, const void* out, int ldo, int out_f32);
// row 0 of the stream: cls + pos[0]
int launch_cls_row(int D, const float* cls, const float* pos, float* stream_row, hipStream_t st);
// the steps of a vit_forward.h policy that do not depend on the precision
struct VitDeviceSteps {
    static int cls_row(int D, const float* cls, const float* pos, float* x, void* st) { return launch_cls_row(D, cls, pos, x, (hipStream_t)st); }
    static int copy_rows(void* dst, const void* src, size_t bytes, void* st) {
        DR_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)st));
        return DR_OK;
    }
};

// ---------------------------------------------------------------------------------------------
// row-wise ops
// ---------------------------------------------------------------------------------------------
// out[r] = (res ? res[r] : 0) + LayerNorm(x[r]) * g + b      (eps = 1e-5)
// rowmax (optional): max |out[r][:]| per row, for the consumer GEMM's operand scaling
int launch_layernorm(const float* x, int ldx, const float* g, const float* b, const float* res, int ldres, float* out,
                     int ldo, int rows, int C, hipStream_t st, float* rowmax = nullptr);
// post-LN form: out[r] = LayerNorm(x[r] + res[r]) * g + b   (vision3d AttentionLayer / AttentionOutput)
int launch_layernorm_postadd(const float* x, int ldx, const float* g, const float* b, const float* res, int ldres, float* out,
                             int ldo, int rows, int C, hipStream_t st);
// warped = R p + t per pair (R, t nullable), mean over the rows of each pair, Fourier embedding
// [p - mean | sin(2^l .), cos(2^l .)] of width (2L+1)*3 zero-padded to ldo (EXP/fusion_module.py:55-59)
int launch_fourier3d(const float* xyz, int P, int rows_per_pair, const float* R, const float* t, int L, float* emb, int ldo,
                     float* warped_ws, hipStream_t st);
// Fourier embedding of 2-D pixel coordinates, no centring (EXP/fusion_module.py:50-53)
int launch_fourier2d(const float* pix, int rows, int L, float* emb, int ldo, hipStream_t st);
// rotary tables of warped points: p' = R p + t (R,t per pair, nullable), cos/sin [rows, C/2]
int launch_vol_pe(const float* xyz, int rows, int rows_per_pair, const float* R, const float* t, int C, float ox,
                  float oy, float oz, float voxel, const float* freq, float* cosT, float* sinT, hipStream_t st, float* cs_pairs = nullptr);

// ---------------------------------------------------------------------------------------------
// top-K weighted Procrustes (procrustes.hip)
// ---------------------------------------------------------------------------------------------
// ws (optional, procrustes_workspace_bytes): lets tiles beyond 256 x 256 select their candidates with the whole chip
size_t procrustes_workspace_bytes(int P, int N, int M);
int procrustes_last_form();
int launch_procrustes(const float* conf, const float* src_pcd, const float* tgt_pcd, const uint8_t* src_mask,
                      const uint8_t* tgt_mask, int P, int N, int M, int use_mask_len, float sample_rate, float max_cond,
                      float* R, float* t, float* Rf, float* tf, double* cond, int* ok, int* topk_idx, hipStream_t st,
                      void* ws = nullptr, size_t ws_bytes = 0);

// ---------------------------------------------------------------------------------------------
// diffusion-state kernels (stateops.hip)
// ---------------------------------------------------------------------------------------------
struct DdimArgs {
    double* x;               // [P, N*M] state, updated in place
    const float* x0;         // [P, N*M] x_start of this step
    const double* shift;     // [P] per-pair minimum or nullptr
    const float* noise;      // [P, N*M] xi of this step or nullptr
    const uint8_t* src_mask; // nullable
    const uint8_t* tgt_mask;
    int N, M, first_step;
    double sra, srm1, c, sigma;
    float sqrt_an;
};
// M, sm, tm (optional): minimum over the entries inside both masks only
// (scratch: pair_min_scratch_bytes(P) bytes whose last 64 P bytes -- the arrival counters -- are zero; enables the multi-workgroup form)
int launch_pair_min(const double* x, int P, int NM, double* out, hipStream_t st, int M = 0, const uint8_t* sm = nullptr,
                    const uint8_t* tm = nullptr, void* scratch = nullptr);
size_t pair_min_scratch_bytes(int P);
int launch_ddim(const DdimArgs& a, int P, hipStream_t st);
int launch_f32_to_f64(const float* in, double* out, size_t n, hipStream_t st);
int launch_f64_to_f32(const double* in, float* out, size_t n, hipStream_t st);
int launch_sigmoid(const double* in, double* out, size_t n, hipStream_t st);
// ws (optional, top1_union_workspace_bytes): arg-maxima with the whole chip (row blocks) instead of one workgroup per pair
size_t top1_union_workspace_bytes(int P, int N, int M, size_t elt);
template <typename T>
int launch_top1_union(const T* conf, int P, int N, int M, long long* out, int* count, hipStream_t st, const uint8_t* sm = nullptr,
                      const uint8_t* tm = nullptr, void* ws = nullptr, size_t ws_bytes = 0);

// collate.hip: in-place bitonic sort of (key, value) pairs ascending by (key, value); n_pad = a power of two (pad keys ~0ull sort last)
int launch_bitonic_sort(unsigned long long* keys, unsigned* vals, int n_pad, hipStream_t st);

// item3d.hip: the targets [nt, 3] of P pairs (int32 device offsets, P + 1) sorted by (pair, cell) for the 27-cell sweep of item3d_index.h:
// origin [P] = a pair's min corner, keys / vals [next_pow2(nt)] = the sorted (key, stacked row) list, sorted [nt] = (x, y, z, stacked row)
// in key order.  A pair with bad offsets has no rows in the list.  nt = 0 launches nothing.
int launch_target_grid(int P, int nt, const float* tgt, const int* t_off, float cell, float4* origin, unsigned long long* keys, unsigned* vals,
                       float4* sorted, hipStream_t st);

// KPConv influence of a kernel point at squared distance d2 (blocks.py:304-321): mode & 3 = 0 'constant', 1 'linear', 2 'gaussian'
// (radius_gaussian with sigma = 0.3 extent, blocks.py:36-44); bit 2 of mode = aggregation 'closest' (applied by the caller: only the nearest
// kernel point of a neighbour keeps its influence, blocks.py:324-326)
enum { KP_CONSTANT = 0, KP_LINEAR = 1, KP_GAUSSIAN = 2, KP_CLOSEST = 4 };
__device__ __forceinline__ float kp_influence(int mode, float d2, float extent) {
    const int inf = mode & 3;
    if (inf == KP_LINEAR) return fmaxf(1.f - sqrtf(d2) / extent, 0.f);
    if (inf == KP_GAUSSIAN) { const float sig = extent * 0.3f; return expf(-d2 / (2.f * sig * sig + 1e-9f)); }
    return 1.f;
}

// sinkhorn.hip (internal form of dr_sinkhorn_*: `shift` = per-tile value subtracted first, nullable)
int sinkhorn_f32(int B, int N, int M, const float* scores, const uint8_t* sm, const uint8_t* tm, const float* bin_score,
                 int iters, int flags, float* out, void* ws, size_t ws_bytes, hipStream_t st, unsigned* call_status = nullptr);
int sinkhorn_f64(int B, int N, int M, const double* scores, const double* shift, const uint8_t* sm, const uint8_t* tm,
                 const float* bin_score, int iters, int flags, void* out, void* ws, size_t ws_bytes, hipStream_t st, unsigned* call_status = nullptr);
// call_status: the caller's own sticky status word (device, 4 bytes, zero-initialised by the caller): bit 0 = a co-resident Sinkhorn of THIS
// caller timed out (set beside the process-wide flag of dr_device_status, so that concurrent engines cannot swallow or misattribute a time-out)
int sinkhorn_call_status(unsigned* word, hipStream_t st, bool clear);
// device address of the process-wide sticky word dr_device_status reads (bit 1: an evaluation entry skipped an index outside its range)
unsigned* device_status_word();

}  // namespace dr
