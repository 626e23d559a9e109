// vit_f32.hip -- the float32 ViT-L/14 encoder of Depth-Anything (DPT_DINOv2.forward, depth_anything/dpt.py:155-166, runs
// self.pretrained.get_intermediate_layers(x, 4, return_class_token=True) of torchhub/facebookresearch_dinov2_main/vision_transformer.py:297-321
// in float32) in exact fp32 products: v_mfma_f32_32x32x2_f32, fp32 accumulation, one fixed k order.  DESIGN 5r.
//   dr_gemm_rows_f32      out = A W^T (+ bias) on float32 rows with four epilogues; operands staged through registers into padded LDS rows
//   dr_patch_rows_f32     the patch gather in front of the patch-embedding GEMM, float32 rows
//   dr_vit_forward_f32    the whole encoder on one stream: no host read-back, no allocation, no atomics (two runs are bit-equal)
// The schedule, its validation order and the workspace carve are vit_forward.h's, shared with vit.hip, and so are the patch-gather, class-row and
// LayerNorm kernels (vit.hip, reached through kernels.h: launch_layernorm_rows with out_f32 = 1); the attention is launch_attention
// (dr_attention_f32's dispatcher) on the packed qkv rows.
// Every global and LDS offset comes from vit_f32_index.h (tools/vit_f32_index_check.cpp walks it on the host).
#include <cstring>
#include "kernels.h"
#include "vit_f32_index.h"
#include "vit_forward.h"

namespace dr {

typedef float vf16 __attribute__((ext_vector_type(16)));
typedef float vf4 __attribute__((ext_vector_type(4)));      // (plain vector values: an array of HIP float4 structs stayed in scratch)

static int g_rows32_tile = -1;     // dr_debug_gemm_rows_f32_tile

struct GemmRows32Args {
    const float* a;
    const float* w;
    const float* bias;
    const float* gamma;
    const float* addend;
    float* out;
    int M, K, N, lda, ldw, ldo, ld_addend, mode, colscale_cols;
    float colscale;
};

// ---------------------------------------------------------------------------------------------------------------------
// The rows GEMM.  gemm.hip's main loop: the float4 slots of chunk c + 1 are fetched into registers before the fragments of chunk c are read, and
// stored into the other LDS buffer behind the MFMAs; one barrier per chunk.  Lane half h = lane >> 5 takes k = 8 g + 4 h .. + 3 of "its" row and
// MFMA step e multiplies element e of both fragments: the k order inside a group of 8 is permuted identically for A and W.  Rows past M and
// columns past N clamp to the last one on the way in and are dropped on the way out.
// ---------------------------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(T::NT) void gemm_rows_f32_kernel(GemmRows32Args A) {
    constexpr int TM = T::TM, TN = T::TN, WN = T::WN, WK = T::WK, NT = T::NT, BM = T::BM, BN = T::BN, LDT = T::LDT, STAGE = T::STAGE;
    constexpr int NA = T::NACC;
    extern __shared__ __attribute__((aligned(16))) float smem_rows32[];
    float* smem = smem_rows32;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, h = lane >> 5, l31 = lane & 31;
    const int wk = w % WK, wn = (w / WK) % WN, wm = w / (WK * WN);
    const int row0 = blockIdx.y * BM, col0 = blockIdx.x * BN;
    const int M = A.M, N = A.N, nchunks = A.K / 32;
    const float* __restrict__ pa = A.a;
    const float* __restrict__ pw = A.w;

    vf4 ra[T::A_SLOTS], rb[T::B_SLOTS];
    auto load_chunk = [&](int ch) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < T::A_SLOTS; ++s) ra[s] = *reinterpret_cast<const vf4*>(pa + vit_f32_src(M, A.lda, row0, t + s * NT, ch));
#pragma unroll
        for (int s = 0; s < T::B_SLOTS; ++s) rb[s] = *reinterpret_cast<const vf4*>(pw + vit_f32_src(N, A.ldw, col0, t + s * NT, ch));
    };
    auto store_chunk = [&](int ch) __attribute__((always_inline)) {
        float* As = smem + (ch & 1) * STAGE;
        float* Bs = As + BM * LDT;
#pragma unroll
        for (int s = 0; s < T::A_SLOTS; ++s) {
            const int slot = t + s * NT;
            *reinterpret_cast<vf4*>(As + vit_f32_lds_at(vit_f32_slot_row(slot), vit_f32_slot_k(slot))) = ra[s];
        }
#pragma unroll
        for (int s = 0; s < T::B_SLOTS; ++s) {
            const int slot = t + s * NT;
            *reinterpret_cast<vf4*>(Bs + vit_f32_lds_at(vit_f32_slot_row(slot), vit_f32_slot_k(slot))) = rb[s];
        }
    };

    vf16 acc[TM][TN][NA];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int n = 0; n < NA; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][n][r] = 0.f;

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        if (ch + 1 < nchunks) load_chunk(ch + 1);
        const float* As = smem + (ch & 1) * STAGE;
        const float* Bs = As + BM * LDT;
        vf4 a[2][TM], b[2][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[0][i] = *reinterpret_cast<const vf4*>(As + vit_f32_frag_at(wm * TM, i, l31, h, wk, T::GROUPS, 0));
#pragma unroll
        for (int j = 0; j < TN; ++j) b[0][j] = *reinterpret_cast<const vf4*>(Bs + vit_f32_frag_at(wn * TN, j, l31, h, wk, T::GROUPS, 0));
#pragma unroll
        for (int g = 0; g < T::GROUPS; ++g) {
            const int cur = g & 1, nxt = cur ^ 1;
            if (g + 1 < T::GROUPS) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    a[nxt][i] = *reinterpret_cast<const vf4*>(As + vit_f32_frag_at(wm * TM, i, l31, h, wk, T::GROUPS, g + 1));
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    b[nxt][j] = *reinterpret_cast<const vf4*>(Bs + vit_f32_frag_at(wn * TN, j, l31, h, wk, T::GROUPS, g + 1));
            }
            // consecutive MFMAs go to different accumulators (tiles, or the even / odd group pair of a single tile)
            const int q = NA == 2 ? (g & 1) : 0;
#define DR_ROWS32_STEP(E)                                                                                       \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j)              \
        acc[i][j][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i].E, b[cur][j].E, acc[i][j][q], 0, 0, 0);
            DR_ROWS32_STEP(x)
            DR_ROWS32_STEP(y)
            DR_ROWS32_STEP(z)
            DR_ROWS32_STEP(w)
#undef DR_ROWS32_STEP
        }
        if (ch + 1 < nchunks) store_chunk(ch + 1);
        __syncthreads();
    }

    if constexpr (NA == 2) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][0][r] += acc[i][j][NA - 1][r];
    }
    if (WK > 1) {
        // the WK partial tiles of each (wm, wn) meet in LDS (everybody is behind the loop's last barrier); k-group 0 adds them in the order 1 .. WK - 1
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) smem[vit_f32_red_at(w, TM, TN, i, j, r, lane)] = acc[i][j][0][r];
        __syncthreads();
        if (wk != 0) return;
#pragma unroll
        for (int o = 1; o < WK; ++o)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][0][r] += smem[vit_f32_red_at(w + o, TM, TN, i, j, r, lane)];
    }

    // ---- epilogue: register r of lane (h, l31) is row (r & 3) + 8 (r >> 2) + 4 h, column l31 of its tile
    const int mode = A.mode;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = col0 + (wn * TN + j) * 32 + l31;
        if (col >= N) continue;
        const float bv = A.bias ? A.bias[col] : 0.f;
        const float gv = (mode == DR_GEMM_ROWS32_SCALE_RESID && A.gamma) ? A.gamma[col] : 1.f;
        const float cs = (mode == DR_GEMM_ROWS32_COLSCALE && col < A.colscale_cols) ? A.colscale : 1.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + (wm * TM + i) * 32 + vit_f32_acc_row(r, h);
                if (row >= M) continue;
                float v = acc[i][j][0][r] + bv;
                float* o = A.out + vit_f32_out_at(row, A.ldo, col);
                if (mode == DR_GEMM_ROWS32_COLSCALE) v *= cs;
                else if (mode == DR_GEMM_ROWS32_GELU) v = 0.5f * v * (1.f + erff(v * 0.70710678118654752440f));
                else if (mode == DR_GEMM_ROWS32_SCALE_RESID) v = *o + gv * v;
                else if (A.addend) v += A.addend[vit_f32_out_at(row, A.ld_addend, col)];
                *o = v;
            }
    }
}

// do the float ranges [p, p + n) and [q, q + m) share an element?  (a NULL range shares nothing)
static bool overlaps(const float* p, long long n, const float* q, long long m) {
    if (!p || !q) return false;
    const uintptr_t p0 = (uintptr_t)p, p1 = p0 + (uintptr_t)n * 4, q0 = (uintptr_t)q, q1 = q0 + (uintptr_t)m * 4;
    return p0 < q1 && q0 < p1;
}

static int gemm_rows32_check(const GemmRows32Args& g) {
    if (!g.a || !g.w || !g.out || g.M < 1 || g.K < 32 || g.N < 16 || g.K % 32 || g.N % 16) return DR_EINVAL;
    if (g.mode < DR_GEMM_ROWS32_COLSCALE || g.mode > DR_GEMM_ROWS32_ADDEND) return DR_EINVAL;
    if (g.lda < g.K || g.lda % 4 || g.ldw < g.K || g.ldw % 4 || g.ldo < g.N) return DR_EINVAL;
    if (!aligned_to(g.a, 16) || !aligned_to(g.w, 16) || !aligned_to(g.out, 4) || !aligned_to(g.bias, 4) || !aligned_to(g.gamma, 4) ||
        !aligned_to(g.addend, 4))
        return DR_EINVAL;
    if (g.gamma && g.mode != DR_GEMM_ROWS32_SCALE_RESID) return DR_EINVAL;
    if (g.addend && (g.mode != DR_GEMM_ROWS32_ADDEND || g.ld_addend < g.N)) return DR_EINVAL;
    if (g.colscale_cols < 0 || g.colscale_cols > g.N || g.colscale_cols % 16 || (g.colscale_cols && g.mode != DR_GEMM_ROWS32_COLSCALE)) return DR_EINVAL;
    if ((long long)g.M * g.lda >= (1ll << 31) || (long long)g.M * g.ldo >= (1ll << 31) || (long long)g.N * g.ldw >= (1ll << 31) ||
        (g.addend && (long long)g.M * g.ld_addend >= (1ll << 31)))
        return DR_ENOSUP;
    // out shares no element with an input (in the in-place residual mode out IS the one input it may be)
    const long long no = (long long)(g.M - 1) * g.ldo + g.N;
    if (overlaps(g.out, no, g.a, (long long)(g.M - 1) * g.lda + g.K) || overlaps(g.out, no, g.w, (long long)(g.N - 1) * g.ldw + g.K) ||
        overlaps(g.out, no, g.bias, g.N) || overlaps(g.out, no, g.gamma, g.N) ||
        overlaps(g.out, no, g.addend, (long long)(g.M - 1) * g.ld_addend + g.N))
        return DR_EINVAL;
    if (g_rows32_tile < -1 || g_rows32_tile > 2) return DR_EINVAL;
    return DR_OK;
}

template <class T>
static int gemm_rows32_launch_tile(const GemmRows32Args& g, hipStream_t st) {
    hipLaunchKernelGGL((gemm_rows_f32_kernel<T>), dim3((g.N + T::BN - 1) / T::BN, (g.M + T::BM - 1) / T::BM), dim3(T::NT),
                       T::SMEM_FLOATS * sizeof(float), st, g);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

static int gemm_rows32_launch(const GemmRows32Args& g, hipStream_t st) {
    const int tile = g_rows32_tile >= 0 ? g_rows32_tile : vit_f32_tile_rule(g.M, g.K, g.N);
    if (tile == 1) return gemm_rows32_launch_tile<VitF32Tile1>(g, st);
    if (tile == 2) return gemm_rows32_launch_tile<VitF32Tile2>(g, st);
    return gemm_rows32_launch_tile<VitF32Tile0>(g, st);
}

// the 128 x 128 tile's two buffers are 72 KB of dynamic LDS: raised once, in dr_init (outside any stream capture)
int vit_f32_configure() {
    DR_HIP_CHECK(hipFuncSetAttribute((const void*)gemm_rows_f32_kernel<VitF32Tile0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(VitF32Tile0::SMEM_FLOATS * sizeof(float))));
    DR_HIP_CHECK(hipFuncSetAttribute((const void*)gemm_rows_f32_kernel<VitF32Tile1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(VitF32Tile1::SMEM_FLOATS * sizeof(float))));
    DR_HIP_CHECK(hipFuncSetAttribute((const void*)gemm_rows_f32_kernel<VitF32Tile2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(VitF32Tile2::SMEM_FLOATS * sizeof(float))));
    return DR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// vit_forward.h's policy for float32 operands: the GEMM kernel reads its two MATRICES by float4 (16 bytes) and every vector (bias, LayerScale,
// the position rows as addend) and its output by scalars (4 bytes); a take goes through the final norm here when norm_take is set
// ---------------------------------------------------------------------------------------------------------------------
struct VitF32 : VitDeviceSteps {
    typedef dr_vit_config_f32 config;
    typedef dr_vit_block_f32 block;
    enum { ELEM = 4, COLSCALE = DR_GEMM_ROWS32_COLSCALE, GELU = DR_GEMM_ROWS32_GELU, SCALE_RESID = DR_GEMM_ROWS32_SCALE_RESID, ADDEND = DR_GEMM_ROWS32_ADDEND };
    static int img_f32(const config&) { return 1; }
    static int norm_take(const config& c) { return c.norm_take; }
    static bool aligned(const config& c) {
        return aligned_to(c.workspace, 256) && aligned_to(c.x_prenorm, 16) && aligned_to(c.x_norm, 4) && aligned_to(c.pos, 4) &&
               aligned_to(c.patch_w, 16) && aligned_to(c.img, 4);
    }
    static bool aligned(const block& b) {
        return aligned_to(b.qkv_w, 16) && aligned_to(b.proj_w, 16) && aligned_to(b.fc1_w, 16) && aligned_to(b.fc2_w, 16);
    }
    static bool take_aligned(const void* p) { return aligned_to(p, 4); }
    static int patch_rows(int H, int W, int p, const void* img, int f32, void* out, int ldo, void* st) {
        return launch_patch_rows(H, W, p, img, f32, out, 1, ldo, (hipStream_t)st);
    }
    static int gemm(const void* a, int lda, int M, int K, int N, const void* w, const float* bias, int mode, void* out, int ldo, float cs, int cs_cols,
                    const float* gamma, const float* addend, int ld_addend, void* st) {
        GemmRows32Args g;
        g.a = (const float*)a; g.w = (const float*)w; g.bias = bias; g.gamma = gamma; g.addend = addend; g.out = (float*)out;
        g.M = M; g.K = K; g.N = N; g.lda = lda; g.ldw = K; g.ldo = ldo; g.ld_addend = ld_addend; g.mode = mode; g.colscale_cols = cs_cols; g.colscale = cs;
        const int rc = gemm_rows32_check(g);
        return rc != DR_OK ? rc : gemm_rows32_launch(g, (hipStream_t)st);
    }
    static int layernorm(int L, int D, const float* x, const float* g, const float* b, float eps, void* out, void* st) {
        return launch_layernorm_rows(L, D, x, D, g, b, eps, 1, out, D, (hipStream_t)st);
    }
    static int attention(int L, int heads, int D, const void* qkv_rows, void* ao, void* st) {
        const float* qkv = (const float*)qkv_rows;
        AttnArgs a;
        memset(&a, 0, sizeof(a));
        a.q = qkv; a.k = qkv + D; a.v = qkv + 2 * D; a.out = (float*)ao; a.ldq = a.ldk = a.ldv = 3 * D; a.ldo = D; a.H = heads; a.d = 64;
        a.nseg = 1; a.qstride = L; a.Lq = L; a.kstride = L; a.Lk = L; a.scale = 1.f;      // q carries d^-0.5 already
        return launch_attention(a, (hipStream_t)st);
    }
};

}  // namespace dr

using namespace dr;

extern "C" {

void dr_debug_gemm_rows_f32_tile(int c) { g_rows32_tile = c; }

int dr_gemm_rows_f32(const dr_gemm_rows_f32_args* a, void* stream) {
    if (!a) return DR_EINVAL;
    GemmRows32Args g;
    g.a = a->a; g.w = a->w; g.bias = a->bias; g.gamma = a->gamma; g.addend = a->addend; g.out = a->out;
    g.M = a->M; g.K = a->K; g.N = a->N; g.lda = a->lda; g.ldw = a->ldw; g.ldo = a->ldo; g.ld_addend = a->ld_addend; g.mode = a->mode;
    g.colscale_cols = a->colscale_cols; g.colscale = a->colscale;
    const int rc = gemm_rows32_check(g);
    return rc != DR_OK ? rc : gemm_rows32_launch(g, (hipStream_t)stream);
}

int dr_patch_rows_f32(int H, int W, int p, const float* img, float* out, int ldo, void* stream) {
    const int rc = patch_rows_check(H, W, p, img, out, ldo, 1);
    return rc != DR_OK ? rc : launch_patch_rows(H, W, p, img, 1, out, 1, ldo, (hipStream_t)stream);
}

size_t dr_vit_workspace_bytes_f32(int H, int W, int p, int D, int Dh) { return vit_workspace_bytes(H, W, p, D, Dh, VitF32::ELEM); }

int dr_vit_forward_f32(const dr_vit_config_f32* c, void* stream) { return c ? vit_forward<VitF32>(*c, stream) : DR_EINVAL; }

}  // extern "C"
