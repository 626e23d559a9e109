// conv2d.hip -- the image backbone's two primitives on token rows [H W, C] float32 (NHWC with a leading dimension):
//   dr_conv2d_rows_f32   nn.Conv2d (groups = 1, zero padding, square kernel, stride, padding, dilation) of vision3d's ConvBlock
//                        (vision3d/layers/conv_block.py:118-119) as the image backbone builds it (EXP/image_backbone.py:21-57, 81-252)
//   dr_resize_rows_f32   F.interpolate(mode="bilinear", align_corners=True) (+ the sum that follows it)   EXP/image_backbone.py:263-281
// EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.
//
// The convolution is an implicit GEMM  out[m][co] = sum_kk A[m][kk] W[co][kk],  m = output pixel, kk = (tap, ci) with ci minor, on
// v_mfma_f32_32x32x2_f32 (exact fp32) with gemm.hip's staging: a tile of each operand in LDS as [rows][32 kk] (+4 pad), every lane reading 4
// consecutive kk of "its" row per ds_read_b128, register prefetch of the next chunk under the MFMAs of the current one.  A is never materialised:
// a staging slot is one (output pixel, 4-channel group of one tap) and is loaded from x with one 16-byte load -- or not at all when the tap lies
// in the zero padding, the pixel beyond the image or kk beyond K: the slot is then zero without touching memory.  Every address comes from
// conv_index.h.  Cin % 4 != 0 (the 7 x 7 stem at Cin = 1) takes a direct VALU kernel.  No atomics, one fixed accumulation order per output
// element: two runs are bit-equal.  Nothing synchronises, nothing allocates.
#include "kernels.h"
#include "conv_index.h"
#include "resize_index.h"

namespace dr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvArgs {
    ConvGeom g;
    const float* x;        // [Hi Wi, ldx]
    const float* w;        // [Cout, K] packed tap-major, ci-minor
    const float* bias;     // [Cout] or nullptr
    const float* addend;   // [Ho Wo, lda] or nullptr
    float* out;            // [Ho Wo, ldo]
    int ldx, lda, ldo;
};

constexpr int CV_BKC = 32, CV_LDT = CV_BKC + 4, CV_C4 = CV_BKC / 4, CV_NT = 256;

// 2 x 2 waves, each TM x TN MFMA tiles of 32 x 32: a workgroup owns 64 TM output pixels x 64 TN output channels.  NBUF = 2: double-buffered LDS,
// one barrier per chunk; NBUF = 1: one buffer, two barriers, half the LDS (the large tile: more workgroups per CU hide the second barrier).
// VEC = false: the scalar-load arm for base pointers or leading dimensions that are not 16-byte multiples.
// Accumulation: the MFMA chain runs over FG groups of 8 kk (4 MFMA steps each) starting from zero, and its partial sum is then added to a
// float32 total -- partial sums per k-window in ascending order.  A single chain over all of K has a rounding error that grows like sqrt(K)
// ulp of the result (measured: 4.7e-7 of max|out| at K = 144, 2-3e-6 at K = 1 152 .. 4 608); windows of m terms leave sqrt(m) from the chains
// plus one rounding per window.  FG = 1 (8 terms) for short sums, where a reference that rounds once leaves no room; FG = 4 (one k-chunk)
// for long ones, where the adds would otherwise rival the MFMAs.  The order is fixed either way: two runs are bit-equal.
template <int TM, int TN, int NBUF, int FG, bool VEC>
__global__ __launch_bounds__(CV_NT) __attribute__((amdgpu_waves_per_eu(2))) void conv2d_mfma_kernel(ConvArgs P) {
    constexpr int BM = 64 * TM, BN = 64 * TN, STAGE = (BM + BN) * CV_LDT;
    constexpr int A_SLOTS = BM * CV_C4 / CV_NT, B_SLOTS = BN * CV_C4 / CV_NT;
    __shared__ __attribute__((aligned(16))) float smem[NBUF * STAGE];

    const ConvGeom g = P.g;
    const float* __restrict__ px = P.x;
    const float* __restrict__ pw = P.w;
    const int ldx = P.ldx;
    const int tiles_n = (g.Cout + BN - 1) / BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
    const int row0 = tm * BM, col0 = tn * BN;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wn = w & 1, wm = w >> 1;
    const int nchunks = (g.K + CV_BKC - 1) / CV_BKC;

    auto fetch = [&](const float* __restrict__ base, long long off) -> float4 {
        if (off < 0) return make_float4(0.f, 0.f, 0.f, 0.f);                 // no load is issued for this slot
        if (VEC) return *reinterpret_cast<const float4*>(base + off);
        return make_float4(base[off], base[off + 1], base[off + 2], base[off + 3]);
    };
    float4 ra[A_SLOTS], rb[B_SLOTS];
    auto load_chunk = [&](int ch) {
#pragma unroll
        for (int s = 0; s < A_SLOTS; ++s) {
            const int slot = t + s * CV_NT;
            ra[s] = fetch(px, conv_a_offset(g, row0 + slot / CV_C4, ch * CV_BKC + 4 * (slot % CV_C4), ldx));
        }
#pragma unroll
        for (int s = 0; s < B_SLOTS; ++s) {
            const int slot = t + s * CV_NT;
            rb[s] = fetch(pw, conv_w_offset(g, col0 + slot / CV_C4, ch * CV_BKC + 4 * (slot % CV_C4)));
        }
    };
    auto store_chunk = [&](int ch) {
        float* As = smem + (NBUF == 2 ? (ch & 1) : 0) * STAGE;
        float* Bs = As + BM * CV_LDT;
#pragma unroll
        for (int s = 0; s < A_SLOTS; ++s) {
            const int slot = t + s * CV_NT;
            *reinterpret_cast<float4*>(As + (slot / CV_C4) * CV_LDT + 4 * (slot % CV_C4)) = ra[s];
        }
#pragma unroll
        for (int s = 0; s < B_SLOTS; ++s) {
            const int slot = t + s * CV_NT;
            *reinterpret_cast<float4*>(Bs + (slot / CV_C4) * CV_LDT + 4 * (slot % CV_C4)) = rb[s];
        }
    };

    f32x16 acc[TM][TN], tot[TM][TN], zero;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero[r] = 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) tot[i][j] = zero;

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    const int h = lane >> 5, l31 = lane & 31;
    for (int ch = 0; ch < nchunks; ++ch) {
        if (ch + 1 < nchunks) load_chunk(ch + 1);
        const float* As = smem + (NBUF == 2 ? (ch & 1) : 0) * STAGE + (wm * TM * 32 + l31) * CV_LDT + 4 * h;
        const float* Bs = smem + (NBUF == 2 ? (ch & 1) : 0) * STAGE + BM * CV_LDT + (wn * TN * 32 + l31) * CV_LDT + 4 * h;
        // lane half h takes kk = 8 gr + 4 h .. + 3 of both operands; MFMA step e multiplies element e of both fragments
#pragma unroll
        for (int gr = 0; gr < CV_BKC / 8; ++gr) {
            float4 a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const float4*>(As + i * 32 * CV_LDT + 8 * gr);
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const float4*>(Bs + j * 32 * CV_LDT + 8 * gr);
#define DR_CONV_STEP(E, C)                                                                                     \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j)             \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i].E, b[j].E, C, 0, 0, 0);
            if (gr % FG == 0) { DR_CONV_STEP(x, zero) } else { DR_CONV_STEP(x, acc[i][j]) }     // a window starts from zero
            DR_CONV_STEP(y, acc[i][j])
            DR_CONV_STEP(z, acc[i][j])
            DR_CONV_STEP(w, acc[i][j])
#undef DR_CONV_STEP
            if (gr % FG == FG - 1) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) tot[i][j] += acc[i][j];
            }
        }
        if (NBUF == 1) __syncthreads();          // single buffer: everyone is done reading before it is overwritten
        if (ch + 1 < nchunks) store_chunk(ch + 1);
        __syncthreads();
    }

    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = col0 + (wn * TN + j) * 32 + l31;
        const float bv = (P.bias && col < g.Cout) ? P.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const long long oo = conv_o_offset(g, row, col, P.ldo);
                if (oo >= 0) {
                    float v = tot[i][j][r] + bv;
                    if (P.addend) v += P.addend[conv_o_offset(g, row, col, P.lda)];
                    P.out[oo] = v;
                }
            }
    }
}

// Direct form for Cin % 4 != 0 (the stem: Cin = 1, K = 49).  A wave owns CV_DPX consecutive output pixels, a lane one output channel: the taps'
// rows are wave-uniform (scalar registers), an input value is one broadcast load, a weight is loaded once for CV_DPX multiply-adds.  Taps in
// the padding are skipped; the order of the sum is (ky, kx, ci) ascending.  The sum (and the bias) is kept in double -- a float32 product is exact
// there -- and rounded once: a short K leaves a float32 chain no room against a reference that rounds once, and this path is ~1 GFLOP of the forward.
constexpr int CV_DPX = 8;
__global__ __launch_bounds__(256) void conv2d_direct_kernel(ConvArgs P) {
    const ConvGeom g = P.g;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int m0 = (blockIdx.x * 4 + wv) * CV_DPX;
    const int co = blockIdx.y * 64 + lane;
    double acc[CV_DPX];
#pragma unroll
    for (int j = 0; j < CV_DPX; ++j) acc[j] = 0.0;
    for (int ky = 0; ky < g.k; ++ky)
        for (int kx = 0; kx < g.k; ++kx) {
            long long ao[CV_DPX];
#pragma unroll
            for (int j = 0; j < CV_DPX; ++j) ao[j] = conv_a_offset(g, m0 + j, (ky * g.k + kx) * g.Cin, P.ldx);
            for (int ci = 0; ci < g.Cin; ++ci) {
                const long long wo = conv_w_offset(g, co, (ky * g.k + kx) * g.Cin + ci);
                const double wt = wo >= 0 ? (double)P.w[wo] : 0.0;
#pragma unroll
                for (int j = 0; j < CV_DPX; ++j)
                    if (ao[j] >= 0) acc[j] = fma((double)P.x[ao[j] + ci], wt, acc[j]);
            }
        }
    const float bv = (P.bias && co < g.Cout) ? P.bias[co] : 0.f;
#pragma unroll
    for (int j = 0; j < CV_DPX; ++j) {
        const long long oo = conv_o_offset(g, m0 + j, co, P.ldo);
        if (oo >= 0) {
            float v = (float)(acc[j] + (double)bv);
            if (P.addend) v += P.addend[conv_o_offset(g, m0 + j, co, P.lda)];
            P.out[oo] = v;
        }
    }
}

// out[p][c] = addend[p][c] + bilinear(in)[p][c]: lanes along the channel, so the four source rows and the destination row are contiguous runs
__global__ __launch_bounds__(256) void resize_rows_kernel(int C, int Hs, int Ws, int Hd, int Wd, const float* __restrict__ in, int ldi,
                                                          const float* __restrict__ addend, int lda, float* __restrict__ out, int ldo) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)Hd * Wd * C) return;
    const int p = (int)(e / C), c = (int)(e % C);
    const int yd = p / Wd, xd = p - yd * Wd;
    const double sh = resize_scale(Hs, Hd), sw = resize_scale(Ws, Wd);
    int y0, y1, x0, x1;
    double ly, lx;
    resize_src(sh, yd, Hs, y0, y1, ly);
    resize_src(sw, xd, Ws, x0, x1, lx);
    const double v00 = in[(size_t)(y0 * Ws + x0) * ldi + c], v01 = in[(size_t)(y0 * Ws + x1) * ldi + c];
    const double v10 = in[(size_t)(y1 * Ws + x0) * ldi + c], v11 = in[(size_t)(y1 * Ws + x1) * ldi + c];
    float v = resize_blend(ly, lx, v00, v01, v10, v11);
    if (addend) v = addend[(size_t)p * lda + c] + v;
    out[(size_t)p * ldo + c] = v;
}

template <int TM, int TN, int NBUF, int FG>
static int launch_conv_mfma(const ConvArgs& A, bool vec, hipStream_t st) {
    const long long tiles = (long long)((A.g.Ho * A.g.Wo + 64 * TM - 1) / (64 * TM)) * ((A.g.Cout + 64 * TN - 1) / (64 * TN));
    ProfScope ps(PK_GEMM, 2.0 * A.g.Ho * A.g.Wo * A.g.Cout * A.g.K, st);
    if (vec) hipLaunchKernelGGL((conv2d_mfma_kernel<TM, TN, NBUF, FG, true>), dim3((unsigned)tiles), dim3(CV_NT), 0, st, A);
    else hipLaunchKernelGGL((conv2d_mfma_kernel<TM, TN, NBUF, FG, false>), dim3((unsigned)tiles), dim3(CV_NT), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// 128 x 128 tiles (half the operand traffic per multiply-add) once there are two of them per compute unit of an MI355X, 64 x 64 tiles below:
// a fixed count, so the same problem takes the same kernel, and sums in the same order, on every device
constexpr long long CV_LARGE_TILES = 512;
// sums of up to this many terms add their partial sums every 8 terms, longer ones every 32 (see the kernel)
constexpr int CV_SHORT_K = 1024;

}  // namespace dr

using namespace dr;

extern "C" {

int dr_conv2d_rows_f32(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation, const float* x, int ldx,
                       const float* weight, const float* bias, const float* addend, int lda, float* out, int ldo, void* stream) {
    if (Hi < 1 || Wi < 1 || Cin < 1 || Cout < 1 || k < 1 || stride < 1 || padding < 0 || dilation < 1) return DR_EINVAL;
    if (!x || !weight || !out || ldx < Cin || ldo < Cout || (addend && lda < Cout)) return DR_EINVAL;
    if ((((uintptr_t)x) | ((uintptr_t)weight) | ((uintptr_t)bias) | ((uintptr_t)addend) | ((uintptr_t)out)) & 3u) return DR_EINVAL;
    if (k > 31 || stride > 64 || padding > 1024 || dilation > 64) return DR_ENOSUP;
    if ((long long)Hi * Wi > (1ll << 24) || Cin > (1 << 16) || Cout > (1 << 16) || (long long)k * k * Cin > (1ll << 20)) return DR_ENOSUP;
    if (ldx > (1 << 20) || ldo > (1 << 20) || lda > (1 << 20)) return DR_ENOSUP;
    const ConvGeom g = conv_geom(Hi, Wi, Cin, Cout, k, stride, padding, dilation);
    if (g.Ho < 1 || g.Wo < 1) return DR_EINVAL;                                 // the dilated kernel does not fit the padded image
    if ((long long)g.Ho * g.Wo > (1ll << 24)) return DR_ENOSUP;
    ConvArgs A{g, x, weight, bias, addend, out, ldx, lda, ldo};
    const hipStream_t st = (hipStream_t)stream;
    if (Cin % 4 == 0) {
        const bool vec = ((((uintptr_t)x) | ((uintptr_t)weight)) & 15u) == 0 && ldx % 4 == 0;
        const long long large = (long long)((g.Ho * g.Wo + 127) / 128) * ((Cout + 127) / 128);
        if (g.K <= CV_SHORT_K) return launch_conv_mfma<1, 1, 2, 1>(A, vec, st);     // (the large tile has no registers for a window per group)
        return large >= CV_LARGE_TILES ? launch_conv_mfma<2, 2, 1, 4>(A, vec, st) : launch_conv_mfma<1, 1, 2, 4>(A, vec, st);
    }
    const dim3 grid((g.Ho * g.Wo + 4 * CV_DPX - 1) / (4 * CV_DPX), (Cout + 63) / 64);
    hipLaunchKernelGGL(conv2d_direct_kernel, grid, dim3(256), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_resize_rows_f32(int C, int Hs, int Ws, int Hd, int Wd, const float* in, int ldi, const float* addend, int lda, float* out, int ldo,
                       void* stream) {
    if (C < 1 || Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1) return DR_EINVAL;
    if (!in || !out || ldi < C || ldo < C || (addend && lda < C)) return DR_EINVAL;
    if ((long long)Hs * Ws > (1ll << 24) || (long long)Hd * Wd > (1ll << 24) || C > (1 << 20) || ldi > (1 << 20) || ldo > (1 << 20) ||
        lda > (1 << 20))
        return DR_ENOSUP;
    const size_t n = (size_t)Hd * Wd * C;
    if ((n + 255) / 256 > 0x7fffffffull) return DR_ENOSUP;
    resize_rows_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(C, Hs, Ws, Hd, Wd, in, ldi, addend, lda, out, ldo);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
