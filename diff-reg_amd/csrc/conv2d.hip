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
//
// The backward, under the same rules and with every output element written:
//   dr_conv2d_rows_backward_data_f32     the same MFMA kernel over a second slot map (BwdMap: m = input pixel, kk = (tap, co)); direct for Cout % 4 != 0
//   dr_conv2d_rows_backward_weight_f32   dW[co][kk] = sum_m G[m][co] A[m][kk] over slabs of output pixels (a function of the shape alone): float32
//                                        partial sums per slab, added in ascending order in double; grad_bias likewise; direct for Cin % 4 != 0
//   dr_resize_rows_backward_f32          the gather of resize_index.h, shared with dr_resize_tokens_backward_f32
//
// The decoder of Depth-Anything (DPTHead.forward, depth_anything/dpt.py:103-136), the same MFMA kernel with an epilogue parameter and a
// third slot map, the main loop untouched:
//   dr_conv2d_rows_act_f32               out = relu?(conv(relu?(x)) + bias) + addend + addend2: the pre-activation ResidualConvUnit and the sum of a
//                                        FeatureFusionBlock (depth_anything/blocks.py:69-92, :126-153) on the fetch and the store
//   dr_conv_transpose2d_rows_f32         nn.ConvTranspose2d with kernel = stride (dpt.py:40-51): one GEMM over TransMap, the store a pixel shuffle
//   dr_conv2d_rows_project_f32           conv -> ReLU -> 1 x 1 conv to one channel -> ReLU (dpt.py:95-99) in one launch: the hidden row of a pixel
//                                        is summed inside the workgroup, in double, in a fixed order
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
    // the DPT head's epilogues (EP != CV_EP_PLAIN); zero elsewhere
    int flags;             // DR_CONV_RELU_IN | DR_CONV_RELU_OUT
    const float* addend2;  // [Ho Wo, lda2] or nullptr, added after addend
    int lda2;
    const float* w2;       // CV_EP_PROJECT: [Cmid]
    const float* b2;       // CV_EP_PROJECT: [1] or nullptr
};

// the epilogue of conv2d_mfma_kernel.  PLAIN: + bias, + addend (every entry before the DPT head's; its code is what it was).  ACT: ReLU on A as
// it is fetched, + bias, ReLU, + addend, + addend2 (dr_conv2d_rows_act_f32).  PROJECT: + bias, ReLU, the dot product with w2 over the
// workgroup's columns, + b2, ReLU: one value per row (dr_conv2d_rows_project_f32).
constexpr int CV_EP_PLAIN = 0, CV_EP_ACT = 1, CV_EP_PROJECT = 2;

constexpr int CV_BKC = 32, CV_LDT = CV_BKC + 4, CV_C4 = CV_BKC / 4, CV_NT = 256;

// The slot map of the implicit GEMM  out[m][n] = sum_kk A[m][kk] B[n][kk]: what m, n and kk mean and where their elements live (conv_index.h).
// FwdMap: m = output pixel, n = output channel, kk = (tap, ci); A = x, B = the packed weight, out = the convolution.
// BwdMap: the roles turned (dr_conv2d_rows_backward_data_f32): m = input pixel, n = input channel, kk = (tap, co); A = grad_out read through
// conv_bwd_a_offset, B = the weight packed [Cin, k k Cout], out = grad_x.  One kernel, one main loop, two instantiations.
struct FwdMap {
    static __device__ __host__ int rows(const ConvGeom& g) { return g.Ho * g.Wo; }
    static __device__ __host__ int cols(const ConvGeom& g) { return g.Cout; }
    static __device__ __host__ int depth(const ConvGeom& g) { return g.K; }
    static __device__ long long a(const ConvGeom& g, int m, int kk, int ld) { return conv_a_offset(g, m, kk, ld); }
    static __device__ long long b(const ConvGeom& g, int n, int kk) { return conv_w_offset(g, n, kk); }
    static __device__ long long o(const ConvGeom& g, int m, int n, int ld) { return conv_o_offset(g, m, n, ld); }
    static __device__ int bias(const ConvGeom&, int n) { return n; }
};
struct BwdMap {
    static __device__ __host__ int rows(const ConvGeom& g) { return g.Hi * g.Wi; }
    static __device__ __host__ int cols(const ConvGeom& g) { return g.Cin; }
    static __device__ __host__ int depth(const ConvGeom& g) { return conv_bwd_k(g); }
    static __device__ long long a(const ConvGeom& g, int m, int kk, int ld) { return conv_bwd_a_offset(g, m, kk, ld); }
    static __device__ long long b(const ConvGeom& g, int n, int kk) { return conv_bwd_w_offset(g, n, kk); }
    static __device__ long long o(const ConvGeom& g, int m, int n, int ld) { return conv_bwd_o_offset(g, m, n, ld); }
    static __device__ int bias(const ConvGeom&, int n) { return n; }
};
// TransMap: nn.ConvTranspose2d with kernel = stride (dr_conv_transpose2d_rows_f32): m = input pixel, n = (i, j, co), kk = ci; A = x, B = the weight
// packed [s s Cout, Cin]; the store is a pixel shuffle and the bias is per co.
struct TransMap {
    static __device__ __host__ int rows(const ConvGeom& g) { return g.Hi * g.Wi; }
    static __device__ __host__ int cols(const ConvGeom& g) { return conv_t_cols(g); }
    static __device__ __host__ int depth(const ConvGeom& g) { return g.Cin; }
    static __device__ long long a(const ConvGeom& g, int m, int kk, int ld) { return conv_t_a_offset(g, m, kk, ld); }
    static __device__ long long b(const ConvGeom& g, int n, int kk) { return conv_t_w_offset(g, n, kk); }
    static __device__ long long o(const ConvGeom& g, int m, int n, int ld) { return conv_t_o_offset(g, m, n, ld); }
    static __device__ int bias(const ConvGeom& g, int n) { return conv_t_channel(g, n); }
};

// 2 x 2 waves, each TM x TN MFMA tiles of 32 x 32: a workgroup owns 64 TM output pixels x 64 TN output channels.  NBUF = 2: double-buffered LDS,
// one barrier per chunk; NBUF = 1: one buffer, two barriers, half the LDS (the large tile: more workgroups per CU hide the second barrier).
// VEC = false: the scalar-load arm for base pointers or leading dimensions that are not 16-byte multiples.
// Accumulation: the MFMA chain runs over FG groups of 8 kk (4 MFMA steps each) starting from zero, and its partial sum is then added to a
// float32 total -- partial sums per k-window in ascending order.  A single chain over all of K has a rounding error that grows like sqrt(K)
// ulp of the result (measured: 4.7e-7 of max|out| at K = 144, 2-3e-6 at K = 1 152 .. 4 608); windows of m terms leave sqrt(m) from the chains
// plus one rounding per window.  FG = 1 (8 terms) for short sums, where a reference that rounds once leaves no room; FG = 4 (one k-chunk)
// for long ones, where the adds would otherwise rival the MFMAs.  The order is fixed either way: two runs are bit-equal.
template <class MAP, int TM, int TN, int NBUF, int FG, bool VEC, int EP>
__global__ __launch_bounds__(CV_NT) __attribute__((amdgpu_waves_per_eu(2))) void conv2d_mfma_kernel(ConvArgs P) {
    static_assert(EP != CV_EP_PROJECT || TN == 1, "the project epilogue sums one 64-wide column tile");
    constexpr int BM = 64 * TM, BN = 64 * TN, STAGE = (BM + BN) * CV_LDT;
    constexpr int A_SLOTS = BM * CV_C4 / CV_NT, B_SLOTS = BN * CV_C4 / CV_NT;
    __shared__ __attribute__((aligned(16))) float smem[NBUF * STAGE];

    const ConvGeom g = P.g;
    const float* __restrict__ px = P.x;
    const float* __restrict__ pw = P.w;
    const int ldx = P.ldx;
    const int tiles_n = (MAP::cols(g) + BN - 1) / BN;
    const int tm = blockIdx.x / tiles_n, tn = blockIdx.x % tiles_n;
    const int row0 = tm * BM, col0 = tn * BN;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wn = w & 1, wm = w >> 1;
    const int nchunks = (MAP::depth(g) + CV_BKC - 1) / CV_BKC;

    auto fetch = [&](const float* __restrict__ base, long long off) -> float4 {
        if (off < 0) return make_float4(0.f, 0.f, 0.f, 0.f);                 // no load is issued for this slot
        if (VEC) return *reinterpret_cast<const float4*>(base + off);
        return make_float4(base[off], base[off + 1], base[off + 2], base[off + 3]);
    };
    float4 ra[A_SLOTS], rb[B_SLOTS];
    const bool relu_in = EP == CV_EP_ACT && (P.flags & DR_CONV_RELU_IN);
    auto load_chunk = [&](int ch) {
#pragma unroll
        for (int s = 0; s < A_SLOTS; ++s) {
            const int slot = t + s * CV_NT;
            ra[s] = fetch(px, MAP::a(g, row0 + slot / CV_C4, ch * CV_BKC + 4 * (slot % CV_C4), ldx));
            if (EP == CV_EP_ACT && relu_in)                     // (a slot that loaded nothing is zero and stays zero)
                ra[s] = make_float4(fmaxf(ra[s].x, 0.f), fmaxf(ra[s].y, 0.f), fmaxf(ra[s].z, 0.f), fmaxf(ra[s].w, 0.f));
        }
#pragma unroll
        for (int s = 0; s < B_SLOTS; ++s) {
            const int slot = t + s * CV_NT;
            rb[s] = fetch(pw, MAP::b(g, col0 + slot / CV_C4, ch * CV_BKC + 4 * (slot % CV_C4)));
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

    if (EP == CV_EP_PROJECT) {
        // One value per output pixel: sum over the Cmid <= 64 columns of relu(acc + b1) w2.  A row's columns lie across the 32 lanes of a lane
        // half of wave wn = 0 and, above 32, of wave wn = 1.  The products are formed in double (exact) and added in double: a butterfly over
        // lane distances 16, 8, 4, 2, 1 (every lane of the half ends with the same bits), then wave 1's sum reaches wave 0 through LDS and the
        // total is (s0 + s1) + b2, rounded once.  The order is fixed.  The staging buffers are free: the main loop ended on a barrier.
        double* red = reinterpret_cast<double*>(smem);
        const int col = wn * 32 + l31;                                    // tiles_n == 1: col0 == 0
        const bool live = col < MAP::cols(g);
        const float bv = (P.bias && live) ? P.bias[col] : 0.f;
        const double w2 = live ? (double)P.w2[col] : 0.0;
        double sum[TM][16];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                double v = (double)fmaxf(tot[i][0][r] + bv, 0.f) * w2;
#pragma unroll
                for (int dist = 16; dist >= 1; dist >>= 1) v += __shfl_xor(v, dist);
                sum[i][r] = v;
            }
        if (wn == 1 && l31 == 0) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[conv_tile_row(wm * TM + i, r, h)] = sum[i][r];
        }
        __syncthreads();
        if (wn == 0 && l31 == 0) {
            const double b2 = P.b2 ? (double)P.b2[0] : 0.0;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int lr = conv_tile_row(wm * TM + i, r, h);
                    const long long oo = conv_p_o_offset(g, row0 + lr, P.ldo);
                    if (oo >= 0) {
                        float v = (float)((sum[i][r] + red[lr]) + b2);
                        if (P.flags & DR_CONV_RELU_OUT) v = fmaxf(v, 0.f);
                        P.out[oo] = v;
                    }
                }
        }
        return;
    }

    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = col0 + (wn * TN + j) * 32 + l31;
        const float bv = (P.bias && col < MAP::cols(g)) ? P.bias[MAP::bias(g, col)] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = row0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const long long oo = MAP::o(g, row, col, P.ldo);
                if (oo >= 0) {
                    float v = tot[i][j][r] + bv;
                    if (EP == CV_EP_ACT && (P.flags & DR_CONV_RELU_OUT)) v = fmaxf(v, 0.f);          // after the bias, before the addends
                    if (P.addend) v += P.addend[MAP::o(g, row, col, P.lda)];
                    if (EP == CV_EP_ACT && P.addend2) v += P.addend2[MAP::o(g, row, col, P.lda2)];
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

// 128 x 128 tiles (half the operand traffic per multiply-add) once there are two of them per compute unit of an MI355X, 64 x 64 tiles below:
// a fixed count, so the same problem takes the same kernel, and sums in the same order, on every device
constexpr long long CV_LARGE_TILES = 512;
// sums of up to this many terms add their partial sums every 8 terms, longer ones every 32 (see the kernel)
constexpr int CV_SHORT_K = 1024;

template <class MAP, int TM, int TN, int NBUF, int FG, int EP = CV_EP_PLAIN>
static int launch_conv_mfma(const ConvArgs& A, bool vec, hipStream_t st) {
    const long long tiles = (long long)((MAP::rows(A.g) + 64 * TM - 1) / (64 * TM)) * ((MAP::cols(A.g) + 64 * TN - 1) / (64 * TN));
    ProfScope ps(PK_GEMM, 2.0 * MAP::rows(A.g) * MAP::cols(A.g) * MAP::depth(A.g), st);
    if (vec) hipLaunchKernelGGL((conv2d_mfma_kernel<MAP, TM, TN, NBUF, FG, true, EP>), dim3((unsigned)tiles), dim3(CV_NT), 0, st, A);
    else hipLaunchKernelGGL((conv2d_mfma_kernel<MAP, TM, TN, NBUF, FG, false, EP>), dim3((unsigned)tiles), dim3(CV_NT), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// the tile and window choice of every implicit GEMM: rows x cols x depth of the map
template <class MAP, int EP = CV_EP_PLAIN>
static int dispatch_conv_mfma(const ConvArgs& A, bool vec, hipStream_t st) {
    const long long large = (long long)((MAP::rows(A.g) + 127) / 128) * ((MAP::cols(A.g) + 127) / 128);
    if (MAP::depth(A.g) <= CV_SHORT_K) return launch_conv_mfma<MAP, 1, 1, 2, 1, EP>(A, vec, st);     // (the large tile has no registers for a window per group)
    return large >= CV_LARGE_TILES ? launch_conv_mfma<MAP, 2, 2, 1, 4, EP>(A, vec, st) : launch_conv_mfma<MAP, 1, 1, 2, 4, EP>(A, vec, st);
}

// The project entry: its Cmid <= 64 columns are ONE 64-wide column tile, which the epilogue sums inside the workgroup, so the 128 x 128 tile
// does not apply; the window rule is the one above.  (Cmid = 32 leaves wave column 1 multiplying zeros: a 32-wide geometry with the four waves
// along m was not built -- DESIGN 5q.)
static int dispatch_conv_project(const ConvArgs& A, bool vec, hipStream_t st) {
    if (FwdMap::depth(A.g) <= CV_SHORT_K) return launch_conv_mfma<FwdMap, 1, 1, 2, 1, CV_EP_PROJECT>(A, vec, st);
    return launch_conv_mfma<FwdMap, 1, 1, 2, 4, CV_EP_PROJECT>(A, vec, st);
}

// [p, p + n) and [q, q + m) share an element
static bool cv_overlap(const float* p, long long n, const float* q, long long m) { return p && q && p < q + m && q < p + n; }
// the extent in floats of rows [R, ld] of C columns
static long long cv_extent(long long R, int ld, int C) { return (R - 1) * ld + C; }


// ---- the backward ---------------------------------------------------------------------------------------------------------------------

// Data gradient, direct form for Cout % 4 != 0: a thread owns one (input pixel, input channel), lanes along the channel; the sum runs over
// (ky, kx, co) ascending in double and is rounded once.  Taps without an output pixel are skipped.
__global__ __launch_bounds__(256) void conv2d_dgrad_direct_kernel(ConvArgs P) {
    const ConvGeom g = P.g;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int m = (int)(e / g.Cin), ci = (int)(e - (long long)m * g.Cin);
    const long long oo = conv_bwd_o_offset(g, m, ci, P.ldo);
    if (oo < 0) return;
    double acc = 0.0;
    for (int tap = 0; tap < g.k * g.k; ++tap) {
        const long long ao = conv_bwd_a_offset(g, m, tap * g.Cout, P.ldx);
        if (ao < 0) continue;
        for (int co = 0; co < g.Cout; ++co) acc = fma((double)P.x[ao + co], (double)P.w[conv_bwd_w_offset(g, ci, tap * g.Cout + co)], acc);
    }
    float v = (float)acc;
    if (P.addend) v += P.addend[conv_bwd_o_offset(g, m, ci, P.lda)];
    P.out[oo] = v;
}

struct WgradArgs {
    ConvGeom g;
    ConvSlabs sl;
    const float* x;        // [Hi Wi, ldx]
    const float* go;       // grad_out [Ho Wo, ldg]
    float* part;           // [S, Cout, K] float32 partial sums
    double* bpart;         // [S, Cout] double partial sums of grad_bias
    float* gw;             // [Cout, K] or nullptr
    float* gb;             // [Cout] or nullptr
    int ldx, ldg;
};

// Weight gradient  dW[co][kk] = sum_m G[m][co] A[m][kk]  on v_mfma_f32_32x32x2_f32.  A workgroup owns one (64 output channels, 64 positions kk,
// slab of output pixels); 2 x 2 waves of one 32 x 32 tile.  Both operands have the REDUCTION index m as their row, so a chunk of CV_WG_CHUNK = 32
// pixels is staged as [m][64 co] and [m][64 kk] and the lanes that read one k-step of the MFMA (lane half h takes pixel 2 e + h, lane & 31 the
// channel / position) touch consecutive words: no transpose.  The A slots are the forward's: one (output pixel, 4-channel group of a tap) per
// 16-byte load through conv_a_offset, or nothing for a tap in the padding.  The row stride 96 puts the two lane halves 32 banks apart.
// Accumulation: the MFMA chain runs over windows of 8 pixels from zero, each window is added to a float32 total (the forward's FG = 1 rule);
// the total of the slab is written to the workspace and wgrad_reduce_kernel adds the slabs in ascending order in double.
constexpr int WG_BT = 64, WG_LDW = WG_BT + 32, WG_Q = WG_BT / 4, WG_SLOTS = CV_WG_CHUNK * WG_Q / CV_NT, WG_STAGE = 2 * CV_WG_CHUNK * WG_LDW;
template <bool VEC>
__global__ __launch_bounds__(CV_NT) void conv2d_wgrad_mfma_kernel(WgradArgs P) {
    __shared__ __attribute__((aligned(16))) float smem[2 * WG_STAGE];
    const ConvGeom g = P.g;
    const ConvSlabs sl = P.sl;
    const float* __restrict__ px = P.x;
    const float* __restrict__ pg = P.go;
    const int ldx = P.ldx, ldg = P.ldg;
    const int tiles_k = (g.K + WG_BT - 1) / WG_BT, tiles_c = (g.Cout + WG_BT - 1) / WG_BT;
    const int tk = blockIdx.x % tiles_k, tc = (blockIdx.x / tiles_k) % tiles_c, slab = blockIdx.x / (tiles_k * tiles_c);
    const int co0 = tc * WG_BT, kk0 = tk * WG_BT;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wn = w & 1, wm = w >> 1;
    const int nchunks = sl.L / CV_WG_CHUNK;

    float4 ra[WG_SLOTS], rg[WG_SLOTS];
    auto load_chunk = [&](int ch) {
#pragma unroll
        for (int s = 0; s < WG_SLOTS; ++s) {
            const int slot = t + s * CV_NT;
            const int m = conv_slab_pixel(g, sl, slab, ch * CV_WG_CHUNK + slot / WG_Q), c4 = 4 * (slot % WG_Q);
            const long long ao = m < 0 ? -1 : conv_a_offset(g, m, kk0 + c4, ldx);
            if (ao < 0) ra[s] = make_float4(0.f, 0.f, 0.f, 0.f);
            else if (VEC) ra[s] = *reinterpret_cast<const float4*>(px + ao);
            else ra[s] = make_float4(px[ao], px[ao + 1], px[ao + 2], px[ao + 3]);
            if (VEC) {                                                               // Cout % 4 == 0: the group is inside the row whenever its first element is
                const long long o = m < 0 ? -1 : conv_o_offset(g, m, co0 + c4, ldg);
                rg[s] = o < 0 ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(pg + o);
            } else {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long long o = m < 0 ? -1 : conv_o_offset(g, m, co0 + c4 + e, ldg);
                    v[e] = o < 0 ? 0.f : pg[o];
                }
                rg[s] = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    };
    auto store_chunk = [&](int ch) {
        float* Gs = smem + (ch & 1) * WG_STAGE;
        float* As = Gs + CV_WG_CHUNK * WG_LDW;
#pragma unroll
        for (int s = 0; s < WG_SLOTS; ++s) {
            const int slot = t + s * CV_NT;
            *reinterpret_cast<float4*>(Gs + (slot / WG_Q) * WG_LDW + 4 * (slot % WG_Q)) = rg[s];
            *reinterpret_cast<float4*>(As + (slot / WG_Q) * WG_LDW + 4 * (slot % WG_Q)) = ra[s];
        }
    };

    f32x16 acc, tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] = 0.f, acc[r] = 0.f;
    const f32x16 zero = tot;
    const int h = lane >> 5, l31 = lane & 31;
    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        if (ch + 1 < nchunks) load_chunk(ch + 1);
        const float* Gs = smem + (ch & 1) * WG_STAGE + h * WG_LDW + wm * 32 + l31;
        const float* As = smem + (ch & 1) * WG_STAGE + CV_WG_CHUNK * WG_LDW + h * WG_LDW + wn * 32 + l31;
#pragma unroll
        for (int e = 0; e < CV_WG_CHUNK / 2; ++e) {
            const float a = Gs[2 * e * WG_LDW], b = As[2 * e * WG_LDW];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, (e % 4 == 0) ? zero : acc, 0, 0, 0);      // a window of 8 pixels starts from zero
            if (e % 4 == 3) tot += acc;
        }
        if (ch + 1 < nchunks) store_chunk(ch + 1);           // the other buffer: its readers passed the barrier below one chunk ago
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31 (the position kk), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (the output channel)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long o = conv_wg_part_offset(g, sl, slab, co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, kk0 + wn * 32 + l31);
        if (o >= 0) P.part[o] = tot[r];
    }
}

// Weight gradient, direct form for Cin % 4 != 0 (the stem: K = 49): a thread owns one (output channel, position kk) of one slab and sums the
// slab's pixels in ascending order in double; the same partials, the same second pass.
__global__ __launch_bounds__(256) void conv2d_wgrad_direct_kernel(WgradArgs P) {
    const ConvGeom g = P.g;
    const ConvSlabs sl = P.sl;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int slab = blockIdx.y, co = (int)(e / g.K), kk = (int)(e - (long long)co * g.K);
    const long long po = conv_wg_part_offset(g, sl, slab, co, kk);
    if (po < 0) return;
    double acc = 0.0;
    for (int j = 0; j < sl.L; ++j) {
        const int m = conv_slab_pixel(g, sl, slab, j);
        if (m < 0) break;
        const long long ao = conv_a_offset(g, m, kk, P.ldx);
        if (ao >= 0) acc = fma((double)P.go[conv_o_offset(g, m, co, P.ldg)], (double)P.x[ao], acc);
    }
    P.part[po] = (float)acc;
}

// grad_bias partials: the column sums of grad_out over one slab.  Lanes along the channel; the four waves take the slab's pixels j = wave, wave + 4,
// ... in ascending order in double and are then added in wave order.
__global__ __launch_bounds__(256) void conv2d_bias_partial_kernel(WgradArgs P) {
    __shared__ double red[4][64];
    const ConvGeom g = P.g;
    const ConvSlabs sl = P.sl;
    const int slab = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, co = blockIdx.x * 64 + lane;
    double acc = 0.0;
    for (int j = wv; j < sl.L; j += 4) {
        const int m = conv_slab_pixel(g, sl, slab, j);
        const long long o = m < 0 ? -1 : conv_o_offset(g, m, co, P.ldg);
        if (o >= 0) acc += (double)P.go[o];
    }
    red[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && co < g.Cout) P.bpart[(size_t)slab * g.Cout + co] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// the second pass: element e < Cout K of grad_w, then element e - Cout K of grad_bias; slabs in ascending order in double, rounded once
__global__ __launch_bounds__(256) void conv2d_wgrad_reduce_kernel(WgradArgs P) {
    const ConvGeom g = P.g;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, nw = (long long)g.Cout * g.K;
    if (e < nw) {
        if (!P.gw) return;
        const int co = (int)(e / g.K), kk = (int)(e - (long long)co * g.K);
        double acc = 0.0;
        for (int s = 0; s < P.sl.S; ++s) acc += (double)P.part[conv_wg_part_offset(g, P.sl, s, co, kk)];
        P.gw[conv_w_offset(g, co, kk)] = (float)acc;
    } else if (e < nw + g.Cout && P.gb) {
        const int co = (int)(e - nw);
        double acc = 0.0;
        for (int s = 0; s < P.sl.S; ++s) acc += P.bpart[(size_t)s * g.Cout + co];
        P.gb[co] = (float)acc;
    }
}

// grad_in[s][c] = the sum over the destination pixels whose footprint holds source texel s (resize_gather: the statement shared with
// dr_resize_tokens_backward_f32): lanes along the channel
__global__ __launch_bounds__(256) void resize_rows_backward_kernel(int C, int Hs, int Ws, int Hd, int Wd, const float* __restrict__ g, int ldg,
                                                                   float* __restrict__ grad_in, int ldgi) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)Hs * Ws * C) return;
    const int s = (int)(e / C), c = (int)(e % C);
    const int ys = s / Ws, xs = s - ys * Ws;
    const double acc = resize_gather(resize_scale(Hs, Hd), resize_scale(Ws, Wd), ys, xs, Hs, Ws, Hd, Wd,
                                     [&](int pd) { return g[(size_t)pd * ldg + c]; });
    grad_in[(size_t)s * ldgi + c] = (float)acc;
}

// the geometry checks of the two gradients (the forward entry's, and k k Cout as well): DR_OK, DR_EINVAL or DR_ENOSUP, and the geometry
static int conv_check_geom(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation, ConvGeom& g) {
    if (Hi < 1 || Wi < 1 || Cin < 1 || Cout < 1 || k < 1 || stride < 1 || padding < 0 || dilation < 1) return DR_EINVAL;
    if (k > 31 || stride > 64 || padding > 1024 || dilation > 64) return DR_ENOSUP;
    if ((long long)Hi * Wi > (1ll << 24) || Cin > (1 << 16) || Cout > (1 << 16) || (long long)k * k * Cin > (1ll << 20) ||
        (long long)k * k * Cout > (1ll << 20))
        return DR_ENOSUP;
    g = conv_geom(Hi, Wi, Cin, Cout, k, stride, padding, dilation);
    if (g.Ho < 1 || g.Wo < 1) return DR_EINVAL;
    if ((long long)g.Ho * g.Wo > (1ll << 24)) return DR_ENOSUP;
    return DR_OK;
}

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
        return dispatch_conv_mfma<FwdMap>(A, vec, st);
    }
    const dim3 grid((g.Ho * g.Wo + 4 * CV_DPX - 1) / (4 * CV_DPX), (Cout + 63) / 64);
    hipLaunchKernelGGL(conv2d_direct_kernel, grid, dim3(256), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_conv2d_rows_act_f32(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation, const float* x, int ldx,
                           const float* weight, const float* bias, int flags, const float* addend, int lda, const float* addend2, int lda2,
                           float* out, int ldo, void* stream) {
    if (Hi < 1 || Wi < 1 || Cin < 1 || Cout < 1 || k < 1 || stride < 1 || padding < 0 || dilation < 1) return DR_EINVAL;
    if (!x || !weight || !out || ldx < Cin || ldo < Cout || (addend && lda < Cout) || (addend2 && lda2 < Cout)) return DR_EINVAL;
    if (flags & ~(DR_CONV_RELU_IN | DR_CONV_RELU_OUT)) return DR_EINVAL;
    if ((((uintptr_t)x) | ((uintptr_t)weight) | ((uintptr_t)bias) | ((uintptr_t)addend) | ((uintptr_t)addend2) | ((uintptr_t)out)) & 3u) return DR_EINVAL;
    if (k > 31 || stride > 64 || padding > 1024 || dilation > 64) return DR_ENOSUP;
    if ((long long)Hi * Wi > (1ll << 24) || Cin > (1 << 16) || Cout > (1 << 16) || (long long)k * k * Cin > (1ll << 20)) return DR_ENOSUP;
    if (ldx > (1 << 20) || ldo > (1 << 20) || lda > (1 << 20) || lda2 > (1 << 20)) return DR_ENOSUP;
    const ConvGeom g = conv_geom(Hi, Wi, Cin, Cout, k, stride, padding, dilation);
    if (g.Ho < 1 || g.Wo < 1) return DR_EINVAL;
    if ((long long)g.Ho * g.Wo > (1ll << 24)) return DR_ENOSUP;
    const long long M = (long long)g.Ho * g.Wo, no = cv_extent(M, ldo, Cout);
    if (cv_overlap(out, no, x, cv_extent((long long)Hi * Wi, ldx, Cin)) || cv_overlap(out, no, weight, (long long)Cout * g.K) ||
        cv_overlap(out, no, bias, Cout) || cv_overlap(out, no, addend, cv_extent(M, lda, Cout)) ||
        cv_overlap(out, no, addend2, cv_extent(M, lda2, Cout)))
        return DR_EINVAL;
    ConvArgs A{g, x, weight, bias, addend, out, ldx, lda, ldo, flags, addend2, lda2, nullptr, nullptr};
    const hipStream_t st = (hipStream_t)stream;
    if (Cin % 4 == 0) {
        const bool vec = ((((uintptr_t)x) | ((uintptr_t)weight)) & 15u) == 0 && ldx % 4 == 0;
        return dispatch_conv_mfma<FwdMap, CV_EP_ACT>(A, vec, st);
    }
    if (flags || addend2) return DR_ENOSUP;                                    // the direct arm has no flags
    const dim3 grid((g.Ho * g.Wo + 4 * CV_DPX - 1) / (4 * CV_DPX), (Cout + 63) / 64);
    hipLaunchKernelGGL(conv2d_direct_kernel, grid, dim3(256), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_conv_transpose2d_rows_f32(int H, int W, int Cin, int Cout, int s, const float* x, int ldx, const float* weight, const float* bias, float* out,
                                 int ldo, void* stream) {
    if (H < 1 || W < 1 || Cin < 1 || Cout < 1 || s < 1) return DR_EINVAL;
    if (!x || !weight || !out || ldx < Cin || ldo < Cout) return DR_EINVAL;
    if ((((uintptr_t)x) | ((uintptr_t)weight) | ((uintptr_t)bias) | ((uintptr_t)out)) & 3u) return DR_EINVAL;
    if (s > 8 || Cin % 4 != 0 || Cin > (1 << 16) || (long long)s * s * Cout > (1ll << 16)) return DR_ENOSUP;
    if ((long long)H * s * W * s > (1ll << 24) || ldx > (1 << 20) || ldo > (1 << 20)) return DR_ENOSUP;
    const ConvGeom g = conv_t_geom(H, W, Cin, Cout, s);
    const long long no = cv_extent((long long)g.Ho * g.Wo, ldo, Cout);
    if (cv_overlap(out, no, x, cv_extent((long long)H * W, ldx, Cin)) || cv_overlap(out, no, weight, (long long)conv_t_cols(g) * Cin) ||
        cv_overlap(out, no, bias, Cout))
        return DR_EINVAL;
    ConvArgs A{g, x, weight, bias, nullptr, out, ldx, 0, ldo, 0, nullptr, 0, nullptr, nullptr};
    const bool vec = ((((uintptr_t)x) | ((uintptr_t)weight)) & 15u) == 0 && ldx % 4 == 0;
    return dispatch_conv_mfma<TransMap>(A, vec, (hipStream_t)stream);
}

int dr_conv2d_rows_project_f32(int Hi, int Wi, int Cin, int Cmid, int k, int stride, int padding, int dilation, const float* x, int ldx,
                               const float* w1, const float* b1, const float* w2, const float* b2, int relu_out, float* out, int ldo, void* stream) {
    if (Hi < 1 || Wi < 1 || Cin < 1 || Cmid < 1 || k < 1 || stride < 1 || padding < 0 || dilation < 1) return DR_EINVAL;
    if (!x || !w1 || !w2 || !out || ldx < Cin || ldo < 1) return DR_EINVAL;
    if ((((uintptr_t)x) | ((uintptr_t)w1) | ((uintptr_t)b1) | ((uintptr_t)w2) | ((uintptr_t)b2) | ((uintptr_t)out)) & 3u) return DR_EINVAL;
    if (k > 31 || stride > 64 || padding > 1024 || dilation > 64) return DR_ENOSUP;
    if (Cmid > 64 || Cin % 4 != 0) return DR_ENOSUP;
    if ((long long)Hi * Wi > (1ll << 24) || Cin > (1 << 16) || (long long)k * k * Cin > (1ll << 20)) return DR_ENOSUP;
    if (ldx > (1 << 20) || ldo > (1 << 20)) return DR_ENOSUP;
    const ConvGeom g = conv_geom(Hi, Wi, Cin, Cmid, k, stride, padding, dilation);
    if (g.Ho < 1 || g.Wo < 1) return DR_EINVAL;
    if ((long long)g.Ho * g.Wo > (1ll << 24)) return DR_ENOSUP;
    const long long no = cv_extent((long long)g.Ho * g.Wo, ldo, 1);
    if (cv_overlap(out, no, x, cv_extent((long long)Hi * Wi, ldx, Cin)) || cv_overlap(out, no, w1, (long long)Cmid * g.K) ||
        cv_overlap(out, no, b1, Cmid) || cv_overlap(out, no, w2, Cmid) || cv_overlap(out, no, b2, 1))
        return DR_EINVAL;
    ConvArgs A{g, x, w1, b1, nullptr, out, ldx, 0, ldo, relu_out ? DR_CONV_RELU_OUT : 0, nullptr, 0, w2, b2};
    const bool vec = ((((uintptr_t)x) | ((uintptr_t)w1)) & 15u) == 0 && ldx % 4 == 0;
    return dispatch_conv_project(A, vec, (hipStream_t)stream);
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

int dr_conv2d_rows_backward_data_f32(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation, const float* grad_out, int ldg,
                                     const float* weight_t, const float* addend, int lda, float* grad_x, int ldgx, void* stream) {
    ConvGeom g;
    if (Hi < 1 || Wi < 1 || Cin < 1 || Cout < 1) return DR_EINVAL;
    if (!grad_out || !weight_t || !grad_x || ldg < Cout || ldgx < Cin || (addend && lda < Cin)) return DR_EINVAL;
    if ((((uintptr_t)grad_out) | ((uintptr_t)weight_t) | ((uintptr_t)addend) | ((uintptr_t)grad_x)) & 3u) return DR_EINVAL;
    const int rc = conv_check_geom(Hi, Wi, Cin, Cout, k, stride, padding, dilation, g);
    if (rc != DR_OK) return rc;
    if (ldg > (1 << 20) || ldgx > (1 << 20) || lda > (1 << 20)) return DR_ENOSUP;
    ConvArgs A{g, grad_out, weight_t, nullptr, addend, grad_x, ldg, lda, ldgx};
    const hipStream_t st = (hipStream_t)stream;
    if (Cout % 4 == 0) {
        const bool vec = ((((uintptr_t)grad_out) | ((uintptr_t)weight_t)) & 15u) == 0 && ldg % 4 == 0;
        return dispatch_conv_mfma<BwdMap>(A, vec, st);
    }
    const long long n = (long long)Hi * Wi * Cin;
    if ((n + 255) / 256 > 0x7fffffffll) return DR_ENOSUP;
    hipLaunchKernelGGL(conv2d_dgrad_direct_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_conv2d_rows_backward_weight_workspace_bytes(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation) {
    ConvGeom g;
    if (conv_check_geom(Hi, Wi, Cin, Cout, k, stride, padding, dilation, g) != DR_OK) return 0;
    return (size_t)conv_wg_workspace_bytes(g, conv_wgrad_slabs(g.Ho * g.Wo));
}

int dr_conv2d_rows_backward_weight_f32(int Hi, int Wi, int Cin, int Cout, int k, int stride, int padding, int dilation, const float* x, int ldx,
                                       const float* grad_out, int ldg, float* grad_w, float* grad_bias, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    ConvGeom g;
    if (Hi < 1 || Wi < 1 || Cin < 1 || Cout < 1) return DR_EINVAL;
    if (!x || !grad_out || !workspace || ldx < Cin || ldg < Cout) return DR_EINVAL;
    if ((((uintptr_t)x) | ((uintptr_t)grad_out) | ((uintptr_t)grad_w) | ((uintptr_t)grad_bias)) & 3u) return DR_EINVAL;
    if (((uintptr_t)workspace) & 15u) return DR_EINVAL;
    const int rc = conv_check_geom(Hi, Wi, Cin, Cout, k, stride, padding, dilation, g);
    if (rc != DR_OK) return rc;
    if (ldx > (1 << 20) || ldg > (1 << 20)) return DR_ENOSUP;
    const ConvSlabs sl = conv_wgrad_slabs(g.Ho * g.Wo);
    if (workspace_bytes < (size_t)conv_wg_workspace_bytes(g, sl)) return DR_EINVAL;
    if (!grad_w && !grad_bias) return DR_OK;
    WgradArgs A{g, sl, x, grad_out, (float*)workspace, (double*)((char*)workspace + conv_wg_bias_part_byte(g, sl)), grad_w, grad_bias, ldx, ldg};
    const hipStream_t st = (hipStream_t)stream;
    if (grad_w) {
        if (Cin % 4 == 0) {
            const bool vec = ((((uintptr_t)x) | ((uintptr_t)grad_out)) & 15u) == 0 && ldx % 4 == 0 && ldg % 4 == 0 && Cout % 4 == 0;
            const unsigned grid = (unsigned)(sl.S * ((Cout + WG_BT - 1) / WG_BT) * ((g.K + WG_BT - 1) / WG_BT));
            ProfScope ps(PK_GEMM, 2.0 * g.Ho * g.Wo * Cout * g.K, st);
            if (vec) hipLaunchKernelGGL(conv2d_wgrad_mfma_kernel<true>, dim3(grid), dim3(CV_NT), 0, st, A);
            else hipLaunchKernelGGL(conv2d_wgrad_mfma_kernel<false>, dim3(grid), dim3(CV_NT), 0, st, A);
        } else {
            const dim3 grid((unsigned)(((long long)Cout * g.K + 255) / 256), (unsigned)sl.S);
            hipLaunchKernelGGL(conv2d_wgrad_direct_kernel, grid, dim3(256), 0, st, A);
        }
        DR_LAUNCH_CHECK();
    }
    if (grad_bias) {
        hipLaunchKernelGGL(conv2d_bias_partial_kernel, dim3((unsigned)((Cout + 63) / 64), (unsigned)sl.S), dim3(256), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    const long long n = (long long)Cout * g.K + Cout;
    hipLaunchKernelGGL(conv2d_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_resize_rows_backward_f32(int C, int Hs, int Ws, int Hd, int Wd, const float* grad_out, int ldg, float* grad_in, int ldgi, void* stream) {
    if (C < 1 || Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1) return DR_EINVAL;
    if (!grad_out || !grad_in || ldg < C || ldgi < C) return DR_EINVAL;
    if ((((uintptr_t)grad_out) | ((uintptr_t)grad_in)) & 3u) return DR_EINVAL;
    if ((long long)Hs * Ws > (1ll << 24) || (long long)Hd * Wd > (1ll << 24) || C > (1 << 20) || ldg > (1 << 20) || ldgi > (1 << 20)) return DR_ENOSUP;
    const size_t n = (size_t)Hs * Ws * C;
    if ((n + 255) / 256 > 0x7fffffffull) return DR_ENOSUP;
    resize_rows_backward_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(C, Hs, Ws, Hd, Wd, grad_out, ldg, grad_in, ldgi);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
