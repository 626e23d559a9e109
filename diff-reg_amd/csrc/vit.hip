// vit.hip -- the frozen DINOv2 ViT encoder of the 2D-3D model in the reference's own arithmetic: fp16 operands, ONE fp16 MFMA product per MAC,
// fp32 accumulation (Diff-Reg-2d3d/transformer/dinov2.py:166-237, layers/block.py:82-107, layers/attention.py:49-62, layers/patch_embed.py:69-82;
// CNNandDinov2(amp=True) casts the module and its input to torch.float16).  DESIGN 5p.  The residual stream stays fp32; fp16 roundings happen at
// the GEMM operands (LayerNorm output, qkv, attention output, the GELU hidden), at P inside the attention and at the final x_norm.
//   dr_gemm_rows_f16       out = A W^T (+ bias) with four epilogues; both operands staged by LDS-DMA, v_mfma_f32_16x16x32_f16
//   dr_layernorm_rows_f16  two-pass fp32 LayerNorm of stream rows -> fp16 (or fp32) rows
//   dr_attention_rows_f16  flash attention over packed qkv rows, d = 64, v_mfma_f32_32x32x16_f16, V by ds_read_b64_tr_b16
//   dr_patch_rows_f16      the patch gather in front of the patch-embedding GEMM
//   dr_vit_forward_f16     the whole encoder on one stream: no host read-back, no allocation, no atomics (two runs are bit-equal)
// The encoder's schedule, its validation order and the workspace carve are vit_forward.h's, shared with vit_f32.hip; so are the patch-gather and
// class-row kernels and the LayerNorm launch below (kernels.h).  Every global offset comes from vit_index.h (tools/vit_index_check.cpp walks it
// on the host).
#include "kernels.h"
#include "vit_forward.h"

namespace dr {

typedef _Float16 vh16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 vh16x4 __attribute__((ext_vector_type(4)));
typedef float vf32x4 __attribute__((ext_vector_type(4)));
typedef float vf32x16 __attribute__((ext_vector_type(16)));
typedef short vs16x4 __attribute__((ext_vector_type(4)));
typedef short vs16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void v_lds_void;
typedef __attribute__((address_space(3))) vs16x4 v_lds_s4;

// one LDS-DMA instruction of the wave: 16 bytes per lane from `src` (per lane) to LDS at dst (wave-uniform) + 16 lane
__device__ __forceinline__ void vit_glds16(unsigned dst, const void* src) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(dst), "v"(src) : "memory");
}

static int g_rows_tile = -1;       // dr_debug_gemm_rows_tile

// ---------------------------------------------------------------------------------------------------------------------
// The rows GEMM.  A workgroup of four waves (2 x 2) owns (32 MT) rows x (32 NT) columns; a wave MT x NT tiles of 16 x 16.  A k-step is two
// 32-deep chunks (K % 32 == 0 only: an odd last chunk is skipped, not padded).  Both operands arrive in 1 KB pieces (vit_index.h) by LDS-DMA
// into one of two buffers; the copy of step t + 1 is issued before the fragments of step t are read and waited for (vmcnt(0)) in front of the
// one barrier per step.  The product is W A^T: the accumulator then has the row on the lane and four consecutive columns in its registers,
// so an fp16 store is 8 bytes and an fp32 one 16 bytes per lane.
// ---------------------------------------------------------------------------------------------------------------------
struct GemmRowsArgs {
    const _Float16* a;
    const _Float16* w;
    const float* bias;
    const float* gamma;
    const float* addend;
    void* out;
    int M, K, N, lda, ldo, ld_addend, mode, colscale_cols;
    float colscale;
};

template <int MT, int NT>
__global__ __launch_bounds__(256) void gemm_rows_f16_kernel(GemmRowsArgs A) {
    constexpr int PA = 4 * MT, PB = 4 * NT, BUF = (PA + PB) * 1024;       // pieces of A and of W per k-step
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF];
    const unsigned lds_base = (unsigned)(size_t)(v_lds_void*)lds;
    const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), wr = w >> 1, wc = w & 1;
    const int bm = blockIdx.y * (32 * MT), bn = blockIdx.x * (32 * NT);
    const int KC = A.K / 32, NTL = A.N / 16, nsteps = (KC + 1) / 2;

    auto stage = [&](int step, int b) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < (PA + PB) / 4; ++i) {
            const int q = w + 4 * i;
            const unsigned dst = lds_base + b * BUF + q * 1024;
            if (q < PA) {
                const int c = q / (2 * MT), row0 = bm + (q % (2 * MT)) * 16, kc = 2 * step + c;
                if (row0 < A.M && kc < KC) vit_glds16(dst, A.a + vit_a_src(A.M, A.lda, row0, kc, lane));
            } else {
                const int q2 = q - PA, c = q2 / (2 * NT), nt = bn / 16 + q2 % (2 * NT), kc = 2 * step + c;
                if (nt < NTL && kc < KC) vit_glds16(dst, A.w + vit_w_piece(KC, nt, kc) + lane * 8);
            }
        }
    };

    vf32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = vf32x4{0.f, 0.f, 0.f, 0.f};

    const int foff = vit_piece_read(lane & 15, lane >> 4);
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
        const int b = step & 1;
        if (step + 1 < nsteps) stage(step + 1, b ^ 1);
        const char* buf = lds + b * BUF;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (2 * step + c < KC) {
                vh16x8 af[MT], bf[NT];
#pragma unroll
                for (int i = 0; i < MT; ++i) af[i] = *reinterpret_cast<const vh16x8*>(buf + (c * 2 * MT + wr * MT + i) * 1024 + foff);
#pragma unroll
                for (int j = 0; j < NT; ++j) bf[j] = *reinterpret_cast<const vh16x8*>(buf + (PA + c * 2 * NT + wc * NT + j) * 1024 + foff);
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[j], af[i], acc[i][j], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // own pieces of step + 1 have landed ...
        __syncthreads();                                           // ... and everybody's; everybody is done reading buffer b
    }

    // ---- epilogue: lane holds row (lane & 15), columns 4 (lane >> 4) .. + 3 of each tile
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int row = bm + (wr * MT + i) * 16 + (lane & 15);
        if (row >= A.M) continue;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = bn + (wc * NT + j) * 16 + (lane >> 4) * 4;
            if (col >= A.N) continue;
            vf32x4 v = acc[i][j];
            if (A.bias) {
                const vf32x4 bv = *reinterpret_cast<const vf32x4*>(A.bias + col);
                v += bv;
            }
            if (A.mode == DR_GEMM_ROWS_F16 || A.mode == DR_GEMM_ROWS_GELU_F16) {
                if (A.mode == DR_GEMM_ROWS_GELU_F16) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.f + erff(v[e] * 0.70710678118654752440f));
                } else if (col < A.colscale_cols) {
                    v *= A.colscale;
                }
                const vh16x4 hv = {(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
                *reinterpret_cast<vh16x4*>(reinterpret_cast<_Float16*>(A.out) + (size_t)row * A.ldo + col) = hv;
            } else {
                float* o = reinterpret_cast<float*>(A.out) + (size_t)row * A.ldo + col;
                if (A.mode == DR_GEMM_ROWS_SCALE_RESID_F32) {
                    if (A.gamma) v *= *reinterpret_cast<const vf32x4*>(A.gamma + col);
                    v += *reinterpret_cast<const vf32x4*>(o);
                } else if (A.addend) {
                    v += *reinterpret_cast<const vf32x4*>(A.addend + (size_t)row * A.ld_addend + col);
                }
                *reinterpret_cast<vf32x4*>(o) = v;
            }
        }
    }
}

static int gemm_rows_check(const GemmRowsArgs& g) {
    if (!g.a || !g.w || !g.out || g.M < 1 || g.K < 32 || g.N < 16 || g.K % 32 || g.N % 16) return DR_EINVAL;
    if (g.mode < DR_GEMM_ROWS_F16 || g.mode > DR_GEMM_ROWS_F32) return DR_EINVAL;
    if (g.lda < g.K || g.lda % 8 || g.ldo < g.N || g.ldo % 4) return DR_EINVAL;
    if (!aligned_to(g.a, 16) || !aligned_to(g.w, 16) || !aligned_to(g.out, 16) || !aligned_to(g.bias, 16) || !aligned_to(g.gamma, 16)) return DR_EINVAL;
    if (g.addend && (g.mode != DR_GEMM_ROWS_F32 || g.ld_addend < g.N || g.ld_addend % 4 || !aligned_to(g.addend, 16))) return DR_EINVAL;
    if (g.colscale_cols < 0 || g.colscale_cols > g.N || g.colscale_cols % 16) return DR_EINVAL;
    if ((long long)g.M * g.lda >= (1ll << 31) || (long long)g.M * g.ldo >= (1ll << 31) || (long long)g.N * g.K >= (1ll << 31)) return DR_ENOSUP;
    if (g_rows_tile < -1 || g_rows_tile > 2) return DR_EINVAL;
    return DR_OK;
}

// the tile: the largest of 128 x 128, 128 x 64, 64 x 64 that still gives every CU a workgroup, else the smallest
static int gemm_rows_tile(int M, int N) {
    if (g_rows_tile >= 0) return g_rows_tile;
    const long long cus = device_cu_count();
    auto blocks = [&](int bm, int bn) { return (long long)((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
    if (blocks(128, 128) >= cus) return 2;
    if (blocks(128, 64) >= cus) return 1;
    return 0;
}

static int gemm_rows_launch(const GemmRowsArgs& g, hipStream_t st) {
    const int tile = gemm_rows_tile(g.M, g.N);
    if (tile == 2) {
        hipLaunchKernelGGL((gemm_rows_f16_kernel<4, 4>), dim3((g.N + 127) / 128, (g.M + 127) / 128), dim3(256), 0, st, g);
    } else if (tile == 1) {
        hipLaunchKernelGGL((gemm_rows_f16_kernel<4, 2>), dim3((g.N + 63) / 64, (g.M + 127) / 128), dim3(256), 0, st, g);
    } else {
        hipLaunchKernelGGL((gemm_rows_f16_kernel<2, 2>), dim3((g.N + 63) / 64, (g.M + 63) / 64), dim3(256), 0, st, g);
    }
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// nn.Linear weight [N, K] fp16 (row stride ldw) -> the packed image of vit_index.h, k padded with zeros to Kp
__global__ void pack_weight_f16_kernel(int N, int K, int Kp, const _Float16* w, int ldw, _Float16* packed) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)N * Kp) return;
    const int n = (int)(idx / Kp), k = (int)(idx % Kp);
    packed[vit_w_packed_at(Kp / 32, n, k)] = k < K ? w[(size_t)n * ldw + k] : (_Float16)0.f;
}

// ---------------------------------------------------------------------------------------------------------------------
// LayerNorm over fp32 rows: one wave per row, statistics in fp32, two passes (mean, then the centred sum of squares: a constant row has
// variance exactly 0), a third pass writes.  The row is re-read from cache, not held in registers: any C.
// ---------------------------------------------------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(int rows, int C, const float* x, int ldx, const float* gamma, const float* beta,
                                                             float eps, void* out, int ldo) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * ldx;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xr[c];
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float dlt = xr[c] - mean;
        q += dlt * dlt;
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
    for (int c = lane; c < C; c += 64) {
        const float y = (xr[c] - mean) * rstd * (gamma ? gamma[c] : 1.f) + (beta ? beta[c] : 0.f);
        if (F32) reinterpret_cast<float*>(out)[(size_t)row * ldo + c] = y;
        else reinterpret_cast<_Float16*>(out)[(size_t)row * ldo + c] = (_Float16)y;
    }
}

int launch_layernorm_rows(int rows, int C, const float* x, int ldx, const float* gamma, const float* beta, float eps, int out_f32, void* out,
                          int ldo, hipStream_t st) {
    const dim3 grid((rows + 3) / 4), block(256);
    if (out_f32) hipLaunchKernelGGL(layernorm_rows_kernel<true>, grid, block, 0, st, rows, C, x, ldx, gamma, beta, eps, out, ldo);
    else hipLaunchKernelGGL(layernorm_rows_kernel<false>, grid, block, 0, st, rows, C, x, ldx, gamma, beta, eps, out, ldo);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Flash attention over packed qkv rows [L, 3 H 64] fp16 (the layout of qkv.reshape(N, 3, H, d); q already carries d^-0.5), no mask.  A
// workgroup: 128 queries of one head, four waves of 32 queries; key tiles of 32.
//   * a K tile and a V tile (32 keys x 128 B each) land in LDS by eight LDS-DMA instructions, two per wave, issued one tile ahead into the other
//     buffer; one barrier per tile.  Keys past L clamp to the last key (finite data) and are dropped by the softmax.
//   * S^T = K Q^T on v_mfma_f32_32x32x16_f16: K fragments by ds_read_b128 (image swizzled on the source side), Q fragments once per wave
//     from global.  A lane then holds 16 keys of ITS query: the softmax is in registers plus one v_permlane32_swap per reduction.
//   * online softmax in fp32 with exp2; the accumulators are rescaled only when some query's running maximum moved; P is rounded to fp16 once
//     (the row sum is of the unrounded P, as in every flash form of attention.hip).
//   * O^T = V^T P^T: the V fragments come out of ds_read_b64_tr_b16, two 4-key blocks per fragment in the order in which the score registers
//     hold the keys, so P goes from registers into the MFMA.
// ---------------------------------------------------------------------------------------------------------------------
template <typename Op>
__device__ __forceinline__ float vit_xhalf(float v, Op op) {
    typedef unsigned vu32x2 __attribute__((ext_vector_type(2)));
    const unsigned u = __float_as_uint(v);
    const vu32x2 r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return op(__uint_as_float(r.x), __uint_as_float(r.y));
}

__global__ __launch_bounds__(256) void attention_rows_f16_kernel(int L, int H, const _Float16* qkv, int ld, _Float16* out, int ldo) {
    constexpr int TILE = 4096, BUF = 2 * TILE;                    // K image, V image
    __shared__ __attribute__((aligned(16))) char lds[2 * BUF];
    const unsigned lds_base = (unsigned)(size_t)(v_lds_void*)lds;
    const int t = threadIdx.x, lane = t & 63, h = lane >> 5, l31 = lane & 31, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int head = blockIdx.y, qb = blockIdx.x * 128;
    const int my_q = qb + w * 32 + l31;
    const int qrow = min(my_q, L - 1);

    // Q fragments: feature 16 s + 8 h + j of this lane's query
    vh16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const vh16x8*>(qkv + (size_t)qrow * ld + head * 64 + 16 * s + 8 * h);

    // instruction ins of a tile: ins < 4 -> K, else V; wave w issues w and w + 4
    auto stage = [&](int kt, int b) __attribute__((always_inline)) {
        vit_glds16(lds_base + b * BUF + w * 1024, qkv + vit_kv_src(L, ld, H, head, 1, kt, w, lane));
        vit_glds16(lds_base + b * BUF + TILE + w * 1024, qkv + vit_kv_src(L, ld, H, head, 2, kt, w, lane));
    };
    const int koff = l31 * 128;                                   // K fragment: key l31
    // V fragments: lane g16 of a 16-lane group supplies key row (g16 >> 2) of a 4-key block, features 4 (g16 & 3) .. + 3 of the group's 16
    const int g16 = l31 & 15, vq = g16 >> 2, vp = g16 & 3, grp = l31 >> 4;
    unsigned voff[2][2][2];                                       // [k-step][block][feature tile]
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int krow = 16 * s + 8 * blk + 4 * h + vq, ch = 4 * i + 2 * grp + (vp >> 1);
                voff[s][blk][i] = TILE + krow * 128 + ((ch ^ vit_v_swz(krow)) << 4) + (vp & 1) * 8;
            }

    vf32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    const int nkt = (L + 31) / 32;
    // the Q loads are consumed here, so the compiler's own wait for them stands in front of the loop and not behind a tile's DMA
#pragma unroll
    for (int s = 0; s < 4; ++s) asm volatile("" ::"v"(qf[s]));

    stage(0, 0);
    for (int kt = 0; kt < nkt; ++kt) {
        const int b = kt & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // own DMA of tile kt has landed ...
        __syncthreads();                                           // ... and everybody's; everybody is done with tile kt - 1's buffer
        if (kt + 1 < nkt) stage(kt + 1, b ^ 1);
        const char* kb = lds + b * BUF + koff;
        // ---- S^T = K Q^T
        vf32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const vh16x8 kf = *reinterpret_cast<const vh16x8*>(kb + (((2 * s + h) ^ vit_k_swz(l31)) << 4));
            sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], sc, 0, 0, 0);
        }
        // ---- running softmax (register r holds key (r & 3) + 8 (r >> 2) + 4 h of the tile)
        constexpr float LOG2E = 1.4426950408889634f;
        float mx = -INFINITY;
        if (kt * 32 + 32 > L) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h >= L) sc[r] = -INFINITY;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[r]);
        mx = vit_xhalf(mx, [](float x, float y) { return fmaxf(x, y); }) * LOG2E;      // every tile has a live key: finite
        const float m_new = fmaxf(m_run, mx);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sc[r], LOG2E, -m_new));
            sc[r] = p;
            psum += p;
        }
        psum = vit_xhalf(psum, [](float x, float y) { return x + y; });
        l_run = l_run * alpha + psum;
        if (__any(m_new != m_run)) {                              // (alpha == 1 exactly in every lane otherwise)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][r] *= alpha;
        }
        m_run = m_new;
        // ---- O^T += V^T P^T: k-step s contracts the keys of score registers 8 s .. 8 s + 7
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            vh16x8 pf;
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[j] = (_Float16)sc[8 * s + j];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const unsigned base = lds_base + b * BUF;
                const vs16x4 va = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v_lds_s4*)(size_t)(base + voff[s][0][i]));
                const vs16x4 vb = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v_lds_s4*)(size_t)(base + voff[s][1][i]));
                const vs16x8 v8 = {va[0], va[1], va[2], va[3], vb[0], vb[1], vb[2], vb[3]};
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(vh16x8, v8), pf, acc[i], 0, 0, 0);
            }
        }
    }
    // ---- out[q][32 i + 8 g + 4 h + e] = O^T / l : four consecutive features per store
    if (my_q < L) {
        const float inv = 1.f / l_run;
        _Float16* o = out + (size_t)my_q * ldo + head * 64;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const vh16x4 hv = {(_Float16)(acc[i][4 * g] * inv), (_Float16)(acc[i][4 * g + 1] * inv), (_Float16)(acc[i][4 * g + 2] * inv),
                                   (_Float16)(acc[i][4 * g + 3] * inv)};
                *reinterpret_cast<vh16x4*>(o + 32 * i + 8 * g + 4 * h) = hv;
            }
    }
}

static int attention_rows_check(int L, int H, int d, const void* qkv, int ld, const void* out, int ldo) {
    if (d != 64 || L < 1 || H < 1 || !qkv || !out) return DR_EINVAL;
    if (ld < 3 * H * 64 || ld % 8 || ldo < H * 64 || ldo % 4 || !aligned_to(qkv, 16) || !aligned_to(out, 8)) return DR_EINVAL;
    if ((long long)L * ld >= (1ll << 31) || H > 65535) return DR_ENOSUP;
    return DR_OK;
}

static int attention_rows_launch(int L, int H, const _Float16* qkv, int ld, _Float16* out, int ldo, hipStream_t st) {
    hipLaunchKernelGGL(attention_rows_f16_kernel, dim3((L + 127) / 128, H), dim3(256), 0, st, L, H, qkv, ld, out, ldo);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// patch gather; the class-token row of the stream (both precisions)
// ---------------------------------------------------------------------------------------------------------------------
template <typename Tin, typename Tout>
__global__ void patch_rows_kernel(int H, int W, int p, int Np, int Kp, const Tin* img, Tout* out, int ldo) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)Np * Kp) return;
    const int patch = (int)(idx / Kp), k = (int)(idx % Kp);
    const long long src = vit_patch_src(H, W, p, patch, k);
    out[(size_t)patch * ldo + k] = src < 0 ? (Tout)0.f : (Tout)img[src];
}

// float32 rows additionally want 4-byte aligned pointers and Np ldo < 2^31 (dr_patch_rows_f32's domain)
int patch_rows_check(int H, int W, int p, const void* img, const void* out, int ldo, int out_f32) {
    if (!img || !out || p < 1 || H < p || W < p || H % p || W % p) return DR_EINVAL;
    if (p > 64 || (long long)H * W >= (1ll << 26)) return DR_ENOSUP;
    if (ldo < vit_patch_kp(p)) return DR_EINVAL;
    if (out_f32 && (!aligned_to(img, 4) || !aligned_to(out, 4))) return DR_EINVAL;
    if (out_f32 && (long long)(H / p) * (W / p) * ldo >= (1ll << 31)) return DR_ENOSUP;
    return DR_OK;
}

int launch_patch_rows(int H, int W, int p, const void* img, int img_f32, void* out, int out_f32, int ldo, hipStream_t st) {
    const int Np = (H / p) * (W / p), Kp = vit_patch_kp(p);
    const size_t n = (size_t)Np * Kp;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (out_f32) hipLaunchKernelGGL((patch_rows_kernel<float, float>), grid, block, 0, st, H, W, p, Np, Kp, (const float*)img, (float*)out, ldo);
    else if (img_f32) hipLaunchKernelGGL((patch_rows_kernel<float, _Float16>), grid, block, 0, st, H, W, p, Np, Kp, (const float*)img, (_Float16*)out, ldo);
    else hipLaunchKernelGGL((patch_rows_kernel<_Float16, _Float16>), grid, block, 0, st, H, W, p, Np, Kp, (const _Float16*)img, (_Float16*)out, ldo);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

__global__ void cls_row_kernel(int D, const float* cls, const float* pos, float* stream) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < D) stream[c] = cls[c] + pos[c];
}

int launch_cls_row(int D, const float* cls, const float* pos, float* stream_row, hipStream_t st) {
    hipLaunchKernelGGL(cls_row_kernel, dim3((D + 255) / 256), dim3(256), 0, st, D, cls, pos, stream_row);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// vit_forward.h's policy for fp16 operands: every pointer a kernel reads by 16-byte vectors (pos as the patch GEMM's addend, the biases and
// LayerScale vectors in the GEMM epilogues, the packed weights) sits on 16 bytes; a take is a raw copy of the stream (the caller norms it)
// ---------------------------------------------------------------------------------------------------------------------
struct VitF16 : VitDeviceSteps {
    typedef dr_vit_config_f16 config;
    typedef dr_vit_block_f16 block;
    enum { ELEM = 2, COLSCALE = DR_GEMM_ROWS_F16, GELU = DR_GEMM_ROWS_GELU_F16, SCALE_RESID = DR_GEMM_ROWS_SCALE_RESID_F32, ADDEND = DR_GEMM_ROWS_F32 };
    static int img_f32(const config& c) { return c.img_f32; }
    static int norm_take(const config&) { return 0; }
    static bool aligned(const config& c) {
        return aligned_to(c.workspace, 256) && aligned_to(c.x_prenorm, 16) && aligned_to(c.pos, 16) && aligned_to(c.patch_b, 16);
    }
    static bool aligned(const block& b) {
        const void* al[] = {b.qkv_w, b.proj_w, b.fc1_w, b.fc2_w, b.qkv_b, b.proj_b, b.fc1_b, b.fc2_b, b.ls1, b.ls2};
        for (const void* q : al)
            if (!aligned_to(q, 16)) return false;
        return true;
    }
    static bool take_aligned(const void*) { return true; }
    static int patch_rows(int H, int W, int p, const void* img, int f32, void* out, int ldo, void* st) {
        return launch_patch_rows(H, W, p, img, f32, out, 0, ldo, (hipStream_t)st);
    }
    static int gemm(const void* a, int lda, int M, int K, int N, const void* w, const float* bias, int mode, void* out, int ldo, float cs, int cs_cols,
                    const float* gamma, const float* addend, int ld_addend, void* st) {
        GemmRowsArgs g;
        g.a = (const _Float16*)a; g.w = (const _Float16*)w; g.bias = bias; g.gamma = gamma; g.addend = addend; g.out = out;
        g.M = M; g.K = K; g.N = N; g.lda = lda; g.ldo = ldo; g.ld_addend = ld_addend; g.mode = mode; g.colscale_cols = cs_cols; g.colscale = cs;
        const int rc = gemm_rows_check(g);
        return rc != DR_OK ? rc : gemm_rows_launch(g, (hipStream_t)st);
    }
    static int layernorm(int L, int D, const float* x, const float* g, const float* b, float eps, void* out, void* st) {
        return launch_layernorm_rows(L, D, x, D, g, b, eps, 0, out, D, (hipStream_t)st);
    }
    static int attention(int L, int heads, int D, const void* qkv, void* ao, void* st) {
        return attention_rows_launch(L, heads, (const _Float16*)qkv, 3 * D, (_Float16*)ao, D, (hipStream_t)st);
    }
};

}  // namespace dr

using namespace dr;

extern "C" {

void dr_debug_gemm_rows_tile(int c) { g_rows_tile = c; }

size_t dr_pack_weight_f16_bytes(int N, int K) {
    if (N < 16 || N % 16 || K < 1) return 0;
    return vit_w_packed_elems(N, vit_round_up(K, 32)) * 2;
}

int dr_pack_weight_f16(int N, int K, const void* w, int ldw, void* packed, void* stream) {
    if (!w || !packed || N < 16 || N % 16 || K < 1 || ldw < K || !aligned_to(packed, 16) || !aligned_to(w, 2)) return DR_EINVAL;
    const int Kp = vit_round_up(K, 32);
    if ((long long)N * Kp >= (1ll << 31) || (long long)N * ldw >= (1ll << 31)) return DR_ENOSUP;
    const size_t n = (size_t)N * Kp;
    hipLaunchKernelGGL(pack_weight_f16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, K, Kp, (const _Float16*)w, ldw,
                       (_Float16*)packed);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

static GemmRowsArgs gemm_rows_args(const dr_gemm_rows_f16_args* a) {
    GemmRowsArgs g;
    g.a = (const _Float16*)a->a; g.w = (const _Float16*)a->w_packed; g.bias = a->bias; g.gamma = a->gamma; g.addend = a->addend; g.out = a->out;
    g.M = a->M; g.K = a->K; g.N = a->N; g.lda = a->lda; g.ldo = a->ldo; g.ld_addend = a->ld_addend; g.mode = a->mode;
    g.colscale_cols = a->mode == DR_GEMM_ROWS_F16 ? a->colscale_cols : 0; g.colscale = a->colscale;
    if (a->mode != DR_GEMM_ROWS_SCALE_RESID_F32) g.gamma = nullptr;
    return g;
}

int dr_gemm_rows_f16(const dr_gemm_rows_f16_args* args, void* stream) {
    if (!args) return DR_EINVAL;
    const GemmRowsArgs g = gemm_rows_args(args);
    const int rc = gemm_rows_check(g);
    return rc != DR_OK ? rc : gemm_rows_launch(g, (hipStream_t)stream);
}

int dr_layernorm_rows_f16(int rows, int C, const float* x, int ldx, const float* gamma, const float* beta, float eps, int out_f32, void* out, int ldo,
                          void* stream) {
    if (rows < 1 || C < 1 || !x || !out || ldx < C || ldo < C || !(eps >= 0.f) || (out_f32 != 0 && out_f32 != 1)) return DR_EINVAL;
    if ((long long)rows * ldx >= (1ll << 31) || (long long)rows * ldo >= (1ll << 31)) return DR_ENOSUP;
    return launch_layernorm_rows(rows, C, x, ldx, gamma, beta, eps, out_f32, out, ldo, (hipStream_t)stream);
}

int dr_attention_rows_f16(int L, int H, int d, const void* qkv, int ldqkv, void* out, int ldo, void* stream) {
    const int rc = attention_rows_check(L, H, d, qkv, ldqkv, out, ldo);
    return rc != DR_OK ? rc : attention_rows_launch(L, H, (const _Float16*)qkv, ldqkv, (_Float16*)out, ldo, (hipStream_t)stream);
}

int dr_patch_rows_f16(int H, int W, int p, const void* img, int img_f32, void* out, int ldo, void* stream) {
    const int rc = patch_rows_check(H, W, p, img, out, ldo, 0);
    if (rc != DR_OK) return rc;
    if (img_f32 != 0 && img_f32 != 1) return DR_EINVAL;
    return launch_patch_rows(H, W, p, img, img_f32, out, 0, ldo, (hipStream_t)stream);
}

size_t dr_vit_workspace_bytes(int H, int W, int p, int D, int Dh) { return vit_workspace_bytes(H, W, p, D, Dh, VitF16::ELEM); }

int dr_vit_forward_f16(const dr_vit_config_f16* c, void* stream) { return c ? vit_forward<VitF16>(*c, stream) : DR_EINVAL; }

}  // extern "C"
