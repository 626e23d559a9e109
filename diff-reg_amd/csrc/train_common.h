// train_common.h -- host helpers shared by the training entry points (train_layer.hip, train_fusion.hip, circle_loss.hip): a batched
// transposition (the GEMM contracts along contiguous k: x W for a gradient w.r.t. the input and g^T x for a weight gradient need the transposed
// operand), a two-operand add and a builder of GEMM launches (the carving of caller memory into 256-byte aligned arrays: Carver of carve.h).
#pragma once
#include <string.h>
#include "loop_common.h"

namespace dr {
namespace {

// out[c][r] = src[r][c] for up to 12 matrices in one launch; a destination row has stride ld_dst; its first w_dst >= rows entries are written,
// zero behind `rows` (the GEMM wants its k extent -- here the token count -- a multiple of 4)
struct TrProblem { const float* src; float* dst; int rows, cols, ld_src, ld_dst, w_dst, tile0, tiles_c; };
struct TrBatch { TrProblem p[12]; int n; };
__global__ __launch_bounds__(256) void transpose_batch_kernel(TrBatch G) {
    __shared__ float tile[32][33];
    int pi = 0;
    while (pi + 1 < G.n && (int)blockIdx.x >= G.p[pi + 1].tile0) ++pi;
    const TrProblem& P = G.p[pi];
    const int tl = blockIdx.x - P.tile0, tr = tl / P.tiles_c, tc = tl % P.tiles_c;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;              // 32 x 8
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = tr * 32 + ty + 8 * k, c = tc * 32 + tx;
        tile[ty + 8 * k][tx] = (r < P.rows && c < P.cols) ? P.src[(size_t)r * P.ld_src + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = tc * 32 + ty + 8 * k, r = tr * 32 + tx;
        if (c < P.cols && r < P.w_dst) P.dst[(size_t)c * P.ld_dst + r] = tile[tx][ty + 8 * k];
    }
}
struct Transposer {
    TrBatch g;
    int tiles;
    bool overflow;                                                        // an add() beyond the batch's 12 slots: launch() then fails instead of overrunning the struct
    static constexpr int CAP = (int)(sizeof(TrBatch::p) / sizeof(TrProblem));
    Transposer() { memset(&g, 0, sizeof(g)); tiles = 0; overflow = false; }
    void add(const float* src, int rows, int cols, int ld_src, float* dst, int ld_dst, int w_dst = -1) {
        if (g.n >= CAP) { overflow = true; return; }
        TrProblem& p = g.p[g.n++];
        p.src = src; p.dst = dst; p.rows = rows; p.cols = cols; p.ld_src = ld_src; p.ld_dst = ld_dst; p.w_dst = w_dst < 0 ? ld_dst : w_dst;
        p.tile0 = tiles; p.tiles_c = (cols + 31) / 32;
        tiles += ((p.w_dst + 31) / 32) * p.tiles_c;                       // (the pad entries of a destination row are covered too)
    }
    int launch(hipStream_t st) {
        if (overflow) return DR_EINVAL;
        if (g.n == 0) return DR_OK;
        hipLaunchKernelGGL(transpose_batch_kernel, dim3(tiles), dim3(256), 0, st, g);
        DR_LAUNCH_CHECK();
        memset(&g, 0, sizeof(g)); tiles = 0;
        return DR_OK;
    }
};

__global__ __launch_bounds__(256) void add2_kernel(long long n4, const float4* __restrict__ a, const float4* __restrict__ b, float4* __restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    const float4 x = a[e], y = b[e];
    out[e] = make_float4(x.x + y.x, x.y + y.y, x.z + y.z, x.w + y.w);
}

inline int up4(int x) { return (x + 3) & ~3; }

// up to 4 GEMMs in one launch (launch_gemm): add() fills the next GemmProblem (everything zero but the operands named here and scale = 1) and
// returns it -- the caller sets `bias` or the rotary tables on the reference
struct Gemms {
    GemmBatch g;
    bool overflow;                                                        // an add() beyond the batch's 4 slots: launch() then fails (add() filled a spare problem)
    GemmProblem spare;
    static constexpr int CAP = (int)(sizeof(GemmBatch::p) / sizeof(GemmProblem));
    Gemms() { memset(&g, 0, sizeof(g)); overflow = false; }
    // out[rows, ncols] = epi([A | A2] W^T) + addend: A holds the first K1 of the K contraction entries of a row, A2 the others
    GemmProblem& add(const float* A, int lda, const float* A2, int lda2, int K1, const float* W, float* out, int ldo, int rows, int ncols, int K,
                     int epi = EPI_NONE, const float* addend = nullptr) {
        if (g.n >= CAP) overflow = true;
        GemmProblem& p = overflow ? spare : g.p[g.n++];
        memset(&p, 0, sizeof(p));
        p.A = A; p.lda = lda; p.A2 = A2; p.lda2 = lda2; p.K1 = K1; p.W = W; p.out = out; p.ldo = ldo; p.rows = rows; p.ncols = ncols; p.K = K;
        p.epi = epi; p.scale = 1.f; p.addend = addend;
        return p;
    }
    GemmProblem& add(const float* A, int lda, const float* W, float* out, int ldo, int rows, int ncols, int K, int epi = EPI_NONE,
                     const float* addend = nullptr) {
        return add(A, lda, nullptr, 0, K, W, out, ldo, rows, ncols, K, epi, addend);
    }
    int launch(hipStream_t st) {
        if (overflow) return DR_EINVAL;
        const int rc = launch_gemm(g, st);
        memset(&g, 0, sizeof(g));
        return rc;
    }
};

}  // namespace
}  // namespace dr
