// front2d3d.hip -- the geometry head and the feature-layout glue of MATR2D3D.forward on the device (ABI 0.7.0, second set):
//   back_project (mode 0)        vision3d/ops/back_project.py:7-55                   EXP/model.py:306
//   back_project_depth (mode 1)  MATR2D3D.back_project_depth, EXP/model.py:852-901   EXP/model.py:349
//   create_meshgrid (pixels)     vision3d/ops/meshgrid.py:4-37 (not normalised)      EXP/model.py:310
//   render                       vision3d/ops/render.py:9-57, ops/se3.py:46-53       EXP/model.py:335
//   resize_tokens                F.interpolate(bilinear, align_corners=True) + view + transpose        EXP/model.py:374-375
//   rows_normalize_chw           view(C, -1).transpose(0, 1).contiguous() + F.normalize(p=2, dim=1)    EXP/model.py:536-538
// EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.  One image per call, enqueued on the stream, nothing read back.
// The two geometry kernels keep the reference's float32 operation order (no contraction into FMA, IEEE division); the two layout kernels
// do their arithmetic in double on the float32 inputs and round once.  No float atomics anywhere: the resample backward is a gather (each
// source texel sums its destinations in ascending order), the sparse normalise backward lets the first occurrence of a row sum its repeats in
// list order -- two runs are bit-identical.
#include "kernels.h"
#include "resize_index.h"

// the geometry kernels restate float32 expressions of the reference term by term: no a * b + c becomes an FMA in this file
#pragma clang fp contract(off)

namespace dr {

constexpr unsigned FRONT_STATUS_BAD_INDEX = 2u;   // bit 1 of the word of dr_device_status (as eval2d3d.hip): a row index outside [0, P)
constexpr int FR_BLOCK = 256;
constexpr int FR_MAX_C = 256;                     // channels one normalise tile holds

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// ------------------------------------------------------------------------------------------------------------
// back projection: one pass over the depth image, four pixels per thread
// ------------------------------------------------------------------------------------------------------------
struct BackProjectArgs {
    const float* depth;      // [H*W]
    const float* K;          // [9]
    const float *a_dev, *b_dev;
    float a, b, limit;
    int mode, has_limit, W;
    long long n;             // H*W
    float* points;           // [n,3]
    unsigned char* mask;     // [n]
    float* pixels;           // [n,2] or NULL
};

__device__ __forceinline__ void back_project_one(const BackProjectArgs& A, float d, long long i, float a, float b, float fx, float fy, float cx,
                                                 float cy, float* xyz, unsigned char* m, float* hw) {
    const int v = (int)(i / A.W), u = (int)(i - (long long)v * A.W);
    float z = A.mode == 0 ? d / a : d * a + b;
    if (A.has_limit && z > A.limit) z = 0.0f;
    xyz[0] = ((float)u - cx) * z / fx;
    xyz[1] = ((float)v - cy) * z / fy;
    xyz[2] = z;
    *m = z > 0.0f ? 1 : 0;
    hw[0] = (float)v;
    hw[1] = (float)u;
}

template <bool VEC>
__global__ void __launch_bounds__(FR_BLOCK) back_project_kernel(BackProjectArgs A) {
    const float fx = A.K[0], cx = A.K[2], fy = A.K[4], cy = A.K[5];
    const float a = (A.mode == 1 && A.a_dev) ? A.a_dev[0] : A.a;
    const float b = (A.mode == 1 && A.b_dev) ? A.b_dev[0] : A.b;
    const long long groups = (A.n + 3) / 4;
    for (long long g = (long long)blockIdx.x * FR_BLOCK + threadIdx.x; g < groups; g += (long long)gridDim.x * FR_BLOCK) {
        const long long i0 = g * 4;
        float xyz[12], hw[8];
        unsigned char m[4];
        if (VEC && i0 + 4 <= A.n) {
            const float4 d4 = *(const float4*)(A.depth + i0);
            const float d[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) back_project_one(A, d[j], i0 + j, a, b, fx, fy, cx, cy, xyz + 3 * j, m + j, hw + 2 * j);
            float4* po = (float4*)(A.points + i0 * 3);           // 48 bytes per thread, consecutive threads consecutive: coalesced
            po[0] = make_float4(xyz[0], xyz[1], xyz[2], xyz[3]);
            po[1] = make_float4(xyz[4], xyz[5], xyz[6], xyz[7]);
            po[2] = make_float4(xyz[8], xyz[9], xyz[10], xyz[11]);
            *(unsigned*)(A.mask + i0) = (unsigned)m[0] | ((unsigned)m[1] << 8) | ((unsigned)m[2] << 16) | ((unsigned)m[3] << 24);
            if (A.pixels) {
                float4* px = (float4*)(A.pixels + i0 * 2);
                px[0] = make_float4(hw[0], hw[1], hw[2], hw[3]);
                px[1] = make_float4(hw[4], hw[5], hw[6], hw[7]);
            }
        } else {
            for (int j = 0; j < 4 && i0 + j < A.n; ++j) {
                const long long i = i0 + j;
                back_project_one(A, A.depth[i], i, a, b, fx, fy, cx, cy, xyz, m, hw);
                A.points[i * 3] = xyz[0]; A.points[i * 3 + 1] = xyz[1]; A.points[i * 3 + 2] = xyz[2];
                A.mask[i] = m[0];
                if (A.pixels) { A.pixels[i * 2] = hw[0]; A.pixels[i * 2 + 1] = hw[1]; }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// render: one thread per point
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FR_BLOCK) render_kernel(int N, const float* __restrict__ pts, const float* __restrict__ K,
                                                          const float* __restrict__ T, float eps, float* __restrict__ pixels,
                                                          float* __restrict__ depth) {
    const int i = blockIdx.x * FR_BLOCK + threadIdx.x;
    if (i >= N) return;
    float x = pts[(size_t)i * 3], y = pts[(size_t)i * 3 + 1], z = pts[(size_t)i * 3 + 2];
    if (T) {                                                     // apply_transform: p R^T + t
        const float qx = x * T[0] + y * T[1] + z * T[2] + T[3];
        const float qy = x * T[4] + y * T[5] + z * T[6] + T[7];
        const float qz = x * T[8] + y * T[9] + z * T[10] + T[11];
        x = qx; y = qy; z = qz;
    }
    const float zc = z < eps ? eps : z;                          // clamp(min=eps): a NaN stays a NaN
    pixels[(size_t)i * 2] = K[4] * y / zc + K[5];                // (h, w)
    pixels[(size_t)i * 2 + 1] = K[0] * x / zc + K[2];
    if (depth) depth[i] = z;
}

// ------------------------------------------------------------------------------------------------------------
// bilinear resample (align_corners=True) written as token rows, and its gather backward
// ------------------------------------------------------------------------------------------------------------
constexpr int RS_TC = 32, RS_TP = 64;             // tile: 32 channels x 64 pixels, [c][p] in LDS with one word of padding per row

// resize_scale / resize_src / resize_blend: resize_index.h (shared with dr_resize_rows_f32)

__global__ void __launch_bounds__(FR_BLOCK) resize_tokens_kernel(int C, int Hs, int Ws, int Hd, int Wd, const float* __restrict__ in,
                                                                 float* __restrict__ out) {
    __shared__ float tile[RS_TC * (RS_TP + 1)];
    const int Pd = Hd * Wd, p0 = blockIdx.x * RS_TP, c0 = blockIdx.y * RS_TC;
    const double sh = resize_scale(Hs, Hd), sw = resize_scale(Ws, Wd);
    {   // lanes along the destination pixel: neighbouring lanes read neighbouring texels
        const int pl = threadIdx.x % RS_TP, p = p0 + pl;
        if (p < Pd) {
            const int yd = p / Wd, xd = p - yd * Wd;
            int y0, y1, x0, x1;
            double ly, lx;
            resize_src(sh, yd, Hs, y0, y1, ly);
            resize_src(sw, xd, Ws, x0, x1, lx);
            for (int cl = threadIdx.x / RS_TP; cl < RS_TC && c0 + cl < C; cl += FR_BLOCK / RS_TP) {
                const float* src = in + (size_t)(c0 + cl) * Hs * Ws;
                const double v00 = src[y0 * Ws + x0], v01 = src[y0 * Ws + x1], v10 = src[y1 * Ws + x0], v11 = src[y1 * Ws + x1];
                tile[cl * (RS_TP + 1) + pl] = resize_blend(ly, lx, v00, v01, v10, v11);
            }
        }
    }
    __syncthreads();
    {   // lanes along the channel: 128-byte runs of one token row
        const int cl = threadIdx.x % RS_TC;
        if (c0 + cl < C)
            for (int pl = threadIdx.x / RS_TC; pl < RS_TP && p0 + pl < Pd; pl += FR_BLOCK / RS_TC)
                out[(size_t)(p0 + pl) * C + c0 + cl] = tile[cl * (RS_TP + 1) + pl];
    }
}

// resize_candidates / resize_gather: resize_index.h (shared with dr_resize_rows_backward_f32)
__global__ void __launch_bounds__(FR_BLOCK) resize_tokens_backward_kernel(int C, int Hs, int Ws, int Hd, int Wd, const float* __restrict__ g,
                                                                          float* __restrict__ grad_in) {
    __shared__ float tile[RS_TC * (RS_TP + 1)];
    const int Ps = Hs * Ws, s0 = blockIdx.x * RS_TP, c0 = blockIdx.y * RS_TC;
    const double sh = resize_scale(Hs, Hd), sw = resize_scale(Ws, Wd);
    {   // lanes along the channel (the token rows of g are read in 128-byte runs); each (texel, channel) sums its destinations in order
        const int cl = threadIdx.x % RS_TC;
        if (c0 + cl < C)
            for (int sl = threadIdx.x / RS_TC; sl < RS_TP && s0 + sl < Ps; sl += FR_BLOCK / RS_TC) {
                const int ys = (s0 + sl) / Ws, xs = (s0 + sl) - ys * Ws;
                const double acc = resize_gather(sh, sw, ys, xs, Hs, Ws, Hd, Wd, [&](int pd) { return g[(size_t)pd * C + c0 + cl]; });
                tile[cl * (RS_TP + 1) + sl] = (float)acc;
            }
    }
    __syncthreads();
    {   // lanes along the source texel
        const int sl = threadIdx.x % RS_TP;
        if (s0 + sl < Ps)
            for (int cl = threadIdx.x / RS_TP; cl < RS_TC && c0 + cl < C; cl += FR_BLOCK / RS_TP)
                grad_in[(size_t)(c0 + cl) * Ps + s0 + sl] = tile[cl * (RS_TP + 1) + sl];
    }
}

// ------------------------------------------------------------------------------------------------------------
// [C, P] -> [P, C] rows divided by max(|row|, eps): an LDS-tiled transpose, every element read once and written once
// ------------------------------------------------------------------------------------------------------------
// tile [C][TP + 1] floats: TP = 64 pixels for C <= 128, TP = 32 for C <= 256 -- at most 8 448 floats (33 KiB), four workgroups per CU.  The row
// stride TP + 1 is odd: the load phase writes consecutive words (lanes along p), the store phase reads words TP + 1 apart (lanes along c), and an
// odd stride visits the 32 banks of ds_read_b32 / ds_write_b32 once per 32-lane half -- neither phase conflicts.
constexpr int NM_TILE_WORDS = FR_MAX_C * 33;
constexpr float NM_EPS = 1e-12f;                  // F.normalize's eps

template <int TP>
__global__ void __launch_bounds__(FR_BLOCK) rows_normalize_kernel(int C, long long P, const float* __restrict__ in, float* __restrict__ out) {
    constexpr int PARTS = FR_BLOCK / TP;
    __shared__ float tile[NM_TILE_WORDS];
    __shared__ double part[PARTS][TP];
    __shared__ float nrm[TP];
    const long long p0 = (long long)blockIdx.x * TP;
    const int np = (int)(P - p0 < TP ? P - p0 : TP);
    const int pl = threadIdx.x % TP, pt = threadIdx.x / TP;
    double s = 0.0;
    if (pl < np)
        for (int c = pt; c < C; c += PARTS) {                   // lanes along p: 4 * TP contiguous bytes of one channel row
            const float x = in[(size_t)c * P + p0 + pl];
            tile[c * (TP + 1) + pl] = x;
            s += (double)x * (double)x;
        }
    part[pt][pl] = s;
    __syncthreads();
    if (threadIdx.x < TP) {
        double t = part[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < PARTS; ++k) t += part[k][threadIdx.x];
        const float n = (float)sqrt(t);
        nrm[threadIdx.x] = n < NM_EPS ? NM_EPS : n;
    }
    __syncthreads();
    float* dst = out + (size_t)p0 * C;                           // the tile's token rows are one contiguous run of np * C floats
    for (int i = threadIdx.x; i < np * C; i += FR_BLOCK) {
        const int p = i / C, c = i - p * C;
        dst[i] = tile[c * (TP + 1) + p] / nrm[p];
    }
}

// dense backward: g [P, C] goes through the LDS tile (transposed), x stays in registers (lanes along p on both of its sides)
template <int TP>
__global__ void __launch_bounds__(FR_BLOCK) rows_normalize_backward_kernel(int C, long long P, const float* __restrict__ in,
                                                                           const float* __restrict__ g, float* __restrict__ grad_in) {
    constexpr int PARTS = FR_BLOCK / TP;
    constexpr int PER = FR_MAX_C * TP / FR_BLOCK / (TP == 64 ? 2 : 1);    // channels per thread: 32 (TP 64: C <= 128; TP 32: C <= 256)
    __shared__ float tile[NM_TILE_WORDS];
    __shared__ double part_xx[PARTS][TP], part_gx[PARTS][TP];
    __shared__ double nrm[TP], dot[TP];
    const long long p0 = (long long)blockIdx.x * TP;
    const int np = (int)(P - p0 < TP ? P - p0 : TP);
    const float* src = g + (size_t)p0 * C;
    for (int i = threadIdx.x; i < np * C; i += FR_BLOCK) {
        const int p = i / C, c = i - p * C;
        tile[c * (TP + 1) + p] = src[i];
    }
    __syncthreads();
    const int pl = threadIdx.x % TP, pt = threadIdx.x / TP;
    float x[PER];
    double sxx = 0.0, sgx = 0.0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int c = pt + k * PARTS;
        x[k] = (pl < np && c < C) ? in[(size_t)c * P + p0 + pl] : 0.0f;
        if (pl < np && c < C) {
            sxx += (double)x[k] * (double)x[k];
            sgx += (double)tile[c * (TP + 1) + pl] * (double)x[k];
        }
    }
    part_xx[pt][pl] = sxx;
    part_gx[pt][pl] = sgx;
    __syncthreads();
    if (threadIdx.x < TP) {
        double a = part_xx[0][threadIdx.x], b = part_gx[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < PARTS; ++k) { a += part_xx[k][threadIdx.x]; b += part_gx[k][threadIdx.x]; }
        float n = (float)sqrt(a);
        n = n < NM_EPS ? NM_EPS : n;
        nrm[threadIdx.x] = (double)n;
        dot[threadIdx.x] = b / (double)n;                        // <g, y>
    }
    __syncthreads();
    if (pl < np) {
        const double n = nrm[pl], d = dot[pl];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int c = pt + k * PARTS;
            if (c < C) grad_in[(size_t)c * P + p0 + pl] = (float)(((double)tile[c * (TP + 1) + pl] - ((double)x[k] / n) * d) / n);
        }
    }
}

// sparse backward: one workgroup per list entry, thread c = channel c.  The FIRST occurrence of a row sums the gradient rows of all its
// occurrences in list order and writes the column; later occurrences do nothing.  grad_in was zero-filled by the entry.
__global__ void __launch_bounds__(FR_BLOCK) rows_normalize_backward_rows_kernel(int C, long long P, int K, const float* __restrict__ in,
                                                                                const int64_t* __restrict__ rows, const float* __restrict__ g,
                                                                                float* __restrict__ grad_in, unsigned* status) {
    __shared__ double s_w[2][FR_BLOCK / WAVE];
    const int k = blockIdx.x, c = threadIdx.x;
    const long long r = rows[k];
    if (r < 0 || r >= P) {                                       // skipped, and reported by dr_device_status
        if (c == 0) atomicOr(status, FRONT_STATUS_BAD_INDEX);
        return;
    }
    for (int j = 0; j < k; ++j)
        if (rows[j] == r) return;                                // uniform over the workgroup
    double gs = 0.0;
    for (int j = k; j < K; ++j)
        if (rows[j] == r && c < C) gs += (double)g[(size_t)j * C + c];
    const double x = c < C ? (double)in[(size_t)c * P + r] : 0.0;
    double sxx = wave_sum(x * x), sgx = wave_sum(gs * x);
    if (lane_id() == 0) { s_w[0][wave_id()] = sxx; s_w[1][wave_id()] = sgx; }
    __syncthreads();
    sxx = s_w[0][0]; sgx = s_w[1][0];
#pragma unroll
    for (int w = 1; w < FR_BLOCK / WAVE; ++w) { sxx += s_w[0][w]; sgx += s_w[1][w]; }
    float nf = (float)sqrt(sxx);
    nf = nf < NM_EPS ? NM_EPS : nf;
    const double n = (double)nf, d = sgx / n;
    if (c < C) grad_in[(size_t)c * P + r] = (float)((gs - (x / n) * d) / n);
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_back_project_f32(int H, int W, const float* depth, const float* intrinsics, int mode, float a, float b, const float* a_dev,
                        const float* b_dev, int has_limit, float depth_limit, float* points, uint8_t* mask, float* pixels, void* stream) {
    if (H < 0 || W < 0 || (mode != 0 && mode != 1)) return DR_EINVAL;
    if (!intrinsics || ((!depth || !points || !mask) && H > 0 && W > 0)) return DR_EINVAL;
    const long long n = (long long)H * W;
    if (n == 0) return DR_OK;
    if (n > (1ll << 31) - 4) return DR_ENOSUP;
    BackProjectArgs A{};
    A.depth = depth; A.K = intrinsics; A.a_dev = a_dev; A.b_dev = b_dev; A.a = a; A.b = b; A.limit = depth_limit;
    A.mode = mode; A.has_limit = has_limit ? 1 : 0; A.W = W; A.n = n; A.points = points; A.mask = mask; A.pixels = pixels;
    const long long groups = (n + 3) / 4;
    long long blocks = (groups + FR_BLOCK - 1) / FR_BLOCK;
    const long long cap = (long long)device_cu_count() * 8;
    if (blocks > cap) blocks = cap;
    const bool vec = aligned16(depth) && aligned16(points) && aligned16(pixels) && ((((uintptr_t)mask) & 3u) == 0);
    if (vec) back_project_kernel<true><<<(unsigned)blocks, FR_BLOCK, 0, (hipStream_t)stream>>>(A);
    else back_project_kernel<false><<<(unsigned)blocks, FR_BLOCK, 0, (hipStream_t)stream>>>(A);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_render_f32(int N, const float* points, const float* intrinsics, const float* extrinsics, float eps, float* pixels, float* depth,
                  void* stream) {
    if (N < 0 || !intrinsics || ((!points || !pixels) && N > 0)) return DR_EINVAL;
    if (N == 0) return DR_OK;
    render_kernel<<<(N + FR_BLOCK - 1) / FR_BLOCK, FR_BLOCK, 0, (hipStream_t)stream>>>(N, points, intrinsics, extrinsics, eps, pixels, depth);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

static int resize_check(int C, int Hs, int Ws, int Hd, int Wd, const void* a, const void* b) {
    if (C < 0 || Hs < 0 || Ws < 0 || Hd < 0 || Wd < 0) return DR_EINVAL;
    if ((long long)Hs * Ws > (1ll << 24) || (long long)Hd * Wd > (1ll << 24) || C > (1 << 20)) return DR_ENOSUP;
    if ((long long)C * Hd * Wd > 0 && ((long long)Hs * Ws == 0 || !a || !b)) return DR_EINVAL;      // nothing to sample from
    return DR_OK;
}

int dr_resize_tokens_f32(int C, int Hs, int Ws, int Hd, int Wd, const float* in, float* out, void* stream) {
    const int rc = resize_check(C, Hs, Ws, Hd, Wd, in, out);
    if (rc != DR_OK) return rc;
    if ((long long)C * Hd * Wd == 0) return DR_OK;
    const dim3 grid((Hd * Wd + RS_TP - 1) / RS_TP, (C + RS_TC - 1) / RS_TC);
    resize_tokens_kernel<<<grid, FR_BLOCK, 0, (hipStream_t)stream>>>(C, Hs, Ws, Hd, Wd, in, out);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_resize_tokens_backward_f32(int C, int Hs, int Ws, int Hd, int Wd, const float* grad_out, float* grad_in, void* stream) {
    if (C < 0 || Hs < 0 || Ws < 0 || Hd < 0 || Wd < 0) return DR_EINVAL;
    if ((long long)Hs * Ws > (1ll << 24) || (long long)Hd * Wd > (1ll << 24) || C > (1 << 20)) return DR_ENOSUP;
    if ((long long)C * Hs * Ws == 0) return DR_OK;
    if (!grad_in || (!grad_out && (long long)Hd * Wd > 0)) return DR_EINVAL;
    const dim3 grid((Hs * Ws + RS_TP - 1) / RS_TP, (C + RS_TC - 1) / RS_TC);
    resize_tokens_backward_kernel<<<grid, FR_BLOCK, 0, (hipStream_t)stream>>>(C, Hs, Ws, Hd, Wd, grad_out, grad_in);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

static int normalize_check(int C, long long P) {
    if (C < 0 || P < 0) return DR_EINVAL;
    if (C > FR_MAX_C || P > (1ll << 31) - 64) return DR_ENOSUP;
    return DR_OK;
}

int dr_rows_normalize_chw_f32(int C, int64_t P, const float* in, float* out, void* stream) {
    const int rc = normalize_check(C, P);
    if (rc != DR_OK) return rc;
    if ((long long)C * P == 0) return DR_OK;
    if (!in || !out) return DR_EINVAL;
    if (C <= 128) rows_normalize_kernel<64><<<(unsigned)((P + 63) / 64), FR_BLOCK, 0, (hipStream_t)stream>>>(C, P, in, out);
    else rows_normalize_kernel<32><<<(unsigned)((P + 31) / 32), FR_BLOCK, 0, (hipStream_t)stream>>>(C, P, in, out);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_rows_normalize_chw_backward_f32(int C, int64_t P, const float* in, const float* grad_out, float* grad_in, void* stream) {
    const int rc = normalize_check(C, P);
    if (rc != DR_OK) return rc;
    if ((long long)C * P == 0) return DR_OK;
    if (!in || !grad_out || !grad_in) return DR_EINVAL;
    if (C <= 128) rows_normalize_backward_kernel<64><<<(unsigned)((P + 63) / 64), FR_BLOCK, 0, (hipStream_t)stream>>>(C, P, in, grad_out, grad_in);
    else rows_normalize_backward_kernel<32><<<(unsigned)((P + 31) / 32), FR_BLOCK, 0, (hipStream_t)stream>>>(C, P, in, grad_out, grad_in);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

int dr_rows_normalize_chw_backward_rows_f32(int C, int64_t P, int K, const float* in, const int64_t* rows, const float* grad_rows,
                                            float* grad_in, void* stream) {
    const int rc = normalize_check(C, P);
    if (rc != DR_OK) return rc;
    if (K < 0) return DR_EINVAL;
    if ((long long)C * P == 0) return DR_OK;
    if (!in || !grad_in || ((!rows || !grad_rows) && K > 0)) return DR_EINVAL;
    unsigned* status = device_status_word();
    if (!status) return DR_ELAUNCH;
    DR_HIP_CHECK(hipMemsetAsync(grad_in, 0, (size_t)C * (size_t)P * sizeof(float), (hipStream_t)stream));
    if (K == 0) return DR_OK;
    rows_normalize_backward_rows_kernel<<<K, FR_BLOCK, 0, (hipStream_t)stream>>>(C, P, K, in, rows, grad_rows, grad_in, status);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
