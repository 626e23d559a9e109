// item2d3d.hip -- the pixel-point ground truth of a 2D-3D dataset item on the device (thirteenth set after ABI 0.7.0):
//   dr_corr_2d3d_mutual_f64   get_2d3d_correspondences_mutual                         2D-3D vision3d/array_ops/registration_utils.py:30-60
//   dr_corr_2d3d_radius_f64   get_2d3d_correspondences_radius                         registration_utils.py:63-89
//   dr_overlap_2d3d_f64       the two np.unique lists of return_overlap_indices       datasets/registration/sevenscenes/sevenscenes_hard.py:184-196
//   dr_column_mean_seq_f32    center = points.mean(axis=0) of the augmentation        sevenscenes_hard.py:140
// with what they call: back_project and render (array_ops/depth_image.py:9-65, 68-99), apply_transform (array_ops/se3.py:7-17), mutual_select
// (array_ops/mutual_select.py:7-35).  The reference builds two cKDTrees per item on a loader worker; here the image points are never stored:
// they lie on the pixel grid, so a cloud point's partners are found in a bounded pixel window (item2d3d_index.h).
//
// All arithmetic is float64 and unfused, operation by operation as numpy performs it.  Asynchronous on the given stream; nothing synchronises,
// allocates or reads back to the host.  No atomics of any kind: every output row has one writer whose position comes from an ordered scan, so
// two runs are bit-equal.  Every index comes from item2d3d_index.h (walked on the host by tools/item2d3d_index_check.cpp).
//
//   prep      per cloud point: q = T p, its window, its render() pixel (truncated, as .astype(int) does)
//   walk      one wave per cloud point; the lanes walk the window, a wave reduction on (d^2, flat pixel) picks the nearest pixel inside radius_3d
//   reverse   one candidate pixel per thread against the whole cloud, streamed through LDS in stages (a broadcast read per point)
//   tiles     (radius, overlap) one workgroup per 16 x 16 pixels: the windows that touch the tile are compacted into LDS in ascending point
//             order, every pixel walks that list -- the window walk transposed, which gives the pixel-major order without a sort
//   scan      chunk sums, one workgroup over the chunk sums, exclusive offsets per value; the writers then place every row by its offset
#include "common.h"
#include "item2d3d_index.h"
#include "../../include/diffreg_hip.h"

// The float64 expressions restate numpy operation by operation: no a * b + c below becomes an FMA.
#pragma clang fp contract(off)

namespace dr {

struct ItArgs {
    int H, W, N, pts_f64;
    const float* depth;
    double scale, limit;
    const double* K;            // intrinsics [9], device
    const void* points;         // [N, 3] float32 or float64
    const double* T;            // transform [16], device
    double r2d, r3d;
    double* pts;                // [N, 4]: q = T p (camera frame), w unused
    ItWindow* win;              // [N]
    int* rpx;                   // [N, 2]: render(q) = (h, w), IT_NO_PIXEL when unusable
    int* pnt;                   // [N]
    int* pix;                   // [H W]
    long long* off;             // [max(H W, N)]
    long long* sums;            // [chunks]
    long long cap;
    long long* out_pix;         // [cap, 2] or [cap]
    long long* out_idx;         // [cap]
    int* counts;                // [2]: written, found
};

struct ItCamera {
    double fx, fy, cx, cy;
};
__device__ __forceinline__ ItCamera it_camera(const double* K) { return {K[0], K[4], K[2], K[5]}; }

// back_project (depth_image.py:36-45) of pixel (h, w): z = depth / scaling_factor, z > limit -> 0; u = coords % width, v = coords / width (a
// TRUE division: v keeps the fraction w / W); x = (u - cx) z / fx, y = (v - cy) z / fy.  false where z > 0 does not hold (the pixel is no point).
__device__ __forceinline__ bool it_image_point(const ItArgs& A, const ItCamera& c, int h, int w, double& x, double& y, double& z) {
    const int flat = h * A.W + w;
    z = (double)A.depth[flat] / A.scale;
    if (z > A.limit) z = 0.0;
    if (!(z > 0.0)) return false;
    const double v = (double)flat / (double)A.W;
    x = ((double)w - c.cx) * z / c.fx;
    y = (v - c.cy) * z / c.fy;
    return true;
}

// ((dx dx + dy dy) + dz dz) with d = image point - cloud point, the same bits in the walk and in the reverse check
__device__ __forceinline__ double it_d2(double px, double py, double pz, double qx, double qy, double qz) {
    const double dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// np.linalg.norm(img_pixel - render_pixel) < radius_2d on integer pixels (registration_utils.py:55, 85)
__device__ __forceinline__ bool it_near_2d(int h, int w, int rh, int rw, double r2d) {
    if (rh == IT_NO_PIXEL || rw == IT_NO_PIXEL) return false;
    const long long dh = (long long)h - rh, dw = (long long)w - rw;
    return sqrt((double)(dh * dh + dw * dw)) < r2d;
}

// .astype(int): truncation toward zero; anything not finite or beyond 2^30 is IT_NO_PIXEL (numpy's cast is undefined there)
__device__ __forceinline__ int it_trunc_pixel(double v) { return (fabs(v) < 1073741824.0) ? (int)v : IT_NO_PIXEL; }

// ------------------------------------------------------------------------------------------------------------
// prep: cloud points into the camera frame, their windows and render() pixels; per-pixel word reset
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void it_prep_kernel(ItArgs A, int pix_fill) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long long)A.H * A.W) A.pix[i] = pix_fill;
    if (i >= A.N) return;
    double x, y, z;
    if (A.pts_f64) {
        const double* p = (const double*)A.points + i * 3;
        x = p[0]; y = p[1]; z = p[2];
    } else {
        const float* p = (const float*)A.points + i * 3;
        x = p[0]; y = p[1]; z = p[2];
    }
    const double* T = A.T;      // apply_transform: points @ R.T + t
    const double qx = ((x * T[0] + y * T[1]) + z * T[2]) + T[3];
    const double qy = ((x * T[4] + y * T[5]) + z * T[6]) + T[7];
    const double qz = ((x * T[8] + y * T[9]) + z * T[10]) + T[11];
    double* o = A.pts + i * 4;
    o[0] = qx; o[1] = qy; o[2] = qz; o[3] = 0.0;
    const ItCamera c = it_camera(A.K);
    A.win[i] = it_window(A.H, A.W, c.fx, c.fy, c.cx, c.cy, qx, qy, qz, A.r3d);
    A.rpx[i * 2 + 0] = it_trunc_pixel(c.fy * qy / qz + c.cy);       // depth_image.py:92-94
    A.rpx[i * 2 + 1] = it_trunc_pixel(c.fx * qx / qz + c.cx);
    A.pnt[i] = -1;
}

// ------------------------------------------------------------------------------------------------------------
// walk: one wave per cloud point over its window.  MODE 0: the nearest pixel closer than radius_3d (-1: none); equal d^2 go to the lowest flat
// pixel index.  MODE 1: is there a pixel closer than radius_3d that also passes the 2D test (0 / 1)
// ------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(IT_WALK_BLOCK) void it_walk_kernel(ItArgs A) {
    const int j = blockIdx.x * (IT_WALK_BLOCK / WAVE) + wave_id();
    if (j >= A.N) return;                                           // uniform over the wave
    const ItCamera c = it_camera(A.K);
    const double qx = A.pts[(size_t)j * 4], qy = A.pts[(size_t)j * 4 + 1], qz = A.pts[(size_t)j * 4 + 2];
    const ItWindow k = A.win[j];
    const int rh = A.rpx[(size_t)j * 2], rw = A.rpx[(size_t)j * 2 + 1];
    const long long area = it_window_area(k);
    double best = INFINITY;
    int arg = 0x7fffffff;
    bool any = false;
    for (long long t = lane_id(); t < area; t += WAVE) {
        int h, w;
        it_window_pixel(k, t, h, w);
        double px, py, pz;
        if (!it_image_point(A, c, h, w, px, py, pz)) continue;
        const double d = it_d2(px, py, pz, qx, qy, qz);
        if (!(sqrt(d) < A.r3d)) continue;                           // np.linalg.norm(...) < matching_radius_3d
        if (MODE == 0) {
            if (d < best) { best = d; arg = h * A.W + w; }          // a lane's t ascends: equal distances keep the lower index
        } else {
            any = any || it_near_2d(h, w, rh, rw, A.r2d);
        }
    }
    if (MODE == 0) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double od = __shfl_xor(best, m);
            const int oi = __shfl_xor(arg, m);
            if (od < best || (od == best && oi < arg)) { best = od; arg = oi; }
        }
        if (lane_id() == 0) A.pnt[j] = arg == 0x7fffffff ? -1 : arg;
    } else {
        const bool hit = __any(any);
        if (lane_id() == 0) A.pnt[j] = hit ? 1 : 0;
    }
}

// ------------------------------------------------------------------------------------------------------------
// reverse: candidate pixel pnt[j] against all cloud points; kept when its nearest cloud point is j (equal d^2: the lowest index) and the 2D
// test passes -> pix[pixel] = j.  A pixel has one nearest point, so it has one writer.
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IT_REV_BLOCK) void it_reverse_kernel(ItArgs A) {
    __shared__ double s_pts[IT_STAGE * 4];
    const int t = threadIdx.x;
    const int j = blockIdx.x * IT_REV_BLOCK + t;
    const ItCamera c = it_camera(A.K);
    const int cand = j < A.N ? A.pnt[j] : -1;
    double px = 0.0, py = 0.0, pz = 0.0;
    int h = 0, w = 0;
    bool active = cand >= 0;
    if (active) {
        h = cand / A.W;
        w = cand % A.W;
        active = it_image_point(A, c, h, w, px, py, pz);
    }
    double best = INFINITY;
    int arg = -1;
    for (int k0 = 0; k0 < A.N; k0 += IT_STAGE) {
        const int nk = it_stage_count(A.N, k0, IT_STAGE);
        for (int e = t; e < nk * 4; e += IT_REV_BLOCK) s_pts[e] = A.pts[(size_t)k0 * 4 + e];
        __syncthreads();
        if (active) {
            for (int k = 0; k < nk; ++k) {
                const double d = it_d2(px, py, pz, s_pts[k * 4], s_pts[k * 4 + 1], s_pts[k * 4 + 2]);
                if (d < best) { best = d; arg = k0 + k; }           // equal distances keep the lower index
            }
        }
        __syncthreads();
    }
    if (active && arg == j && it_near_2d(h, w, A.rpx[(size_t)j * 2], A.rpx[(size_t)j * 2 + 1], A.r2d)) A.pix[cand] = j;
}

// ------------------------------------------------------------------------------------------------------------
// tiles: the pixel-major walk of the radius variant.  WRITE 0: pix[pixel] = number of pairs; WRITE 1: the pairs from row off[pixel], in ascending
// point index
// ------------------------------------------------------------------------------------------------------------
template <int WRITE>
__global__ __launch_bounds__(IT_TILE_BLOCK) void it_tile_kernel(ItArgs A) {
    __shared__ int s_list[IT_TILE_BLOCK];
    __shared__ int s_wave[IT_TILE_BLOCK / WAVE];
    const int t = threadIdx.x, th = blockIdx.y, tw = blockIdx.x;
    const ItCamera c = it_camera(A.K);
    int h, w;
    const bool inside = it_tile_pixel(A.H, A.W, th, tw, t, h, w);
    double px = 0.0, py = 0.0, pz = 0.0;
    const bool has = inside && it_image_point(A, c, h, w, px, py, pz);
    const int flat = inside ? h * A.W + w : 0;
    long long pos = (WRITE && inside) ? A.off[flat] : 0;
    int n = 0;
    for (int k0 = 0; k0 < A.N; k0 += IT_TILE_BLOCK) {
        const int k = k0 + t;
        const bool hit = k < A.N && it_window_hits_tile(A.win[k], th, tw);
        const unsigned long long b = __ballot(hit);
        if (lane_id() == 0) s_wave[wave_id()] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int v = 0; v < IT_TILE_BLOCK / WAVE; ++v) {
            const int cnt = s_wave[v];
            before += v < wave_id() ? cnt : 0;
            total += cnt;
        }
        if (hit) s_list[before + __popcll(b & ((1ull << lane_id()) - 1ull))] = k;
        __syncthreads();
        if (has) {
            for (int m = 0; m < total; ++m) {
                const int q = s_list[m];
                if (!it_window_has(A.win[q], h, w)) continue;
                const double* p = A.pts + (size_t)q * 4;
                if (!(sqrt(it_d2(px, py, pz, p[0], p[1], p[2])) < A.r3d)) continue;
                if (!it_near_2d(h, w, A.rpx[(size_t)q * 2], A.rpx[(size_t)q * 2 + 1], A.r2d)) continue;
                if (WRITE) {
                    if (pos < A.cap) {
                        A.out_pix[pos * 2] = h;
                        A.out_pix[pos * 2 + 1] = w;
                        A.out_idx[pos] = q;
                    }
                    ++pos;
                } else {
                    ++n;
                }
            }
        }
        __syncthreads();
    }
    if (!WRITE && inside) A.pix[flat] = n;
}

// ------------------------------------------------------------------------------------------------------------
// the ordered scan over n int32 words (it_scan_value says what a word counts for)
// ------------------------------------------------------------------------------------------------------------
// exclusive prefix of v over the workgroup (IT_SCAN_BLOCK threads) and the workgroup's total; s_wave holds one entry per wave
__device__ __forceinline__ long long it_block_exclusive(long long v, long long* s_wave, long long& total) {
    long long inc = v;
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const long long o = __shfl_up(inc, d);
        if (lane_id() >= d) inc += o;
    }
    __syncthreads();                                                // the previous use of s_wave is over
    if (lane_id() == WAVE - 1) s_wave[wave_id()] = inc;
    __syncthreads();
    long long before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < IT_SCAN_BLOCK / WAVE; ++w) {
        const long long s = s_wave[w];
        before += w < wave_id() ? s : 0;
        total += s;
    }
    return before + inc - v;
}

__global__ __launch_bounds__(IT_SCAN_BLOCK) void it_scan_sums_kernel(const int* val, long long n, int mode, long long* sums) {
    __shared__ long long s_wave[IT_SCAN_BLOCK / WAVE];
    const long long first = it_scan_first(blockIdx.x, threadIdx.x);
    long long s = 0;
#pragma unroll
    for (int e = 0; e < IT_SCAN_ITEMS; ++e)
        if (first + e < n) s += it_scan_value(mode, val[first + e]);
    long long total;
    it_block_exclusive(s, s_wave, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: chunk sums -> exclusive chunk offsets; counts = (min(found, cap), found saturated to int32)
__global__ __launch_bounds__(IT_SCAN_BLOCK) void it_scan_top_kernel(long long* sums, int chunks, long long cap, int* counts) {
    __shared__ long long s_wave[IT_SCAN_BLOCK / WAVE];
    long long running = 0;
    for (int c0 = 0; c0 < chunks; c0 += IT_SCAN_BLOCK) {
        const int c = c0 + threadIdx.x;
        const long long v = c < chunks ? sums[c] : 0;
        long long total;
        const long long ex = it_block_exclusive(v, s_wave, total);
        if (c < chunks) sums[c] = running + ex;
        running += total;
    }
    if (threadIdx.x == 0) {
        counts[0] = it_saturate_i32(running < cap ? running : cap);
        counts[1] = it_saturate_i32(running);
    }
}

__global__ __launch_bounds__(IT_SCAN_BLOCK) void it_scan_offsets_kernel(const int* val, long long n, int mode, const long long* sums,
                                                                        long long* off) {
    __shared__ long long s_wave[IT_SCAN_BLOCK / WAVE];
    const long long first = it_scan_first(blockIdx.x, threadIdx.x);
    long long v[IT_SCAN_ITEMS], s = 0;
#pragma unroll
    for (int e = 0; e < IT_SCAN_ITEMS; ++e) {
        v[e] = first + e < n ? it_scan_value(mode, val[first + e]) : 0;
        s += v[e];
    }
    long long total;
    long long at = sums[blockIdx.x] + it_block_exclusive(s, s_wave, total);
#pragma unroll
    for (int e = 0; e < IT_SCAN_ITEMS; ++e) {
        if (first + e < n) off[first + e] = at;
        at += v[e];
    }
}

// writers behind the scan.  PAIRS 1: pixel i with partner pix[i] >= 0 -> (h, w), partner;  PAIRS 0: index i of every word > 0
template <int PAIRS>
__global__ __launch_bounds__(256) void it_emit_kernel(const int* val, long long n, int W, const long long* off, long long cap,
                                                      long long* out_a, long long* out_b) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int v = val[i];
    const long long r = off[i];
    if (r >= cap) return;
    if (PAIRS) {
        if (v < 0) return;
        out_a[r * 2] = i / W;
        out_a[r * 2 + 1] = i % W;
        out_b[r] = v;
    } else {
        if (v <= 0) return;
        out_a[r] = i;
    }
}

// points.mean(axis=0) of a C-ordered float32 [n, 3] array as numpy performs it: a reduction over the OUTER axis adds row after row (no pairwise
// blocks), then divides by n in float32.  One workgroup; the rows pass through LDS, three threads keep the running sums.
__global__ __launch_bounds__(256) void it_column_mean_kernel(int n, const float* __restrict__ x, float* __restrict__ out) {
    __shared__ float s_rows[IT_STAGE * 3];
    float sum = 0.f;
    for (int k0 = 0; k0 < n; k0 += IT_STAGE) {
        const int nk = it_stage_count(n, k0, IT_STAGE);
        for (int e = threadIdx.x; e < nk * 3; e += 256) s_rows[e] = x[(size_t)k0 * 3 + e];
        __syncthreads();
        if (threadIdx.x < 3)
            for (int k = 0; k < nk; ++k) sum = sum + s_rows[k * 3 + threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < 3) out[threadIdx.x] = sum / (float)n;
}

static int it_scan(const int* val, long long n, int mode, const ItArgs& A, long long cap, int* counts, hipStream_t st) {
    const int chunks = it_scan_chunks(n);
    if (chunks > 0) {
        hipLaunchKernelGGL(it_scan_sums_kernel, dim3(chunks), dim3(IT_SCAN_BLOCK), 0, st, val, n, mode, A.sums);
        DR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(it_scan_top_kernel, dim3(1), dim3(IT_SCAN_BLOCK), 0, st, A.sums, chunks, cap, counts);
    DR_LAUNCH_CHECK();
    if (chunks > 0) {
        hipLaunchKernelGGL(it_scan_offsets_kernel, dim3(chunks), dim3(IT_SCAN_BLOCK), 0, st, val, n, mode, (const long long*)A.sums, A.off);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

static unsigned it_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// argument checks shared by the three entries, then the carve -> A
static int it_setup(ItArgs& A, int H, int W, int N, const float* depth, double scaling_factor, double depth_limit, const double* intrinsics,
                    const void* points, int points_f64, const double* transform, double radius_2d, double radius_3d, void* workspace,
                    size_t workspace_bytes) {
    if (H < 0 || W < 0 || N < 0) return DR_EINVAL;
    const long long P = (long long)H * W;
    if (P > IT_MAX_PIXELS || N > IT_MAX_POINTS) return DR_ENOSUP;
    if (!intrinsics || !transform || (P > 0 && !depth) || (N > 0 && !points)) return DR_EINVAL;
    if (!aligned_to(depth, 4) || !aligned_to(intrinsics, 8) || !aligned_to(transform, 8) || !aligned_to(points, points_f64 ? 8 : 4))
        return DR_EINVAL;
    const ItCarve c = it_carve(H, W, N);
    if (c.bytes > 0 && (!workspace || workspace_bytes < c.bytes)) return DR_EWORKSPACE;
    if (!aligned_to(workspace, 32)) return DR_EINVAL;
    char* w = (char*)workspace;
    A.H = H; A.W = W; A.N = N; A.pts_f64 = points_f64 ? 1 : 0;
    A.depth = depth; A.scale = scaling_factor; A.limit = depth_limit;
    A.K = intrinsics; A.points = points; A.T = transform;
    A.r2d = radius_2d; A.r3d = radius_3d;
    A.pts = (double*)(w + c.pts); A.win = (ItWindow*)(w + c.win); A.rpx = (int*)(w + c.rpx); A.pnt = (int*)(w + c.pnt);
    A.pix = (int*)(w + c.pix); A.off = (long long*)(w + c.off); A.sums = (long long*)(w + c.sums);
    A.cap = 0; A.out_pix = nullptr; A.out_idx = nullptr; A.counts = nullptr;
    return DR_OK;
}

static int it_prep(const ItArgs& A, int pix_fill, hipStream_t st) {
    const long long P = (long long)A.H * A.W, m = P > A.N ? P : A.N;
    if (m > 0) {
        hipLaunchKernelGGL(it_prep_kernel, dim3(it_blocks(m, 256)), dim3(256), 0, st, A, pix_fill);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_column_mean_seq_f32(int n, const float* x, float* out, void* stream) {
    if (n <= 0 || !x || !out || n > IT_MAX_POINTS) return DR_EINVAL;
    hipLaunchKernelGGL(it_column_mean_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n, x, out);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

size_t dr_corr_2d3d_mutual_workspace_bytes(int H, int W, int N) { return it_carve(H, W, N).bytes; }
size_t dr_corr_2d3d_radius_workspace_bytes(int H, int W, int N) { return it_carve(H, W, N).bytes; }
size_t dr_overlap_2d3d_workspace_bytes(int H, int W, int N) { return it_carve(H, W, N).bytes; }

int dr_corr_2d3d_mutual_f64(int H, int W, int N, const float* depth, double scaling_factor, double depth_limit, const double* intrinsics,
                            const void* points, int points_f64, const double* transform, double radius_2d, double radius_3d, long long cap,
                            int64_t* img_corr_pixels, int64_t* pcd_corr_indices, int32_t* counts, void* workspace, size_t workspace_bytes,
                            void* stream) {
    ItArgs A;
    const int rc = it_setup(A, H, W, N, depth, scaling_factor, depth_limit, intrinsics, points, points_f64, transform, radius_2d, radius_3d,
                            workspace, workspace_bytes);
    if (rc != DR_OK) return rc;
    if (cap < 0 || !counts || (cap > 0 && (!img_corr_pixels || !pcd_corr_indices))) return DR_EINVAL;
    A.cap = cap; A.out_pix = (long long*)img_corr_pixels; A.out_idx = (long long*)pcd_corr_indices; A.counts = counts;
    hipStream_t st = (hipStream_t)stream;
    const long long P = (long long)H * W;
    int e = it_prep(A, -1, st);
    if (e != DR_OK) return e;
    if (N > 0 && P > 0) {
        hipLaunchKernelGGL(it_walk_kernel<0>, dim3(it_blocks(N, IT_WALK_BLOCK / WAVE)), dim3(IT_WALK_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
        hipLaunchKernelGGL(it_reverse_kernel, dim3(it_blocks(N, IT_REV_BLOCK)), dim3(IT_REV_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    e = it_scan(A.pix, P, IT_SCAN_SET, A, cap, counts, st);
    if (e != DR_OK) return e;
    if (P > 0 && cap > 0) {
        hipLaunchKernelGGL(it_emit_kernel<1>, dim3(it_blocks(P, 256)), dim3(256), 0, st, (const int*)A.pix, P, W, (const long long*)A.off, cap,
                           A.out_pix, A.out_idx);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

int dr_corr_2d3d_radius_f64(int H, int W, int N, const float* depth, double scaling_factor, double depth_limit, const double* intrinsics,
                            const void* points, int points_f64, const double* transform, double radius_2d, double radius_3d, long long cap,
                            int64_t* img_corr_pixels, int64_t* pcd_corr_indices, int32_t* counts, void* workspace, size_t workspace_bytes,
                            void* stream) {
    ItArgs A;
    const int rc = it_setup(A, H, W, N, depth, scaling_factor, depth_limit, intrinsics, points, points_f64, transform, radius_2d, radius_3d,
                            workspace, workspace_bytes);
    if (rc != DR_OK) return rc;
    if (cap < 0 || !counts || (cap > 0 && (!img_corr_pixels || !pcd_corr_indices))) return DR_EINVAL;
    A.cap = cap; A.out_pix = (long long*)img_corr_pixels; A.out_idx = (long long*)pcd_corr_indices; A.counts = counts;
    hipStream_t st = (hipStream_t)stream;
    const long long P = (long long)H * W;
    int e = it_prep(A, 0, st);
    if (e != DR_OK) return e;
    const dim3 tiles(it_tiles(W), it_tiles(H));
    if (N > 0 && P > 0) {
        hipLaunchKernelGGL(it_tile_kernel<0>, tiles, dim3(IT_TILE_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    e = it_scan(A.pix, P, IT_SCAN_SUM, A, cap, counts, st);
    if (e != DR_OK) return e;
    if (N > 0 && P > 0 && cap > 0) {
        hipLaunchKernelGGL(it_tile_kernel<1>, tiles, dim3(IT_TILE_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

int dr_overlap_2d3d_f64(int H, int W, int N, const float* depth, double scaling_factor, double depth_limit, const double* intrinsics,
                        const void* points, int points_f64, const double* transform, double radius_2d, double radius_3d, long long cap_img,
                        long long cap_pcd, int64_t* img_overlap_indices, int64_t* pcd_overlap_indices, int32_t* counts, void* workspace,
                        size_t workspace_bytes, void* stream) {
    ItArgs A;
    const int rc = it_setup(A, H, W, N, depth, scaling_factor, depth_limit, intrinsics, points, points_f64, transform, radius_2d, radius_3d,
                            workspace, workspace_bytes);
    if (rc != DR_OK) return rc;
    if (cap_img < 0 || cap_pcd < 0 || !counts || (cap_img > 0 && !img_overlap_indices) || (cap_pcd > 0 && !pcd_overlap_indices)) return DR_EINVAL;
    A.counts = counts;
    hipStream_t st = (hipStream_t)stream;
    const long long P = (long long)H * W;
    int e = it_prep(A, 0, st);
    if (e != DR_OK) return e;
    if (N > 0 && P > 0) {
        hipLaunchKernelGGL(it_tile_kernel<0>, dim3(it_tiles(W), it_tiles(H)), dim3(IT_TILE_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
        hipLaunchKernelGGL(it_walk_kernel<1>, dim3(it_blocks(N, IT_WALK_BLOCK / WAVE)), dim3(IT_WALK_BLOCK), 0, st, A);
        DR_LAUNCH_CHECK();
    }
    e = it_scan(A.pix, P, IT_SCAN_POS, A, cap_img, counts, st);
    if (e != DR_OK) return e;
    if (P > 0 && cap_img > 0) {
        hipLaunchKernelGGL(it_emit_kernel<0>, dim3(it_blocks(P, 256)), dim3(256), 0, st, (const int*)A.pix, P, W, (const long long*)A.off, cap_img,
                           (long long*)img_overlap_indices, (long long*)nullptr);
        DR_LAUNCH_CHECK();
    }
    e = it_scan(A.pnt, N, IT_SCAN_POS, A, cap_pcd, counts + 2, st);
    if (e != DR_OK) return e;
    if (N > 0 && cap_pcd > 0) {
        hipLaunchKernelGGL(it_emit_kernel<0>, dim3(it_blocks(N, 256)), dim3(256), 0, st, (const int*)A.pnt, (long long)N, 1, (const long long*)A.off,
                           cap_pcd, (long long*)pcd_overlap_indices, (long long*)nullptr);
        DR_LAUNCH_CHECK();
    }
    return DR_OK;
}

}  // extern "C"
