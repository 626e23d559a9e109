// item2d3d_index.h -- every index and bound the 2D-3D dataset-item kernels (item2d3d.hip: dr_corr_2d3d_mutual_f64, dr_corr_2d3d_radius_f64,
// dr_overlap_2d3d_f64) compute, stated once for the device and for the host check (tools/item2d3d_index_check.cpp): the pixel window a cloud
// point's partners can lie in, the walk of a wave's lanes over a window, the image tiles of the pixel-major walk, the LDS stages of the cloud,
// the chunks of the ordered scan, and the carve of the workspace that the size queries and the entry points share.  Outside hipcc the file
// compiles as plain C++.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "carve.h"               // align256

namespace dr {

constexpr int IT_WALK_BLOCK = 256;     // point walk: one wave per cloud point, four points per workgroup
constexpr int IT_WAVE = 64;
constexpr int IT_REV_BLOCK = 128;      // reverse check: one candidate per thread
constexpr int IT_STAGE = 512;          // cloud points per LDS stage of the reverse check (four doubles each: 16 KiB)
constexpr int IT_TILE = 16;            // pixel-major walk: one workgroup per IT_TILE x IT_TILE pixels, one pixel per thread
constexpr int IT_TILE_BLOCK = IT_TILE * IT_TILE;   // = windows tested against the tile per stage
constexpr int IT_SCAN_BLOCK = 256;
constexpr int IT_SCAN_ITEMS = 4;       // consecutive values per thread
constexpr int IT_SCAN_CHUNK = IT_SCAN_BLOCK * IT_SCAN_ITEMS;
constexpr int IT_MAX_PIXELS = 1 << 30; // H W and N stay below these: a flat pixel index, h W + w, and every count of a pixel fit an int32
constexpr int IT_MAX_POINTS = 1 << 28;
constexpr int IT_NO_PIXEL = INT32_MIN; // a render() result that is not a finite value below 2^30 in magnitude: it passes no 2D test

// rows [h0, h1) x columns [w0, w1) of the image; empty when h1 <= h0 or w1 <= w0
struct ItWindow {
    int h0, h1, w0, w1;
};

// [lo, hi] (inclusive, doubles that may lie far outside the image or be infinite) -> the half-open int range clipped to [0, n)
__host__ __device__ inline void it_clip_range(double lo, double hi, int n, int& a, int& b) {
    a = lo <= 0.0 ? 0 : (lo >= (double)n ? n : (int)lo);
    b = hi < 0.0 ? 0 : (hi >= (double)(n - 1) ? n : (int)hi + 1);
    if (b < a) b = a;
}

// smallest and largest of a s / z over the four corners s in {s0, s1}, z in {z0, z1} (z0, z1 > 0: s / z is monotone in either argument, so the
// corners bound it over the whole rectangle)
__host__ __device__ inline void it_corner_range(double a, double s0, double s1, double z0, double z1, double& lo, double& hi) {
    const double c0 = a * s0 / z0, c1 = a * s0 / z1, c2 = a * s1 / z0, c3 = a * s1 / z1;
    lo = fmin(fmin(c0, c1), fmin(c2, c3));
    hi = fmax(fmax(c0, c1), fmax(c2, c3));
}

// The pixels whose image point p can lie closer than r to the cloud point q = (qx, qy, qz) (camera frame).  |p - q| < r needs |px - qx| < r,
// |py - qy| < r and |pz - qz| < r.  With pz in (qz - r, qz + r) and qz > r the column obeys w - cx = fx px / pz, which lies between the corner
// values of fx (qx +- r) / (qz +- r); the row obeys (h + w / W) - cy = fy py / pz likewise, and h <= h + w / W < h + 1.  The range is widened
// by one pixel for the rounding of the kernel's arithmetic and by one more row for the fractional part of v, then clipped to the image.
//   qz <= -r: no pixel (an image point has pz > 0, so pz - qz > r);   -r < qz <= r, or anything not finite: the whole image.
__host__ __device__ inline ItWindow it_window(int H, int W, double fx, double fy, double cx, double cy, double qx, double qy, double qz,
                                              double r) {
    ItWindow all = {0, H, 0, W}, none = {0, 0, 0, 0};
    if (!(r > 0.0)) return none;                                   // d < r has no solution (r <= 0) or r is NaN
    const double span = (fabs(qx) + fabs(qy)) + (fabs(qz) + r) + (fabs(fx) + fabs(fy)) + (fabs(cx) + fabs(cy));
    if (!(span < INFINITY)) return all;                            // an infinity or a NaN among the inputs
    if (qz <= -r) return none;
    if (!(qz > r) || !(qz - r > 0.0)) return all;
    double lo, hi;
    ItWindow k;
    it_corner_range(fx, qx - r, qx + r, qz - r, qz + r, lo, hi);
    if (!(lo == lo) || !(hi == hi)) return all;
    it_clip_range(floor(lo + cx) - 1.0, ceil(hi + cx) + 1.0, W, k.w0, k.w1);
    it_corner_range(fy, qy - r, qy + r, qz - r, qz + r, lo, hi);
    if (!(lo == lo) || !(hi == hi)) return all;
    it_clip_range(floor(lo + cy) - 2.0, ceil(hi + cy) + 1.0, H, k.h0, k.h1);
    return k;
}

__host__ __device__ inline long long it_window_area(const ItWindow& k) {
    return (k.h1 <= k.h0 || k.w1 <= k.w0) ? 0 : (long long)(k.h1 - k.h0) * (k.w1 - k.w0);
}

// the t-th pixel of a window in row-major order (0 <= t < area): ascending t is ascending flat index h W + w
__host__ __device__ inline void it_window_pixel(const ItWindow& k, long long t, int& h, int& w) {
    const int ww = k.w1 - k.w0;
    h = k.h0 + (int)(t / ww);
    w = k.w0 + (int)(t % ww);
}

__host__ __device__ inline bool it_window_has(const ItWindow& k, int h, int w) { return h >= k.h0 && h < k.h1 && w >= k.w0 && w < k.w1; }

// image tiles of the pixel-major walk
__host__ __device__ inline int it_tiles(int n) { return n <= 0 ? 0 : (n + IT_TILE - 1) / IT_TILE; }
__host__ __device__ inline bool it_window_hits_tile(const ItWindow& k, int th, int tw) {
    return k.h0 < (th + 1) * IT_TILE && k.h1 > th * IT_TILE && k.w0 < (tw + 1) * IT_TILE && k.w1 > tw * IT_TILE && it_window_area(k) > 0;
}
// thread t of tile (th, tw) -> its pixel; false outside the image
__host__ __device__ inline bool it_tile_pixel(int H, int W, int th, int tw, int t, int& h, int& w) {
    h = th * IT_TILE + t / IT_TILE;
    w = tw * IT_TILE + t % IT_TILE;
    return h < H && w < W;
}

// points of the stage of `size` that starts at k0 of a cloud of n: min(size, n - k0), never negative
__host__ __device__ inline int it_stage_count(int n, int k0, int size) {
    const int left = n - k0;
    return left <= 0 ? 0 : (left < size ? left : size);
}

// the ordered scan over n values: chunks of IT_SCAN_CHUNK, thread t of chunk c owns values [it_scan_first(c, t), + IT_SCAN_ITEMS) below n
__host__ __device__ inline int it_scan_chunks(long long n) { return n <= 0 ? 0 : (int)((n + IT_SCAN_CHUNK - 1) / IT_SCAN_CHUNK); }
__host__ __device__ inline long long it_scan_first(int chunk, int t) { return (long long)chunk * IT_SCAN_CHUNK + (long long)t * IT_SCAN_ITEMS; }
// what a stored int32 counts for: IT_SCAN_SET v >= 0 (a pixel's partner, -1 = none), IT_SCAN_SUM v itself (a pixel's pair count),
// IT_SCAN_POS v > 0 (a flag)
constexpr int IT_SCAN_SET = 0, IT_SCAN_SUM = 1, IT_SCAN_POS = 2;
__host__ __device__ inline long long it_scan_value(int mode, int v) {
    return mode == IT_SCAN_SUM ? (v > 0 ? v : 0) : (mode == IT_SCAN_SET ? (v >= 0 ? 1 : 0) : (v > 0 ? 1 : 0));
}
__host__ __device__ inline int it_saturate_i32(long long v) { return v > 0x7fffffffLL ? 0x7fffffff : (int)v; }

// the workspace of the three entries (one layout): per cloud point its camera-frame coordinates, window, render() pixel and one int32 (mutual: the
// candidate pixel, overlap: the flag); per pixel one int32 (mutual: the partner, radius / overlap: the pair count); the scan's exclusive offsets
// over max(H W, N) values and its chunk sums
struct ItCarve {
    size_t pts, win, rpx, pnt, pix, off, sums, bytes;
};
__host__ __device__ inline ItCarve it_carve(int H, int W, int N) {
    ItCarve c;
    const size_t n = N > 0 ? (size_t)N : 0, p = (H > 0 && W > 0) ? (size_t)H * (size_t)W : 0, m = n > p ? n : p;
    c.pts = 0;
    c.win = c.pts + align256(n * 4 * sizeof(double));
    c.rpx = c.win + align256(n * 4 * sizeof(int32_t));
    c.pnt = c.rpx + align256(n * 2 * sizeof(int32_t));
    c.pix = c.pnt + align256(n * sizeof(int32_t));
    c.off = c.pix + align256(p * sizeof(int32_t));
    c.sums = c.off + align256(m * sizeof(int64_t));
    c.bytes = c.sums + align256((size_t)it_scan_chunks((long long)m) * sizeof(int64_t));
    return c;
}

}  // namespace dr
