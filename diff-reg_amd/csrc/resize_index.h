// resize_index.h -- the bilinear align_corners=True rule shared by dr_resize_tokens_f32 (front2d3d.hip) and dr_resize_rows_f32 (conv2d.hip): ATen's
// source index and weights in double on the float32 texels, rounded once.  One statement of it, so the two entries agree bit for bit; the same
// for the gather of their backwards, dr_resize_tokens_backward_f32 and dr_resize_rows_backward_f32 (resize_gather).  Outside hipcc the file
// compiles as plain C++ (tools/conv_bwd_index_check.cpp walks resize_gather on the host).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#include <cmath>
#define __host__
#define __device__
#define __forceinline__ inline
#endif

namespace dr {

// ATen's area_pixel_compute_source_index with align_corners: scale = (in - 1) / (out - 1), 0 when out == 1
__host__ __device__ inline double resize_scale(int in, int out) { return out > 1 ? (double)(in - 1) / (double)(out - 1) : 0.0; }
__device__ __forceinline__ void resize_src(double scale, int d, int in, int& i0, int& i1, double& l1) {
#pragma clang fp contract(off)
    const double s = scale * d;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - i0;
}
// the blend of the four texels, term by term (no a * b + c becomes an FMA)
__device__ __forceinline__ float resize_blend(double ly, double lx, double v00, double v01, double v10, double v11) {
#pragma clang fp contract(off)
    return (float)((1.0 - ly) * ((1.0 - lx) * v00 + lx * v01) + ly * ((1.0 - lx) * v10 + lx * v11));
}

// the destinations d in [lo, hi] are the only ones whose footprint can hold source index s (widened by one on either side; every
// candidate is then tested with resize_src itself, so forward and backward agree on every footprint)
__device__ __forceinline__ void resize_candidates(double scale, int s, int out, int& lo, int& hi) {
    if (scale <= 0.0) { lo = 0; hi = out - 1; return; }
    lo = (int)floor((s - 1) / scale) - 1;
    hi = (int)ceil((s + 1) / scale) + 1;
    if (lo < 0) lo = 0;
    if (hi > out - 1) hi = out - 1;
}

// The backward as a GATHER: the gradient of source texel (ys, xs) = the sum, over the destination pixels (yd, xd) whose footprint holds it, of
// weight x g_at(yd Wd + xd), rows then columns ascending, in double.  g_at(pd) reads one channel of destination pixel pd in [0, Hd Wd).
template <class F>
__device__ __forceinline__ double resize_gather(double sh, double sw, int ys, int xs, int Hs, int Ws, int Hd, int Wd, F&& g_at) {
    int ylo, yhi, xlo, xhi;
    resize_candidates(sh, ys, Hd, ylo, yhi);
    resize_candidates(sw, xs, Wd, xlo, xhi);
    double acc = 0.0;
    for (int yd = ylo; yd <= yhi; ++yd) {
        int y0, y1, x0, x1;
        double ly, lx;
        resize_src(sh, yd, Hs, y0, y1, ly);
        const double wy = (y0 == ys ? 1.0 - ly : 0.0) + (y1 == ys ? ly : 0.0);
        if (y0 != ys && y1 != ys) continue;
        for (int xd = xlo; xd <= xhi; ++xd) {
            resize_src(sw, xd, Ws, x0, x1, lx);
            if (x0 != xs && x1 != xs) continue;
            const double wx = (x0 == xs ? 1.0 - lx : 0.0) + (x1 == xs ? lx : 0.0);
            acc += wy * wx * (double)g_at(yd * Wd + xd);
        }
    }
    return acc;
}

}  // namespace dr
