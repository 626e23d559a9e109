// resize_index.h -- the bilinear align_corners=True rule shared by dr_resize_tokens_f32 (front2d3d.hip) and dr_resize_rows_f32 (conv2d.hip): ATen's
// source index and weights in double on the float32 texels, rounded once.  One statement of it, so the two entries agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace dr
