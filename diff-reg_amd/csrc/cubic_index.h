// cubic_index.h -- the bicubic resample rule of dr_image_cubic_chw_f32 (image_transform.hip), stated once for the device and for the host check
// (tools/cubic_index_check.cpp): OpenCV's INTER_CUBIC for CV_32F in our own words -- the pixel-centre mapping in double narrowed to float, the
// fraction and the four Keys coefficients (A = -0.75) in float, the taps s-1 .. s+2 clamped to the image (replicate border), no antialiasing, no
// special case at s < 0 -- and the blend of the 16 float32 texels in double, columns first, then rows, rounded once.  Outside hipcc the file
// compiles as plain C++.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#include <cmath>
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#ifndef __forceinline__
#define __forceinline__ inline
#endif
#endif

namespace dr {

// per axis: scale = in / out
__host__ __device__ inline double cubic_scale(int in, int out) { return (double)in / (double)out; }

// destination d of an axis with `in` source texels: s = floor(f), t = f - s with f = (float)((d + 0.5) scale - 0.5)
__host__ __device__ __forceinline__ void cubic_src(double scale, int d, int& s, float& t) {
#pragma clang fp contract(off)
    const float f = (float)(((double)d + 0.5) * scale - 0.5);
    const float fl = floorf(f);
    s = (int)fl;
    t = f - fl;
}

// the four weights of taps s-1, s, s+1, s+2 at fraction t, in float, term by term (no a * b + c becomes an FMA)
__host__ __device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
#pragma clang fp contract(off)
    const float A = -0.75f;
    const float u = t + 1.0f, w = 1.0f - t;
    c[0] = ((A * u - 5.0f * A) * u + 8.0f * A) * u - 4.0f * A;
    c[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
    c[2] = ((A + 2.0f) * w - (A + 3.0f)) * w * w + 1.0f;
    c[3] = 1.0f - c[0] - c[1] - c[2];
}

__host__ __device__ __forceinline__ int cubic_clamp(int i, int in) { return i < 0 ? 0 : (i > in - 1 ? in - 1 : i); }

// everything an axis contributes to destination d: the clamped tap indices and their weights
__host__ __device__ __forceinline__ void cubic_taps(double scale, int d, int in, int idx[4], float c[4]) {
    int s;
    float t;
    cubic_src(scale, d, s, t);
    cubic_coeffs(t, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = cubic_clamp(s - 1 + k, in);
}

// v[row tap][column tap] of one channel: columns first, then rows, in double on the float32 texels, rounded once
__host__ __device__ __forceinline__ float cubic_blend(const float cy[4], const float cx[4], const float v[4][4]) {
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double row = (double)cx[0] * (double)v[j][0] + (double)cx[1] * (double)v[j][1] + (double)cx[2] * (double)v[j][2] +
                           (double)cx[3] * (double)v[j][3];
        acc = acc + (double)cy[j] * row;
    }
    return (float)acc;
}

// numpy's float64 (image - mean) / std narrowed to float32
__host__ __device__ __forceinline__ float cubic_normalize(float v, double mean, double std) {
#pragma clang fp contract(off)
    return (float)(((double)v - mean) / std);
}

}  // namespace dr
