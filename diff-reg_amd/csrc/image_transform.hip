// image_transform.hip -- the input transform of Depth-Anything on the device (tenth set after ABI 0.7.0):
//   dr_image_cubic_chw_f32   [Hs, Ws, 3] float32 image -> bicubic resample to Hd x Wd -> (v - mean) / std -> [3, Hd, Wd] float32, one launch
// What it restates: Resize.__call__ with cv2.INTER_CUBIC, NormalizeImage.__call__ and PrepareForNet.__call__ of
// depth_anything/util/transform.py:168-178, 219-222, 232-234, reached through EXP/model.py:339-342.  The resample rule is csrc/cubic_index.h
// and nothing here restates it.
//
// One thread per destination pixel computes all three channels: a tap's three channels are 12 contiguous bytes and a row of four unclamped taps
// 48.  The x weights and tap offsets are computed once per thread and kept across the rows the thread walks.  Consecutive lanes take consecutive
// xd, so each of the three channel planes is stored coalesced.  The source (3.7 MB at 480 x 640) stays in L2: 48 independent loads per pixel and
// no LDS tile.  No workspace, no atomics, no scratch; two runs are bit-equal; nothing synchronises, so the call can be captured into a graph.
#include "common.h"
#include "cubic_index.h"
#include "../../include/diffreg_hip.h"

namespace dr {

struct ImageNormArgs {
    double mean[3], std[3];
};

constexpr int IMG_BX = 64, IMG_BY = 4;

__global__ __launch_bounds__(IMG_BX* IMG_BY) void image_cubic_chw_kernel(int Hs, int Ws, int ld_src, const float* __restrict__ src, int Hd, int Wd,
                                                                          double sh, double sw, int normalize, ImageNormArgs nm,
                                                                          float* __restrict__ out) {
    const int xd = blockIdx.x * IMG_BX + threadIdx.x;
    if (xd >= Wd) return;
    int xi[4];
    float cx[4];
    cubic_taps(sw, xd, Ws, xi, cx);
    const size_t plane = (size_t)Hd * Wd;
    for (int yd = blockIdx.y * IMG_BY + threadIdx.y; yd < Hd; yd += gridDim.y * IMG_BY) {
        int yi[4];
        float cy[4];
        cubic_taps(sh, yd, Hs, yi, cy);
        float v[3][4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* row = src + (size_t)yi[j] * ld_src;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* tap = row + 3 * (size_t)xi[i];
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c][j][i] = tap[c];
            }
        }
        float* o = out + (size_t)yd * Wd + xd;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float r = cubic_blend(cy, cx, v[c]);
            if (normalize) r = cubic_normalize(r, nm.mean[c], nm.std[c]);
            o[c * plane] = r;
        }
    }
}

}  // namespace dr

using namespace dr;

extern "C" {

int dr_image_cubic_chw_f32(int Hs, int Ws, int ld_src, const float* src_hwc, int Hd, int Wd, int normalize, const dr_image_norm* norm,
                           float* out_chw, void* stream) {
    if (Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1 || !src_hwc || !out_chw) return DR_EINVAL;
    if ((long long)ld_src < 3LL * Ws) return DR_EINVAL;
    ImageNormArgs nm = {{0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}};
    if (normalize) {
        if (!norm) return DR_EINVAL;
        for (int c = 0; c < 3; ++c) {
            if (norm->std[c] == 0.0) return DR_EINVAL;
            nm.mean[c] = norm->mean[c];
            nm.std[c] = norm->std[c];
        }
    }
    const unsigned gy = (unsigned)((Hd + IMG_BY - 1) / IMG_BY);
    const dim3 grid((unsigned)((Wd + IMG_BX - 1) / IMG_BX), gy < 65535u ? gy : 65535u), block(IMG_BX, IMG_BY);
    hipLaunchKernelGGL(image_cubic_chw_kernel, grid, block, 0, (hipStream_t)stream, Hs, Ws, ld_src, src_hwc, Hd, Wd, cubic_scale(Hs, Hd),
                       cubic_scale(Ws, Wd), normalize ? 1 : 0, nm, out_chw);
    DR_LAUNCH_CHECK();
    return DR_OK;
}

}  // extern "C"
