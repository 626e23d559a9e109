// conv_index.h -- the index arithmetic of dr_conv2d_rows_f32 (conv2d.hip): nn.Conv2d (groups = 1, zero padding, square kernel k, stride s,
// padding p, dilation d) on token rows [H W, C].  The kernels compute every address through these functions and nothing else, and
// tools/conv_index_check.cpp walks the same functions on the host over every (output pixel, tap, 4-channel group) of the tested and the
// production shapes before anything runs on a device.  No HIP type in here: the file compiles as plain C++.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DR_HD __host__ __device__ inline
#else
#define DR_HD inline
#endif

namespace dr {

struct ConvGeom {
    int Hi, Wi, Cin, Cout;      // input image and channel counts
    int k, s, p, d;             // square kernel, stride, zero padding, dilation
    int Ho, Wo;                 // conv_out_size of Hi, Wi
    int K;                      // k k Cin: the length of one packed weight row [tap][ci]
};

// nn.Conv2d's output extent: floor((in + 2p - d(k - 1) - 1) / s) + 1; <= 0 when the dilated kernel does not fit the padded image
DR_HD int conv_out_size(int in, int k, int s, int p, int d) {
    const int span = in + 2 * p - d * (k - 1) - 1;
    return span < 0 ? 0 : span / s + 1;
}

DR_HD ConvGeom conv_geom(int Hi, int Wi, int Cin, int Cout, int k, int s, int p, int d) {
    ConvGeom g;
    g.Hi = Hi; g.Wi = Wi; g.Cin = Cin; g.Cout = Cout;
    g.k = k; g.s = s; g.p = p; g.d = d;
    g.Ho = conv_out_size(Hi, k, s, p, d);
    g.Wo = conv_out_size(Wi, k, s, p, d);
    g.K = k * k * Cin;
    return g;
}

// (output pixel (oy, ox), tap (ky, kx)) -> the input row iy Wi + ix, or -1 when the tap lies in the zero padding
DR_HD int conv_tap_row(const ConvGeom& g, int oy, int ox, int ky, int kx) {
    const int iy = oy * g.s - g.p + ky * g.d, ix = ox * g.s - g.p + kx * g.d;
    return (iy >= 0 && iy < g.Hi && ix >= 0 && ix < g.Wi) ? iy * g.Wi + ix : -1;
}

// position kk of a packed weight row (tap-major, ci-minor) -> tap and channel
DR_HD void conv_split_k(const ConvGeom& g, int kk, int& ky, int& kx, int& ci) {
    const int tap = kk / g.Cin;
    ci = kk - tap * g.Cin;
    ky = tap / g.k;
    kx = tap - ky * g.k;
}

// The A operand of the implicit GEMM: element (output pixel m, position kk) -> offset into x [Hi Wi, ldx], or -1 for "contributes zero, load nothing"
// (m or kk outside the problem: a ragged tile or the tail of the last k-chunk; or a tap in the padding).  A 4-channel group starts at kk % 4 == 0
// and, with Cin % 4 == 0, lies inside one tap: offsets .. + 3 are then in range whenever the first one is.
DR_HD long long conv_a_offset(const ConvGeom& g, int m, int kk, int ldx) {
    if (m < 0 || m >= g.Ho * g.Wo || kk < 0 || kk >= g.K) return -1;
    const int oy = m / g.Wo, ox = m - oy * g.Wo;
    int ky, kx, ci;
    conv_split_k(g, kk, ky, kx, ci);
    const int row = conv_tap_row(g, oy, ox, ky, kx);
    return row < 0 ? -1 : (long long)row * ldx + ci;
}

// The B operand: element (output channel co, position kk) of the packed weight [Cout, K], or -1 outside it
DR_HD long long conv_w_offset(const ConvGeom& g, int co, int kk) {
    if (co < 0 || co >= g.Cout || kk < 0 || kk >= g.K) return -1;
    return (long long)co * g.K + kk;
}

// The result (and the addend): element (output pixel m, channel co) of a [Ho Wo, ld] buffer, or -1 outside it
DR_HD long long conv_o_offset(const ConvGeom& g, int m, int co, int ld) {
    if (m < 0 || m >= g.Ho * g.Wo || co < 0 || co >= g.Cout) return -1;
    return (long long)m * ld + co;
}

}  // namespace dr
