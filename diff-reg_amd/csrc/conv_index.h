// conv_index.h -- the index arithmetic of dr_conv2d_rows_f32 and of its two gradients (conv2d.hip): nn.Conv2d (groups = 1, zero padding, square kernel k, stride s,
// padding p, dilation d) on token rows [H W, C].  The kernels compute every address through these functions and nothing else, and
// tools/conv_index_check.cpp walks the same functions on the host over every (output pixel, tap, 4-channel group) of the tested and the
// production shapes before anything runs on a device (tools/conv_bwd_index_check.cpp for the gradients; tools/dpt_index_check.cpp for the transposed
// convolution and the project entry at the end of the file).  No HIP type in here: the file compiles as plain C++.
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

// ---- the backward (dr_conv2d_rows_backward_data_f32, dr_conv2d_rows_backward_weight_f32); walked by tools/conv_bwd_index_check.cpp ----------

// (input pixel (iy, ix), tap (ky, kx)) -> the output row oy Wo + ox whose tap (ky, kx) reads that pixel, or -1 when there is none: iy = oy s - p +
// ky d has a solution only if iy + p - ky d is >= 0, divisible by s, and its quotient lies inside Ho (the same for x)
DR_HD int conv_bwd_tap_row(const ConvGeom& g, int iy, int ix, int ky, int kx) {
    const int ty = iy + g.p - ky * g.d, tx = ix + g.p - kx * g.d;
    if (ty < 0 || tx < 0 || ty % g.s != 0 || tx % g.s != 0) return -1;
    const int oy = ty / g.s, ox = tx / g.s;
    return (oy < g.Ho && ox < g.Wo) ? oy * g.Wo + ox : -1;
}

// the length of one row of the data gradient's packed weight [Cin, k k Cout] (tap-major, co-minor)
DR_HD int conv_bwd_k(const ConvGeom& g) { return g.k * g.k * g.Cout; }

// The A operand of the data gradient: element (input pixel m, position kk = (tap, co)) -> offset into grad_out [Ho Wo, ldg], or -1 for "zero, load
// nothing".  With Cout % 4 == 0 a 4-wide group lies inside one tap.
DR_HD long long conv_bwd_a_offset(const ConvGeom& g, int m, int kk, int ldg) {
    if (m < 0 || m >= g.Hi * g.Wi || kk < 0 || kk >= conv_bwd_k(g)) return -1;
    const int iy = m / g.Wi, ix = m - iy * g.Wi;
    const int tap = kk / g.Cout, co = kk - tap * g.Cout;
    const int ky = tap / g.k, kx = tap - ky * g.k;
    const int row = conv_bwd_tap_row(g, iy, ix, ky, kx);
    return row < 0 ? -1 : (long long)row * ldg + co;
}

// The B operand of the data gradient: element (input channel ci, position kk) of the packed [Cin, k k Cout], or -1 outside it
DR_HD long long conv_bwd_w_offset(const ConvGeom& g, int ci, int kk) {
    if (ci < 0 || ci >= g.Cin || kk < 0 || kk >= conv_bwd_k(g)) return -1;
    return (long long)ci * conv_bwd_k(g) + kk;
}

// The data gradient (and its addend): element (input pixel m, channel ci) of a [Hi Wi, ld] buffer, or -1 outside it
DR_HD long long conv_bwd_o_offset(const ConvGeom& g, int m, int ci, int ld) {
    if (m < 0 || m >= g.Hi * g.Wi || ci < 0 || ci >= g.Cin) return -1;
    return (long long)m * ld + ci;
}

// The weight gradient reduces over the M = Ho Wo output pixels in S slabs of L pixels (the last one ragged).  S and L are functions of M alone --
// never of the device -- so a problem sums in the same order everywhere: S0 = min(64, ceil(M / 2048)), L = ceil(M / S0) rounded up to the
// 32-pixel chunk of the kernel, S = ceil(M / L) (no slab is empty).
constexpr int CV_WG_CHUNK = 32, CV_WG_SLAB = 2048, CV_WG_MAX_SLABS = 64;
struct ConvSlabs {
    int S, L;
};
DR_HD ConvSlabs conv_wgrad_slabs(int M) {
    int s0 = (M + CV_WG_SLAB - 1) / CV_WG_SLAB;
    if (s0 > CV_WG_MAX_SLABS) s0 = CV_WG_MAX_SLABS;
    if (s0 < 1) s0 = 1;
    ConvSlabs r;
    r.L = ((M + s0 - 1) / s0 + CV_WG_CHUNK - 1) / CV_WG_CHUNK * CV_WG_CHUNK;
    if (r.L < CV_WG_CHUNK) r.L = CV_WG_CHUNK;
    r.S = (M + r.L - 1) / r.L;
    if (r.S < 1) r.S = 1;
    return r;
}

// output pixel j of slab s -> the pixel m, or -1 beyond the slab or the image (a ragged chunk)
DR_HD int conv_slab_pixel(const ConvGeom& g, const ConvSlabs& sl, int s, int j) {
    if (s < 0 || s >= sl.S || j < 0 || j >= sl.L) return -1;
    const long long m = (long long)s * sl.L + j;
    return m < (long long)g.Ho * g.Wo ? (int)m : -1;
}

// element (slab s, output channel co, position kk) of the float32 partial sums [S, Cout, K], or -1 outside them
DR_HD long long conv_wg_part_offset(const ConvGeom& g, const ConvSlabs& sl, int s, int co, int kk) {
    if (s < 0 || s >= sl.S || co < 0 || co >= g.Cout || kk < 0 || kk >= g.K) return -1;
    return ((long long)s * g.Cout + co) * g.K + kk;
}

// the workspace of the weight gradient: the float32 partials [S, Cout, K] (rounded up to 8 bytes), then the double partials [S, Cout] of grad_bias
DR_HD long long conv_wg_bias_part_byte(const ConvGeom& g, const ConvSlabs& sl) {
    return ((long long)sl.S * g.Cout * g.K * 4 + 7) / 8 * 8;
}
DR_HD long long conv_wg_workspace_bytes(const ConvGeom& g, const ConvSlabs& sl) {
    return conv_wg_bias_part_byte(g, sl) + (long long)sl.S * g.Cout * 8;
}

// ---- the DPT head's two other forms (dr_conv_transpose2d_rows_f32, dr_conv2d_rows_project_f32); walked by tools/dpt_index_check.cpp ----------

// nn.ConvTranspose2d(Cin, Cout, k = s, stride = s, padding 0): no two taps meet, so out[(y s + i)(W s) + x s + j][co] = sum_ci x[y W + x][ci]
// W[ci][co][i][j] is a plain GEMM with m = input pixel, n = (i, j, co) (tap-major, co-minor), kk = ci.  The geometry reuses ConvGeom: k = s,
// Ho = Hi s, Wo = Wi s, K = Cin (the length of one row of the packed weight [s s Cout, Cin]).
DR_HD ConvGeom conv_t_geom(int Hi, int Wi, int Cin, int Cout, int s) {
    ConvGeom g;
    g.Hi = Hi; g.Wi = Wi; g.Cin = Cin; g.Cout = Cout;
    g.k = s; g.s = s; g.p = 0; g.d = 1;
    g.Ho = Hi * s;
    g.Wo = Wi * s;
    g.K = Cin;
    return g;
}

// the number of GEMM columns n = (i, j, co)
DR_HD int conv_t_cols(const ConvGeom& g) { return g.k * g.k * g.Cout; }

// The A operand: element (input pixel m, channel kk) of x [Hi Wi, ldx], or -1 outside the problem
DR_HD long long conv_t_a_offset(const ConvGeom& g, int m, int kk, int ldx) {
    if (m < 0 || m >= g.Hi * g.Wi || kk < 0 || kk >= g.Cin) return -1;
    return (long long)m * ldx + kk;
}

// The B operand: element (column n, channel kk) of the packed weight [s s Cout, Cin], or -1 outside it
DR_HD long long conv_t_w_offset(const ConvGeom& g, int n, int kk) {
    if (n < 0 || n >= conv_t_cols(g) || kk < 0 || kk >= g.Cin) return -1;
    return (long long)n * g.Cin + kk;
}

// column n -> its output channel (the bias index); n inside [0, conv_t_cols)
DR_HD int conv_t_channel(const ConvGeom& g, int n) { return n % g.Cout; }

// The store, a pixel shuffle: (input pixel m = y Wi + x, column n = ((i s + j) Cout + co)) -> element (row (y s + i)(Wi s) + x s + j, co) of
// out [Hi s Wi s, ld], or -1 outside the problem
DR_HD long long conv_t_o_offset(const ConvGeom& g, int m, int n, int ld) {
    if (m < 0 || m >= g.Hi * g.Wi || n < 0 || n >= conv_t_cols(g)) return -1;
    const int y = m / g.Wi, x = m - y * g.Wi;
    const int tap = n / g.Cout, co = n - tap * g.Cout;
    const int i = tap / g.s, j = tap - i * g.s;
    return ((long long)(y * g.s + i) * g.Wo + x * g.s + j) * ld + co;
}

// The C/D layout of the 32 x 32 MFMA: register r of lane half h of 32-row tile `tile` holds row tile 32 + (r & 3) + 8 (r >> 2) + 4 h of the
// workgroup's rows (the column is lane & 31).  The project entry's epilogue keeps one sum per such row.
DR_HD int conv_tile_row(int tile, int r, int h) { return tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h; }

// The project entry's result: output pixel m of out [Ho Wo] with the leading dimension ld (one value per pixel), or -1 outside it
DR_HD long long conv_p_o_offset(const ConvGeom& g, int m, int ld) {
    if (m < 0 || m >= g.Ho * g.Wo) return -1;
    return (long long)m * ld;
}

}  // namespace dr
