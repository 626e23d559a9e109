// conv_index_check.cpp -- host check of csrc/conv_index.h, the only place dr_conv2d_rows_f32 computes an address.  Build and run:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/conv_index_check.cpp \
//         -o /tmp/conv_index_check && /tmp/conv_index_check
//
// For every shape of the tests (tests/image_backbone2d3d_ref.CONV_CASES, every conv of the three fixture cases and of the real-width case) and of
// production (480 x 640, 128 base channels), with contiguous and padded leading dimensions, it walks what the kernels walk:
//   MFMA path (Cin % 4 == 0): every workgroup tile of both tile sizes, every staging slot (tile row, 4-wide group of every k-chunk, tails
//     included) of A and of the packed weight, every element of the epilogue;
//   direct path: every (output pixel of every wave's pixel group, tap, channel) and every (lane, weight position);
// and asserts (1) every offset returned lies, with the 4 floats a slot reads, inside its buffer; (2) every (output pixel, in-image tap, channel)
// of the convolution's definition is visited exactly once and nothing else is; (3) every output element is stored exactly once; (4) the output
// extents agree with the closed form of nn.Conv2d.  The x buffer is a real allocation of exactly Hi Wi ldx floats (AddressSanitizer guards its
// ends) and every visited offset is read.
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv_index.h"

using namespace dr;

static long long g_slots = 0;

#define CHECK(c)                                                                     \
    do {                                                                             \
        if (!(c)) {                                                                  \
            std::fprintf(stderr, "conv_index_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

static void check_shape(int k, int s, int p, int d, int Cin, int Cout, int Hi, int Wi, int pad_ld) {
    const ConvGeom g = conv_geom(Hi, Wi, Cin, Cout, k, s, p, d);
    const int ldx = Cin + pad_ld, ldo = Cout + pad_ld;
    // (4) closed form
    CHECK(g.Ho == (Hi + 2 * p - d * (k - 1) - 1) / s + 1 && g.Wo == (Wi + 2 * p - d * (k - 1) - 1) / s + 1 && g.Ho >= 1 && g.Wo >= 1);
    CHECK(g.K == k * k * Cin);
    const int M = g.Ho * g.Wo;
    std::vector<float> x((size_t)Hi * Wi * ldx, 1.0f), w((size_t)Cout * g.K, 1.0f);
    std::vector<unsigned char> seen((size_t)M * g.K, 0), expect((size_t)M * g.K, 0), wseen((size_t)Cout * g.K, 0), oseen((size_t)M * Cout, 0);
    // the definition: which (m, kk) are in-image
    for (int oy = 0; oy < g.Ho; ++oy)
        for (int ox = 0; ox < g.Wo; ++ox)
            for (int ky = 0; ky < k; ++ky)
                for (int kx = 0; kx < k; ++kx) {
                    const int iy = oy * s - p + ky * d, ix = ox * s - p + kx * d;
                    const bool in = iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
                    const int row = conv_tap_row(g, oy, ox, ky, kx);
                    CHECK(in ? row == iy * Wi + ix : row == -1);
                    for (int ci = 0; ci < Cin; ++ci) expect[(size_t)(oy * g.Wo + ox) * g.K + (ky * k + kx) * Cin + ci] = in;
                }
    volatile float sink = 0.f;
    const int tile_sizes[2] = {64, 128};
    const int ntile = (Cin % 4 == 0) ? 2 : 1;
    for (int ts = 0; ts < ntile; ++ts) {
        std::fill(seen.begin(), seen.end(), 0);
        std::fill(wseen.begin(), wseen.end(), 0);
        std::fill(oseen.begin(), oseen.end(), 0);
        if (Cin % 4 == 0) {
            const int B = tile_sizes[ts], tiles_m = (M + B - 1) / B, tiles_n = (Cout + B - 1) / B, nchunks = (g.K + 31) / 32;
            for (int tm = 0; tm < tiles_m; ++tm) {
                for (int ch = 0; ch < nchunks; ++ch)
                    for (int r = 0; r < B; ++r)
                        for (int q = 0; q < 8; ++q) {
                            const int m = tm * B + r, kk = ch * 32 + 4 * q;
                            const long long off = conv_a_offset(g, m, kk, ldx);
                            ++g_slots;
                            if (off < 0) continue;
                            CHECK(m < M && kk + 3 < g.K && off + 3 < (long long)x.size());
                            for (int e = 0; e < 4; ++e) {
                                sink = sink + x[(size_t)off + e];
                                CHECK(conv_a_offset(g, m, kk + e, ldx) == off + e);           // the 4-wide group lies inside one tap
                                CHECK(++seen[(size_t)m * g.K + kk + e] == 1);
                            }
                        }
            }
            for (int tn = 0; tn < tiles_n; ++tn)
                for (int ch = 0; ch < nchunks; ++ch)
                    for (int r = 0; r < B; ++r)
                        for (int q = 0; q < 8; ++q) {
                            const int co = tn * B + r, kk = ch * 32 + 4 * q;
                            const long long off = conv_w_offset(g, co, kk);
                            if (off < 0) continue;
                            CHECK(co < Cout && kk + 3 < g.K && off + 3 < (long long)w.size());
                            for (int e = 0; e < 4; ++e) {
                                sink = sink + w[(size_t)off + e];
                                CHECK(++wseen[(size_t)off + e] == 1);
                            }
                        }
            for (int tm = 0; tm < tiles_m; ++tm)
                for (int tn = 0; tn < tiles_n; ++tn)
                    for (int r = 0; r < B; ++r)
                        for (int c = 0; c < B; ++c) {
                            const long long off = conv_o_offset(g, tm * B + r, tn * B + c, ldo);
                            if (off < 0) continue;
                            CHECK(off < (long long)M * ldo && off % ldo < Cout);
                            CHECK(++oseen[(size_t)(off / ldo) * Cout + off % ldo] == 1);
                        }
        } else {
            const int DPX = 8, groups = (M + 4 * DPX - 1) / (4 * DPX), cblocks = (Cout + 63) / 64;
            for (int bx = 0; bx < groups; ++bx)
                for (int wv = 0; wv < 4; ++wv)
                    for (int j = 0; j < DPX; ++j) {
                        const int m = (bx * 4 + wv) * DPX + j;
                        for (int tap = 0; tap < k * k; ++tap) {
                            const long long off = conv_a_offset(g, m, tap * Cin, ldx);
                            ++g_slots;
                            if (off < 0) continue;
                            CHECK(m < M && off + Cin - 1 < (long long)x.size());
                            for (int ci = 0; ci < Cin; ++ci) {
                                sink = sink + x[(size_t)off + ci];
                                CHECK(conv_a_offset(g, m, tap * Cin + ci, ldx) == off + ci);
                                CHECK(++seen[(size_t)m * g.K + tap * Cin + ci] == 1);
                            }
                        }
                        for (int by = 0; by < cblocks; ++by)
                            for (int lane = 0; lane < 64; ++lane) {
                                const long long off = conv_o_offset(g, m, by * 64 + lane, ldo);
                                if (off < 0) continue;
                                CHECK(off < (long long)M * ldo && off % ldo < Cout);
                                CHECK(++oseen[(size_t)(off / ldo) * Cout + off % ldo] == 1);
                            }
                    }
            for (int by = 0; by < cblocks; ++by)
                for (int lane = 0; lane < 64; ++lane)
                    for (int kk = 0; kk < g.K; ++kk) {
                        const long long off = conv_w_offset(g, by * 64 + lane, kk);
                        if (off < 0) continue;
                        CHECK(off < (long long)w.size());
                        sink = sink + w[(size_t)off];
                        CHECK(++wseen[(size_t)off] == 1);
                    }
        }
        // (2), (3): exactly the definition's set, each once
        for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == expect[i]);
        for (size_t i = 0; i < wseen.size(); ++i) CHECK(wseen[i] == 1);
        for (size_t i = 0; i < oseen.size(); ++i) CHECK(oseen[i] == 1);
    }
    (void)sink;
}

// every conv of ImageBackbone(1, out, base) on an H x W image (EXP/image_backbone.py:81-252)
static void check_backbone(int H, int W, int base, int out, int pad_ld) {
    const int b = base;
    const int H1 = conv_out_size(H, 7, 2, 3, 1), W1 = conv_out_size(W, 7, 2, 3, 1);
    const int H2 = conv_out_size(H1, 3, 2, 1, 1), W2 = conv_out_size(W1, 3, 2, 1, 1);
    const int H3 = conv_out_size(H2, 3, 2, 1, 1), W3 = conv_out_size(W2, 3, 2, 1, 1);
    check_shape(7, 2, 3, 1, 1, b, H, W, pad_ld);                 // encoder1
    check_shape(3, 1, 1, 1, b, b, H1, W1, pad_ld);               // encoder2, decoder1 at half size
    check_shape(3, 2, 1, 1, b, 2 * b, H1, W1, pad_ld);           // encoder3.0 conv1 / identity
    check_shape(3, 1, 1, 1, 2 * b, 2 * b, H2, W2, pad_ld);       // encoder3, decoder2_2.0
    check_shape(3, 2, 1, 1, 2 * b, 4 * b, H2, W2, pad_ld);       // encoder4.0 conv1 / identity
    check_shape(3, 1, 1, 1, 4 * b, 4 * b, H3, W3, pad_ld);       // encoder4, decoder3_2.0
    check_shape(1, 1, 0, 1, 4 * b, 4 * b, H3, W3, pad_ld);       // decoder4_1
    check_shape(1, 1, 0, 1, 2 * b, 4 * b, H2, W2, pad_ld);       // decoder3_1
    check_shape(3, 1, 1, 1, 4 * b, 2 * b, H2, W2, pad_ld);       // decoder3_2.1
    check_shape(1, 1, 0, 1, b, 2 * b, H1, W1, pad_ld);           // decoder2_1
    check_shape(3, 1, 1, 1, 2 * b, b, H1, W1, pad_ld);           // decoder2_2.1
    check_shape(1, 1, 0, 1, b, b, H1, W1, pad_ld);               // decoder1_1
    check_shape(3, 1, 1, 1, b, b, H, W, pad_ld);                 // decoder1_2
    check_shape(1, 1, 0, 1, b, out, H, W, pad_ld);               // out_proj
}

int main() {
    // tests/image_backbone2d3d_ref.CONV_CASES: (k, s, p, d, Cin, Cout, H, W)
    const int cases[][8] = {{3, 1, 1, 1, 16, 16, 5, 7},   {3, 2, 1, 1, 16, 32, 21, 27}, {7, 2, 3, 1, 1, 16, 21, 27},   {7, 2, 3, 1, 3, 16, 21, 27},
                            {1, 1, 0, 1, 64, 64, 3, 4},   {3, 1, 2, 2, 16, 16, 9, 9},   {3, 1, 1, 1, 20, 160, 13, 11}, {3, 1, 1, 1, 16, 16, 1, 1},
                            {3, 1, 1, 1, 128, 16, 240, 280}};
    for (const auto& c : cases)
        for (int pad_ld = 0; pad_ld <= 8; pad_ld += 4) check_shape(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], pad_ld);
    check_shape(3, 1, 1, 1, 16, 16, 5, 7, 3);                    // an odd leading dimension (the scalar-load arm)
    check_backbone(24, 32, 16, 16, 0);                           // fixture cases a, b, c
    check_backbone(21, 27, 16, 16, 0);
    check_backbone(24, 32, 16, 24, 0);
    check_backbone(48, 64, 128, 128, 0);                         // the real-width test
    check_backbone(480, 640, 128, 128, 0);                       // production
    // closed form of the output extent over a grid of small geometries, degenerate ones included
    for (int in = 1; in <= 40; ++in)
        for (int k = 1; k <= 7; ++k)
            for (int s = 1; s <= 3; ++s)
                for (int p = 0; p <= 3; ++p)
                    for (int d = 1; d <= 3; ++d) {
                        int n = 0;                               // count the output positions whose dilated kernel fits the padded extent
                        for (int o = 0; o * s - p + d * (k - 1) <= in - 1 + p; ++o) ++n;
                        CHECK(conv_out_size(in, k, s, p, d) == n);
                    }
    std::printf("conv_index_check ok: %lld staging slots walked\n", g_slots);
    return 0;
}
