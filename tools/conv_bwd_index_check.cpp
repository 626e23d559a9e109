// conv_bwd_index_check.cpp -- host check of the index arithmetic of the image backbone's backward (csrc/conv_index.h, csrc/resize_index.h): the
// only places dr_conv2d_rows_backward_data_f32, dr_conv2d_rows_backward_weight_f32 and dr_resize_rows_backward_f32 compute an address.  Build
// and run; host code only, never loaded into Python and never run on a device:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/conv_bwd_index_check.cpp \
//         -o /tmp/conv_bwd_index_check && /tmp/conv_bwd_index_check
//
// For every shape of the tests (tests/image_backbone2d3d_ref.CONV_CASES, the extra cases of tests/test_image_backbone2d3d_bwd_gpu.py, every conv
// of the fixture cases and of the real-width case) and of production (480 x 640, 128 base channels), with contiguous and padded leading
// dimensions, it walks what the kernels walk:
//   data gradient, MFMA arm (Cout % 4 == 0): every workgroup tile of both tile sizes, every staging slot of grad_out and of the packed
//     [Cin, k k Cout] weight (k-chunk tails included), every element of the epilogue; direct arm: every (input pixel, channel) thread;
//   weight gradient: every slab (the ragged last one included), every chunk, every staging slot of x and of grad_out of every tile, every
//     element of the partial sums and of the second pass; direct arm: every (output channel, position) thread of every slab;
//   resample backward: every (source texel) gather.
// and asserts (1) every offset, with the 4 floats a slot reads, lies inside a real allocation of exactly the buffer's size (AddressSanitizer
// guards its ends; every visited offset is read); (2) every (input pixel, tap, channel) triple the forward visits is visited exactly once by the
// data gradient's map and nothing else is, and the weight gradient visits exactly the forward's (output pixel, position) set, each once;
// (3) every output element -- grad_x, partial sum, grad_w, grad_bias partial -- is stored exactly once; (4) every output pixel lies in exactly
// one slab, and the workspace size covers both partial arrays; (5) the weights of the resample gather sum to one per destination pixel.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv_index.h"
#include "resize_index.h"

using namespace dr;

static long long g_slots = 0;

#define CHECK(c)                                                                         \
    do {                                                                                 \
        if (!(c)) {                                                                      \
            std::fprintf(stderr, "conv_bwd_index_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

static volatile float sink = 0.f;

// the forward's set: cnt[(input row, tap)] = how many output pixels read input row through tap (0 or 1), and the output row that does
static void forward_set(const ConvGeom& g, std::vector<int>& owner) {
    owner.assign((size_t)g.Hi * g.Wi * g.k * g.k, -1);
    for (int oy = 0; oy < g.Ho; ++oy)
        for (int ox = 0; ox < g.Wo; ++ox)
            for (int ky = 0; ky < g.k; ++ky)
                for (int kx = 0; kx < g.k; ++kx) {
                    const int row = conv_tap_row(g, oy, ox, ky, kx);
                    if (row < 0) continue;
                    int& o = owner[(size_t)row * g.k * g.k + ky * g.k + kx];
                    CHECK(o == -1);                                                  // one output pixel per (input pixel, tap)
                    o = oy * g.Wo + ox;
                }
}

static void check_dgrad(const ConvGeom& g, int pad_ld) {
    const int Mi = g.Hi * g.Wi, Mo = g.Ho * g.Wo, KB = conv_bwd_k(g), taps = g.k * g.k;
    const int ldg = g.Cout + pad_ld, ldo = g.Cin + pad_ld;
    CHECK(KB == taps * g.Cout);
    std::vector<int> owner;
    forward_set(g, owner);
    for (int m = 0; m < Mi; ++m)                                                     // the slot map is the forward's map turned round
        for (int tap = 0; tap < taps; ++tap) CHECK(conv_bwd_tap_row(g, m / g.Wi, m % g.Wi, tap / g.k, tap % g.k) == owner[(size_t)m * taps + tap]);
    std::vector<float> go((size_t)Mo * ldg, 1.0f), wt((size_t)g.Cin * KB, 1.0f);
    std::vector<int> cnt((size_t)Mi * taps);
    std::vector<unsigned char> wseen((size_t)g.Cin * KB), oseen((size_t)Mi * g.Cin);
    auto verify = [&]() {
        for (size_t i = 0; i < cnt.size(); ++i) CHECK(cnt[i] == (owner[i] >= 0 ? g.Cout : 0));
        for (size_t i = 0; i < wseen.size(); ++i) CHECK(wseen[i] == 1);
        for (size_t i = 0; i < oseen.size(); ++i) CHECK(oseen[i] == 1);
    };
    if (g.Cout % 4 == 0) {
        const int tile_sizes[2] = {64, 128};
        for (int ts = 0; ts < 2; ++ts) {
            std::fill(cnt.begin(), cnt.end(), 0);
            std::fill(wseen.begin(), wseen.end(), 0);
            std::fill(oseen.begin(), oseen.end(), 0);
            const int B = tile_sizes[ts], tiles_m = (Mi + B - 1) / B, tiles_n = (g.Cin + B - 1) / B, nchunks = (KB + 31) / 32;
            for (int tm = 0; tm < tiles_m; ++tm)
                for (int ch = 0; ch < nchunks; ++ch)
                    for (int r = 0; r < B; ++r)
                        for (int q = 0; q < 8; ++q) {
                            const int m = tm * B + r, kk = ch * 32 + 4 * q;
                            const long long off = conv_bwd_a_offset(g, m, kk, ldg);
                            ++g_slots;
                            if (off < 0) continue;
                            CHECK(m < Mi && kk + 3 < KB && off + 3 < (long long)go.size());
                            for (int e = 0; e < 4; ++e) {
                                sink = sink + go[(size_t)off + e];
                                CHECK(conv_bwd_a_offset(g, m, kk + e, ldg) == off + e);      // the 4-wide group lies inside one tap
                                CHECK((off + e) % ldg < g.Cout);
                            }
                            CHECK(off / ldg == owner[(size_t)m * taps + kk / g.Cout]);
                            cnt[(size_t)m * taps + kk / g.Cout] += 4;
                        }
            for (int tn = 0; tn < tiles_n; ++tn)
                for (int ch = 0; ch < nchunks; ++ch)
                    for (int r = 0; r < B; ++r)
                        for (int q = 0; q < 8; ++q) {
                            const long long off = conv_bwd_w_offset(g, tn * B + r, ch * 32 + 4 * q);
                            if (off < 0) continue;
                            CHECK(off + 3 < (long long)wt.size());
                            for (int e = 0; e < 4; ++e) {
                                sink = sink + wt[(size_t)off + e];
                                CHECK(++wseen[(size_t)off + e] == 1);
                            }
                        }
            for (int tm = 0; tm < tiles_m; ++tm)
                for (int tn = 0; tn < tiles_n; ++tn)
                    for (int r = 0; r < B; ++r)
                        for (int c = 0; c < B; ++c) {
                            const long long off = conv_bwd_o_offset(g, tm * B + r, tn * B + c, ldo);
                            if (off < 0) continue;
                            CHECK(off < (long long)Mi * ldo && off % ldo < g.Cin);
                            CHECK(++oseen[(size_t)(off / ldo) * g.Cin + off % ldo] == 1);
                        }
            verify();
        }
    } else {
        std::fill(cnt.begin(), cnt.end(), 0);
        std::fill(wseen.begin(), wseen.end(), 0);
        std::fill(oseen.begin(), oseen.end(), 0);
        const long long n = (long long)Mi * g.Cin, blocks = (n + 255) / 256;
        for (long long e = 0; e < blocks * 256; ++e) {
            const int m = (int)(e / g.Cin), ci = (int)(e - (long long)m * g.Cin);
            const long long oo = conv_bwd_o_offset(g, m, ci, ldo);
            if (oo < 0) continue;
            CHECK(oo < (long long)Mi * ldo && oo % ldo < g.Cin);
            CHECK(++oseen[(size_t)(oo / ldo) * g.Cin + oo % ldo] == 1);
            for (int tap = 0; tap < taps; ++tap) {
                const long long ao = conv_bwd_a_offset(g, m, tap * g.Cout, ldg);
                ++g_slots;
                for (int co = 0; co < g.Cout; ++co) {
                    const long long wo = conv_bwd_w_offset(g, ci, tap * g.Cout + co);
                    CHECK(wo >= 0 && wo < (long long)wt.size());
                    if (ao >= 0) sink = sink + wt[(size_t)wo];
                    if (m == 0) CHECK(++wseen[(size_t)wo] == 1);
                }
                if (ao < 0) continue;
                CHECK(ao + g.Cout - 1 < (long long)go.size() && ao / ldg == owner[(size_t)m * taps + tap]);
                for (int co = 0; co < g.Cout; ++co) sink = sink + go[(size_t)ao + co];
                if (ci == 0) cnt[(size_t)m * taps + tap] += g.Cout;
            }
        }
        verify();
    }
}

static void check_wgrad(const ConvGeom& g, int pad_ld) {
    const int Mo = g.Ho * g.Wo, taps = g.k * g.k, K = g.K;
    const int ldx = g.Cin + pad_ld, ldg = g.Cout + pad_ld;
    const ConvSlabs sl = conv_wgrad_slabs(Mo);
    // (4) the slab rule: a function of Mo alone, chunk-aligned, no empty slab, every pixel in exactly one slab
    CHECK(sl.S >= 1 && sl.S <= CV_WG_MAX_SLABS && sl.L % CV_WG_CHUNK == 0 && (long long)sl.S * sl.L >= Mo && (long long)(sl.S - 1) * sl.L < Mo);
    {
        std::vector<unsigned char> pix(Mo, 0);
        for (int s = -1; s <= sl.S; ++s)
            for (int j = -1; j <= sl.L; ++j) {
                const int m = conv_slab_pixel(g, sl, s, j);
                if (m < 0) continue;
                CHECK(s >= 0 && s < sl.S && j >= 0 && j < sl.L && m < Mo);
                CHECK(++pix[m] == 1);
            }
        for (int m = 0; m < Mo; ++m) CHECK(pix[m] == 1);
    }
    const long long ws_bytes = conv_wg_workspace_bytes(g, sl), bias_at = conv_wg_bias_part_byte(g, sl);
    CHECK(bias_at % 8 == 0 && bias_at >= (long long)sl.S * g.Cout * K * 4 && ws_bytes == bias_at + (long long)sl.S * g.Cout * 8);
    std::vector<float> x((size_t)g.Hi * g.Wi * ldx, 1.0f), go((size_t)Mo * ldg, 1.0f);
    std::vector<unsigned char> aseen((size_t)Mo * K, 0), gseen((size_t)Mo * g.Cout, 0), pseen((size_t)sl.S * g.Cout * K, 0);
    if (g.Cin % 4 == 0) {
        const int BT = 64, Q = BT / 4, tiles_k = (K + BT - 1) / BT, tiles_c = (g.Cout + BT - 1) / BT, nchunks = sl.L / CV_WG_CHUNK;
        for (int slab = 0; slab < sl.S; ++slab) {
            for (int ch = 0; ch < nchunks; ++ch)
                for (int r = 0; r < CV_WG_CHUNK; ++r) {
                    const int m = conv_slab_pixel(g, sl, slab, ch * CV_WG_CHUNK + r);
                    for (int tk = 0; tk < tiles_k; ++tk)
                        for (int q = 0; q < Q; ++q) {
                            const int kk = tk * BT + 4 * q;
                            const long long ao = m < 0 ? -1 : conv_a_offset(g, m, kk, ldx);
                            ++g_slots;
                            if (ao < 0) continue;
                            CHECK(kk + 3 < K && ao + 3 < (long long)x.size());
                            for (int e = 0; e < 4; ++e) {
                                sink = sink + x[(size_t)ao + e];
                                CHECK(conv_a_offset(g, m, kk + e, ldx) == ao + e);
                                CHECK(++aseen[(size_t)m * K + kk + e] == 1);
                            }
                        }
                    for (int tc = 0; tc < tiles_c; ++tc)
                        for (int q = 0; q < Q; ++q)
                            for (int e = 0; e < 4; ++e) {                             // the scalar arm's four guarded loads; the vector arm (Cout % 4 == 0) reads
                                const int co = tc * BT + 4 * q + e;                   // the same four from the first one's offset
                                const long long o = m < 0 ? -1 : conv_o_offset(g, m, co, ldg);
                                if (o < 0) continue;
                                CHECK(o < (long long)go.size() && o % ldg < g.Cout);
                                if (g.Cout % 4 == 0) CHECK(o == conv_o_offset(g, m, co - e, ldg) + e);
                                sink = sink + go[(size_t)o];
                                CHECK(++gseen[(size_t)m * g.Cout + co] == 1);
                            }
                }
            for (int tc = 0; tc < tiles_c; ++tc)
                for (int tk = 0; tk < tiles_k; ++tk)
                    for (int r = 0; r < BT; ++r)
                        for (int c = 0; c < BT; ++c) {
                            const long long o = conv_wg_part_offset(g, sl, slab, tc * BT + r, tk * BT + c);
                            if (o < 0) continue;
                            CHECK(o * 4 + 4 <= bias_at);
                            CHECK(++pseen[(size_t)o] == 1);
                        }
        }
    } else {
        const long long n = (long long)g.Cout * K, blocks = (n + 255) / 256;
        for (int slab = 0; slab < sl.S; ++slab) {
            for (long long e = 0; e < blocks * 256; ++e) {
                const int co = (int)(e / K), kk = (int)(e - (long long)co * K);
                const long long po = conv_wg_part_offset(g, sl, slab, co, kk);
                if (po < 0) continue;
                CHECK(po * 4 + 4 <= bias_at);
                CHECK(++pseen[(size_t)po] == 1);
                if (co > 0 && kk > 0) continue;                                      // x offsets do not depend on co, grad_out offsets not on kk
                for (int j = 0; j < sl.L; ++j) {
                    const int m = conv_slab_pixel(g, sl, slab, j);
                    if (m < 0) break;
                    ++g_slots;
                    if (kk == 0) {
                        const long long o = conv_o_offset(g, m, co, ldg);
                        CHECK(o >= 0 && o < (long long)go.size());
                        sink = sink + go[(size_t)o];
                        CHECK(++gseen[(size_t)m * g.Cout + co] == 1);
                    }
                    if (co == 0) {
                        const long long ao = conv_a_offset(g, m, kk, ldx);
                        if (ao < 0) continue;
                        CHECK(ao < (long long)x.size());
                        sink = sink + x[(size_t)ao];
                        CHECK(++aseen[(size_t)m * K + kk] == 1);
                    }
                }
            }
        }
    }
    // (2) exactly the forward's (output pixel, position) set
    for (int m = 0; m < Mo; ++m)
        for (int tap = 0; tap < taps; ++tap) {
            const bool in = conv_tap_row(g, m / g.Wo, m % g.Wo, tap / g.k, tap % g.k) >= 0;
            for (int ci = 0; ci < g.Cin; ++ci) CHECK(aseen[(size_t)m * K + tap * g.Cin + ci] == (in ? 1 : 0));
        }
    for (size_t i = 0; i < gseen.size(); ++i) CHECK(gseen[i] == 1);
    for (size_t i = 0; i < pseen.size(); ++i) CHECK(pseen[i] == 1);
    // the bias partials: (slab, 64-channel block, lane), pixels j = wave, wave + 4, ...; and the second pass
    std::vector<unsigned char> bseen((size_t)Mo * g.Cout, 0);
    for (int slab = 0; slab < sl.S; ++slab)
        for (int bx = 0; bx < (g.Cout + 63) / 64; ++bx)
            for (int lane = 0; lane < 64; ++lane)
                for (int wv = 0; wv < 4; ++wv)
                    for (int j = wv; j < sl.L; j += 4) {
                        const int m = conv_slab_pixel(g, sl, slab, j), co = bx * 64 + lane;
                        const long long o = m < 0 ? -1 : conv_o_offset(g, m, co, ldg);
                        if (o < 0) continue;
                        CHECK(o < (long long)go.size());
                        CHECK(++bseen[(size_t)m * g.Cout + co] == 1);
                        CHECK(bias_at + ((long long)slab * g.Cout + co) * 8 + 8 <= ws_bytes);
                    }
    for (size_t i = 0; i < bseen.size(); ++i) CHECK(bseen[i] == 1);
    std::vector<unsigned char> wseen((size_t)g.Cout * K, 0);
    const long long n2 = (long long)g.Cout * K + g.Cout;
    for (long long e = 0; e < (n2 + 255) / 256 * 256; ++e)
        if (e < (long long)g.Cout * K) {
            const int co = (int)(e / K), kk = (int)(e - (long long)co * K);
            for (int s = 0; s < sl.S; ++s) CHECK(conv_wg_part_offset(g, sl, s, co, kk) >= 0);
            const long long o = conv_w_offset(g, co, kk);
            CHECK(o >= 0 && o < (long long)g.Cout * K && ++wseen[(size_t)o] == 1);
        }
    for (size_t i = 0; i < wseen.size(); ++i) CHECK(wseen[i] == 1);
}

static void check_shape(int k, int s, int p, int d, int Cin, int Cout, int Hi, int Wi, int pad_ld) {
    const ConvGeom g = conv_geom(Hi, Wi, Cin, Cout, k, s, p, d);
    CHECK(g.Ho >= 1 && g.Wo >= 1);
    check_dgrad(g, pad_ld);
    check_wgrad(g, pad_ld);
}

// dr_resize_rows_backward_f32: every source texel's gather reads inside grad_out, and each destination pixel's weights sum to one
static void check_resize(int Hs, int Ws, int Hd, int Wd, int C, int pad_ld) {
    const int ldg = C + pad_ld;
    std::vector<float> go((size_t)Hd * Wd * ldg, 1.0f);
    const double sh = resize_scale(Hs, Hd), sw = resize_scale(Ws, Wd);
    double total = 0.0;
    for (int ys = 0; ys < Hs; ++ys)
        for (int xs = 0; xs < Ws; ++xs)
            total += resize_gather(sh, sw, ys, xs, Hs, Ws, Hd, Wd, [&](int pd) {
                CHECK(pd >= 0 && pd < Hd * Wd);
                ++g_slots;
                return go[(size_t)pd * ldg + C - 1];                                 // the last channel a lane reads
            });
    CHECK(std::fabs(total - (double)Hd * Wd) <= 1e-9 * Hd * Wd);
}

// every conv and resample of ImageBackbone(1, out, base) on an H x W image with an h x w DINO grid (EXP/image_backbone.py:81-289)
static void check_backbone(int H, int W, int h, int w, int base, int out, int pad_ld) {
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
    check_resize(h, w, H3, W3, 4 * b, pad_ld);
    check_resize(H3, W3, H2, W2, 4 * b, pad_ld);
    check_resize(H2, W2, H1, W1, 2 * b, pad_ld);
    check_resize(H1, W1, H, W, b, pad_ld);
}

int main() {
    // tests/image_backbone2d3d_ref.CONV_CASES, then the cases of tests/test_image_backbone2d3d_bwd_gpu.py: (k, s, p, d, Cin, Cout, H, W)
    const int cases[][8] = {{3, 1, 1, 1, 16, 16, 5, 7},   {3, 2, 1, 1, 16, 32, 21, 27},  {7, 2, 3, 1, 1, 16, 21, 27},   {7, 2, 3, 1, 3, 16, 21, 27},
                            {1, 1, 0, 1, 64, 64, 3, 4},   {3, 1, 2, 2, 16, 16, 9, 9},    {3, 1, 1, 1, 20, 160, 13, 11}, {3, 1, 1, 1, 16, 16, 1, 1},
                            {3, 1, 1, 1, 128, 16, 240, 280},
                            {3, 2, 0, 1, 16, 16, 8, 10},  {3, 3, 2, 2, 8, 12, 14, 17},   {3, 1, 1, 1, 20, 72, 65, 67},  {3, 1, 1, 1, 16, 10, 9, 11},
                            {3, 2, 1, 1, 6, 12, 9, 11}};
    for (const auto& c : cases)
        for (int pad_ld = 0; pad_ld <= 8; pad_ld += 4) check_shape(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], pad_ld);
    check_shape(3, 1, 1, 1, 16, 16, 5, 7, 3);                    // odd leading dimensions (the scalar-load arms)
    check_shape(3, 2, 1, 1, 16, 32, 21, 27, 5);
    {   // the slab rule over a range of pixel counts, the cap and its neighbourhood included
        const ConvGeom g1 = conv_geom(1, 1, 4, 4, 1, 1, 0, 1);
        for (int M = 1; M <= 400000; M += (M < 5000 ? 1 : 997)) {
            const ConvSlabs sl = conv_wgrad_slabs(M);
            CHECK(sl.S >= 1 && sl.S <= CV_WG_MAX_SLABS && sl.L % CV_WG_CHUNK == 0 && (long long)sl.S * sl.L >= M && (long long)(sl.S - 1) * sl.L < M);
            (void)g1;
        }
    }
    const int resizes[][4] = {{3, 4, 6, 7}, {11, 14, 21, 27}, {6, 7, 6, 7}, {1, 1, 5, 3}, {21, 27, 6, 7}};
    for (const auto& r : resizes)
        for (int pad_ld = 0; pad_ld <= 3; pad_ld += 3) check_resize(r[0], r[1], r[2], r[3], 37, pad_ld);
    check_backbone(24, 32, 2, 3, 16, 16, 0);                     // fixture cases a, b, c
    check_backbone(21, 27, 2, 3, 16, 16, 0);
    check_backbone(24, 32, 3, 4, 16, 24, 0);
    check_backbone(48, 64, 4, 5, 128, 128, 0);                   // the real-width test
    check_backbone(480, 640, 34, 45, 128, 128, 0);               // production
    std::printf("conv_bwd_index_check ok: %lld staging slots walked\n", g_slots);
    return 0;
}
