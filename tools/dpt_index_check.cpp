// dpt_index_check.cpp -- host check of the DPT head's additions to csrc/conv_index.h: the slot and store map of dr_conv_transpose2d_rows_f32
// (TransMap in csrc/conv2d.hip) and the row map of dr_conv2d_rows_project_f32's epilogue.  Build and run:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/dpt_index_check.cpp \
//         -o /tmp/dpt_index_check && /tmp/dpt_index_check
//
// Transposed convolution, over a sweep of small geometries (s = 1 .. 8, odd extents, Cin and s s Cout on both sides of a k-chunk and of a
// column tile, contiguous and padded leading dimensions), the tested shapes and production (34 x 45, 256 and 512 channels), for both tile sizes:
// it walks what the kernel walks -- every workgroup tile, every staging slot (tile row, 4-wide group of every k-chunk, tails included) of x and
// of the packed weight, every element of the epilogue -- and asserts (1) every offset returned lies, with the 4 floats a slot reads, inside its
// buffer; (2) every (input pixel, channel) and every packed weight element is visited exactly once per tile row / column and nothing else is;
// (3) every element of out [H s W s, Cout] is stored exactly once and no pad column is touched; (4) the store agrees with the definition
// out[(y s + i)(W s) + x s + j][co], and the bias index is co.  The buffers are real allocations of exactly their extent (AddressSanitizer
// guards their ends); every visited offset is read or written.
// Project entry: for every geometry of a sweep (k = 1, 3, stride 1 and 2, odd extents, ldo = 1 and padded) every workgroup's (wave row, tile,
// register, lane half) maps through conv_tile_row to each of the tile's 64 rows exactly once, the LDS slot it names lies inside the 64 doubles
// the epilogue uses, and conv_p_o_offset stores every output pixel exactly once, inside out, and nothing else.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv_index.h"

using namespace dr;

static long long g_slots = 0, g_geoms = 0;

#define CHECK(c)                                                                    \
    do {                                                                            \
        if (!(c)) {                                                                 \
            std::fprintf(stderr, "dpt_index_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

static void check_transpose(int H, int W, int Cin, int Cout, int s, int pad_ld) {
    const ConvGeom g = conv_t_geom(H, W, Cin, Cout, s);
    const int ldx = Cin + pad_ld, ldo = Cout + pad_ld, M = H * W, N = conv_t_cols(g), R = g.Ho * g.Wo;
    CHECK(g.Ho == H * s && g.Wo == W * s && g.K == Cin && N == s * s * Cout && Cin % 4 == 0);
    std::vector<float> x((size_t)M * ldx, 1.0f), w((size_t)N * Cin, 1.0f), out((size_t)(R - 1) * ldo + Cout, 0.0f);
    volatile float sink = 0.f;
    const int tile_sizes[2] = {64, 128};
    for (int ts = 0; ts < 2; ++ts) {
        const int B = tile_sizes[ts], tiles_m = (M + B - 1) / B, tiles_n = (N + B - 1) / B, nchunks = (Cin + 31) / 32;
        std::vector<unsigned char> seen((size_t)M * Cin, 0), wseen((size_t)N * Cin, 0);
        std::fill(out.begin(), out.end(), 0.0f);
        for (int tm = 0; tm < tiles_m; ++tm)
            for (int ch = 0; ch < nchunks; ++ch)
                for (int r = 0; r < B; ++r)
                    for (int q = 0; q < 8; ++q) {
                        const int m = tm * B + r, kk = ch * 32 + 4 * q;
                        const long long off = conv_t_a_offset(g, m, kk, ldx);
                        ++g_slots;
                        if (off < 0) {
                            CHECK(m >= M || kk >= Cin);
                            continue;
                        }
                        CHECK(m < M && kk + 3 < Cin && off + 3 < (long long)x.size());
                        for (int e = 0; e < 4; ++e) {
                            sink = sink + x[(size_t)off + e];
                            CHECK(conv_t_a_offset(g, m, kk + e, ldx) == off + e && off + e == (long long)m * ldx + kk + e);
                            CHECK(++seen[(size_t)m * Cin + kk + e] == 1);
                        }
                    }
        for (int tn = 0; tn < tiles_n; ++tn)
            for (int ch = 0; ch < nchunks; ++ch)
                for (int r = 0; r < B; ++r)
                    for (int q = 0; q < 8; ++q) {
                        const int n = tn * B + r, kk = ch * 32 + 4 * q;
                        const long long off = conv_t_w_offset(g, n, kk);
                        if (off < 0) {
                            CHECK(n >= N || kk >= Cin);
                            continue;
                        }
                        CHECK(n < N && kk + 3 < Cin && off + 3 < (long long)w.size());
                        for (int e = 0; e < 4; ++e) {
                            sink = sink + w[(size_t)off + e];
                            CHECK(++wseen[(size_t)off + e] == 1);
                        }
                    }
        for (int tm = 0; tm < tiles_m; ++tm)
            for (int tn = 0; tn < tiles_n; ++tn)
                for (int r = 0; r < B; ++r)
                    for (int c = 0; c < B; ++c) {
                        const int m = tm * B + r, n = tn * B + c;
                        const long long off = conv_t_o_offset(g, m, n, ldo);
                        if (off < 0) {
                            CHECK(m >= M || n >= N);
                            continue;
                        }
                        CHECK(m < M && n < N && off < (long long)out.size());
                        // (4) the definition
                        const int y = m / W, xx = m % W, co = n % Cout, tap = n / Cout, i = tap / s, j = tap % s;
                        CHECK(i < s && j < s && conv_t_channel(g, n) == co);
                        CHECK(off == ((long long)(y * s + i) * (W * s) + xx * s + j) * ldo + co);
                        out[(size_t)off] += 1.0f;
                    }
        for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1);
        for (size_t i = 0; i < wseen.size(); ++i) CHECK(wseen[i] == 1);
        for (size_t i = 0; i < out.size(); ++i) CHECK(out[i] == ((int)(i % ldo) < Cout ? 1.0f : 0.0f));       // (3): each once, pads untouched
    }
    (void)sink;
    ++g_geoms;
}

static void check_project(int Hi, int Wi, int k, int stride, int padding, int ldo) {
    const ConvGeom g = conv_geom(Hi, Wi, 4, 32, k, stride, padding, 1);
    CHECK(g.Ho >= 1 && g.Wo >= 1);
    const int M = g.Ho * g.Wo, tiles_m = (M + 63) / 64;
    std::vector<float> out((size_t)(M - 1) * ldo + 1, 0.0f);
    std::vector<double> red(64, 0.0);                                     // the LDS words the epilogue uses: one double per tile row
    for (int tm = 0; tm < tiles_m; ++tm) {
        int hit[64] = {0};
        for (int wm = 0; wm < 2; ++wm)                                    // TM = 1: wave row wm owns 32-row tile wm
            for (int h = 0; h < 2; ++h)
                for (int r = 0; r < 16; ++r) {
                    const int lr = conv_tile_row(wm, r, h);
                    CHECK(lr >= 0 && lr < 64);
                    red[(size_t)lr] += 1.0;                               // wave column 1 writes it, wave column 0 reads it
                    ++hit[lr];
                    const long long off = conv_p_o_offset(g, tm * 64 + lr, ldo);
                    if (off < 0) {
                        CHECK(tm * 64 + lr >= M);
                        continue;
                    }
                    CHECK(off < (long long)out.size() && off == (long long)(tm * 64 + lr) * ldo);
                    out[(size_t)off] += 1.0f;
                }
        for (int i = 0; i < 64; ++i) CHECK(hit[i] == 1);
    }
    for (size_t i = 0; i < out.size(); ++i) CHECK(out[i] == (i % ldo == 0 ? 1.0f : 0.0f));
    CHECK(conv_p_o_offset(g, -1, ldo) == -1 && conv_p_o_offset(g, M, ldo) == -1);
    ++g_geoms;
}

int main() {
    const int extents[][2] = {{1, 1}, {3, 5}, {5, 7}, {10, 13}, {17, 23}};
    const int cins[] = {4, 36, 64}, couts[] = {1, 4, 20, 64};
    for (const auto& e : extents)
        for (int s = 1; s <= 8; ++s)
            for (int cin : cins)
                for (int cout : couts) {
                    if ((long long)e[0] * e[1] * s * s * cout > 600000) continue;                    // (keeps the run to seconds)
                    for (int pad_ld = 0; pad_ld <= 4; pad_ld += 3) check_transpose(e[0], e[1], cin, cout, s, pad_ld);
                }
    check_transpose(34, 45, 256, 256, 4, 0);                             // production: resize_layers[0], resize_layers[1]
    check_transpose(34, 45, 512, 512, 2, 0);
    for (const auto& e : extents)
        for (int k = 1; k <= 3; k += 2)
            for (int stride = 1; stride <= 2; ++stride)
                for (int ldo = 1; ldo <= 3; ldo += 2) check_project(e[0], e[1], k, stride, k / 2, ldo);
    check_project(140, 182, 3, 1, 1, 1);                                 // the largest fixture grid
    check_project(476, 630, 3, 1, 1, 1);                                 // production
    std::printf("dpt_index_check ok: %lld geometries, %lld staging slots walked\n", g_geoms, g_slots);
    return 0;
}
