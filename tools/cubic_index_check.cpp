// cubic_index_check.cpp -- host check of csrc/cubic_index.h, the only place dr_image_cubic_chw_f32 computes a source index.  Build and run
// (DESIGN 5t), on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/cubic_index_check.cpp \
//         -o /tmp/cubic_index_check && /tmp/cubic_index_check
//
// For every (in, out) in 1..48 x 1..48 and for the production axes (480, 476), (640, 630), (640, 644) it walks every destination of the axis as
// the kernel does and asserts (1) every clamped tap lies in [0, in); (2) s lies in [-1, in - 1]; (3) |c0 + c1 + c2 + c3 - 1| <= 2^-22; and, what
// the rule implies: 0 <= t <= 1, the taps never decrease, in == out gives t == 0 and the weights (0, 1, 0, 0).  Each axis is a real allocation of
// exactly 3 `in` floats (AddressSanitizer guards its ends) and every tap the kernel would load is read through the kernel's own address
// expression; a 2-D walk over small images does the same for a padded leading dimension and blends what it reads.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cubic_index.h"

using namespace dr;

static long long g_taps = 0;

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            std::fprintf(stderr, "cubic_index_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static void check_axis(int in, int out) {
    const double scale = cubic_scale(in, out);
    std::vector<float> row((size_t)3 * in, 1.0f);
    volatile float sink = 0.f;
    for (int d = 0; d < out; ++d) {
        int s, idx[4];
        float t, c[4];
        cubic_src(scale, d, s, t);
        CHECK(s >= -1 && s <= in - 1);
        CHECK(t >= 0.0f && t <= 1.0f);                  // (a tiny negative f rounds t to 1: tap s + 1 then carries the whole weight)
        cubic_taps(scale, d, in, idx, c);
        for (int k = 0; k < 4; ++k) {
            CHECK(idx[k] >= 0 && idx[k] < in);
            CHECK(idx[k] == cubic_clamp(s - 1 + k, in));
            if (k) CHECK(idx[k] >= idx[k - 1]);
            for (int ch = 0; ch < 3; ++ch) sink = sink + row[3 * (size_t)idx[k] + ch];
            ++g_taps;
        }
        const double sum = (double)c[0] + (double)c[1] + (double)c[2] + (double)c[3];
        CHECK(std::fabs(sum - 1.0) <= std::ldexp(1.0, -22));
        if (in == out) CHECK(s == d && t == 0.0f && c[0] == 0.0f && c[1] == 1.0f && c[2] == 0.0f && c[3] == 0.0f);
    }
    (void)sink;
}

// the kernel's loads and stores on a real image with `pad` extra floats per source row
static void check_image(int Hs, int Ws, int Hd, int Wd, int pad) {
    const int ld = 3 * Ws + pad;
    std::vector<float> src((size_t)(Hs - 1) * ld + 3 * Ws), out((size_t)3 * Hd * Wd, -1.0f);      // the last row carries no pad
    for (size_t i = 0; i < src.size(); ++i) src[i] = 0.25f;
    const double sh = cubic_scale(Hs, Hd), sw = cubic_scale(Ws, Wd);
    const size_t plane = (size_t)Hd * Wd;
    for (int yd = 0; yd < Hd; ++yd)
        for (int xd = 0; xd < Wd; ++xd) {
            int yi[4], xi[4];
            float cy[4], cx[4], v[3][4][4];
            cubic_taps(sh, yd, Hs, yi, cy);
            cubic_taps(sw, xd, Ws, xi, cx);
            for (int j = 0; j < 4; ++j)
                for (int i = 0; i < 4; ++i)
                    for (int c = 0; c < 3; ++c) v[c][j][i] = src[(size_t)yi[j] * ld + 3 * (size_t)xi[i] + c];
            for (int c = 0; c < 3; ++c) {
                const float r = cubic_blend(cy, cx, v[c]);
                CHECK(std::fabs((double)r - 0.25) <= 0.25 * std::ldexp(1.0, -21));            // a constant image stays constant: both weight sums are 1
                out[c * plane + (size_t)yd * Wd + xd] = cubic_normalize(r, 0.25, 0.5);
            }
        }
    for (float o : out) CHECK(std::fabs(o) <= std::ldexp(1.0, -20));
}

int main() {
    for (int in = 1; in <= 48; ++in)
        for (int out = 1; out <= 48; ++out) check_axis(in, out);
    check_axis(480, 476);
    check_axis(640, 630);
    check_axis(640, 644);
    const int images[][4] = {{1, 1, 14, 14}, {2, 3, 14, 14}, {3, 5, 14, 14}, {5, 7, 5, 7}, {30, 40, 28, 42}, {48, 64, 14, 70}, {9, 11, 28, 28},
                             {4, 640, 4, 630}};
    for (const auto& g : images)
        for (int pad = 0; pad <= 5; pad += 5) check_image(g[0], g[1], g[2], g[3], pad);
    std::printf("cubic_index_check ok: %lld taps walked\n", g_taps);
    return 0;
}
