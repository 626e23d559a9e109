// item2d3d_index_check.cpp -- host check of csrc/item2d3d_index.h, the only place dr_corr_2d3d_mutual_f64, dr_corr_2d3d_radius_f64 and
// dr_overlap_2d3d_f64 compute an index.  Build and run, on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/item2d3d_index_check.cpp \
//         -o /tmp/item2d3d_index_check && /tmp/item2d3d_index_check
//
// For images of 24 x 40, 7 x 5, 1 x 67, 1 x 1, 33 x 16 and 16 x 33 pixels and clouds of 0, 1, 63, 64, 65, 300, IT_STAGE +- 1 and IT_SCAN_CHUNK + 1
// points it walks the launches as the kernels do:
//   windows   for cloud points drawn around, beside, before and behind the image (on every border and corner, nearer to the camera than the
//             radius, with infinite and NaN coordinates), EVERY pixel of the image whose image point the definition admits (|p - q| < r in the
//             kernel's own float64 arithmetic, depth drawn per pixel) lies inside it_window; the lanes' walk visits every pixel of a window
//             exactly once, in ascending flat index per lane, and reads depth from an allocation of exactly H W floats;
//   tiles     every pixel belongs to one thread of one tile, and every window that contains a pixel hits that pixel's tile;
//   stages    the stages of a cloud tile it without gap or overlap and stay inside the [N, 4] array;
//   scan      chunks x threads x items cover 0 .. n exactly once, the offsets of the three phases equal a serial exclusive sum for all three
//             value modes, and every row a writer places lies below its cap inside real output allocations;
//   carve     order, alignment, no overlap, the total.
// AddressSanitizer guards the ends of every allocation.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "item2d3d_index.h"

using namespace dr;

#define CHECK(c)                                                                             \
    do {                                                                                     \
        if (!(c)) {                                                                          \
            std::fprintf(stderr, "item2d3d_index_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
static double rnd() {       // [0, 1)
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

static long long g_pixels = 0, g_admitted = 0;

struct Cam {
    double fx, fy, cx, cy;
};

static bool image_point(const std::vector<float>& depth, int W, const Cam& c, int h, int w, double& x, double& y, double& z) {
    const int flat = h * W + w;
    z = (double)depth[(size_t)flat] / 1000.0;
    if (z > 6.0) z = 0.0;
    if (!(z > 0.0)) return false;
    x = ((double)w - c.cx) * z / c.fx;
    y = ((double)flat / (double)W - c.cy) * z / c.fy;
    return true;
}

static void check_window(int H, int W, const Cam& c, const std::vector<float>& depth, double qx, double qy, double qz, double r) {
    const ItWindow k = it_window(H, W, c.fx, c.fy, c.cx, c.cy, qx, qy, qz, r);
    CHECK(k.h0 >= 0 && k.h1 <= H && k.w0 >= 0 && k.w1 <= W);
    const long long area = it_window_area(k);
    CHECK(area >= 0 && area <= (long long)H * W);
    // the lanes' walk: every pixel of the window once, ascending per lane, depth read inside the allocation
    std::vector<int> seen((size_t)H * W, 0);
    volatile float sink = 0.f;
    for (int lane = 0; lane < IT_WAVE; ++lane) {
        int last = -1;
        for (long long t = lane; t < area; t += IT_WAVE) {
            int h, w;
            it_window_pixel(k, t, h, w);
            CHECK(it_window_has(k, h, w));
            const int flat = h * W + w;
            CHECK(flat > last);
            last = flat;
            sink = sink + depth[(size_t)flat];
            ++seen[(size_t)flat];
            ++g_pixels;
        }
    }
    // containment: whatever the definition admits lies in the window, and the window's pixels were visited exactly once
    for (int h = 0; h < H; ++h)
        for (int w = 0; w < W; ++w) {
            CHECK(seen[(size_t)h * W + w] == (it_window_has(k, h, w) ? 1 : 0));
            double x, y, z;
            if (!image_point(depth, W, c, h, w, x, y, z)) continue;
            const double dx = x - qx, dy = y - qy, dz = z - qz;
            if (std::sqrt((dx * dx + dy * dy) + dz * dz) < r) {
                ++g_admitted;
                CHECK(it_window_has(k, h, w));
                CHECK(it_window_hits_tile(k, h / IT_TILE, w / IT_TILE));
            }
        }
    // tiles: a window hits exactly the tiles it shares a pixel with
    for (int th = 0; th < it_tiles(H); ++th)
        for (int tw = 0; tw < it_tiles(W); ++tw) {
            bool shares = false;
            for (int t = 0; t < IT_TILE_BLOCK; ++t) {
                int h, w;
                if (it_tile_pixel(H, W, th, tw, t, h, w) && it_window_has(k, h, w)) shares = true;
            }
            CHECK(shares == it_window_hits_tile(k, th, tw));
        }
    (void)sink;
}

static void check_image(int H, int W) {
    const double f = 0.75 * (H > W ? H : W);
    const Cam cams[] = {{f, 1.1 * f, (W - 1) / 2.0 + 0.13, (H - 1) / 2.0 + 0.21}, {585.0, 585.0, 320.0, 240.0}, {f, f, -3.5, H + 2.25}};
    std::vector<float> depth((size_t)H * W);
    for (auto& d : depth) {
        const double u = rnd();
        d = u < 0.1 ? 0.f : (u < 0.15 ? 7000.f : (u < 0.25 ? (float)(30 + (int)(rnd() * 90)) : (float)(1400 + (int)(rnd() * 900))));
    }
    // tiles: every pixel has exactly one (tile, thread)
    std::vector<int> owner((size_t)H * W, 0);
    for (int th = 0; th < it_tiles(H); ++th)
        for (int tw = 0; tw < it_tiles(W); ++tw)
            for (int t = 0; t < IT_TILE_BLOCK; ++t) {
                int h, w;
                if (it_tile_pixel(H, W, th, tw, t, h, w)) ++owner[(size_t)h * W + w];
            }
    for (int o : owner) CHECK(o == 1);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (const Cam& c : cams) {
        const double radii[] = {0.0375, 0.12, 0.5};
        for (double r : radii) {
            // around image points (partners exist), shifted by up to 1.5 r
            for (int n = 0; n < 60; ++n) {
                const int h = (int)(rnd() * H), w = (int)(rnd() * W);
                double x, y, z;
                if (!image_point(depth, W, c, h, w, x, y, z)) continue;
                check_window(H, W, c, depth, x + (rnd() - 0.5) * 1.5 * r, y + (rnd() - 0.5) * 1.5 * r, z + (rnd() - 0.5) * 1.5 * r, r);
            }
            // every border and corner, half a pixel and more outside, at a depth the image holds
            const int hs[] = {-2, -1, 0, H / 2, H - 1, H, H + 1}, ws[] = {-2, -1, 0, W / 2, W - 1, W, W + 1};
            for (int h : hs)
                for (int w : ws) {
                    const double z = 1.4 + rnd() * 0.9;
                    check_window(H, W, c, depth, (w + 0.4 - c.cx) * z / c.fx, (h + 0.4 - c.cy) * z / c.fy, z, r);
                    const double zn = 0.03 + rnd() * 0.09;      // near the camera: a small z makes a wide window
                    check_window(H, W, c, depth, (w + 0.4 - c.cx) * zn / c.fx, (h + 0.4 - c.cy) * zn / c.fy, zn, r);
                }
            // nearer than r, on the camera plane, behind it; far outside; not finite
            const double zs[] = {r, 0.5 * r, 1e-300, 0.0, -0.5 * r, -r, -1.0, r * (1 + 1e-15), 1e300};
            for (double z : zs) check_window(H, W, c, depth, (rnd() - 0.5) * 0.1, (rnd() - 0.5) * 0.1, z, r);
            check_window(H, W, c, depth, 1e6, -1e6, 2.0, r);
            check_window(H, W, c, depth, inf, 0.0, 2.0, r);
            check_window(H, W, c, depth, 0.0, nan, 2.0, r);
            check_window(H, W, c, depth, 0.0, 0.0, inf, r);
            check_window(H, W, c, depth, 0.0, 0.0, 2.0, nan);
            check_window(H, W, c, depth, 0.0, 0.0, 2.0, inf);
            check_window(H, W, c, depth, 0.0, 0.0, 2.0, 0.0);
        }
    }
    // qz <= -r admits nothing and r <= 0 admits nothing: the windows are empty there
    CHECK(it_window_area(it_window(H, W, f, f, 1.0, 1.0, 0.0, 0.0, -0.2, 0.1)) == 0);
    CHECK(it_window_area(it_window(H, W, f, f, 1.0, 1.0, 0.0, 0.0, 2.0, 0.0)) == 0);
    CHECK(it_window_area(it_window(H, W, f, f, 1.0, 1.0, 0.0, 0.0, 0.05, 0.1)) == (long long)H * W);
}

static void check_stages(int N) {
    std::vector<double> pts((size_t)N * 4, 1.0);
    volatile double sink = 0.0;
    int covered = 0;
    for (int k0 = 0; k0 < N; k0 += IT_STAGE) {
        const int nk = it_stage_count(N, k0, IT_STAGE);
        CHECK(nk >= 1 && nk <= IT_STAGE && k0 + nk <= N);
        for (int t = 0; t < IT_REV_BLOCK; ++t)
            for (int e = t; e < nk * 4; e += IT_REV_BLOCK) sink = sink + pts[(size_t)k0 * 4 + e];
        covered += nk;
    }
    CHECK(covered == N && it_stage_count(N, N, IT_STAGE) == 0);
    // the tile kernel's stages of IT_TILE_BLOCK windows
    covered = 0;
    for (int k0 = 0; k0 < N; k0 += IT_TILE_BLOCK)
        for (int t = 0; t < IT_TILE_BLOCK; ++t)
            if (k0 + t < N) ++covered;
    CHECK(covered == N);
    (void)sink;
}

static void check_scan(long long n, int mode, long long cap) {
    std::vector<int> val((size_t)n);
    for (auto& v : val) v = mode == IT_SCAN_SET ? (rnd() < 0.3 ? (int)(rnd() * 1000) : -1) : (rnd() < 0.4 ? (int)(rnd() * 5) : 0);
    const int chunks = it_scan_chunks(n);
    CHECK((long long)chunks * IT_SCAN_CHUNK >= n && (chunks == 0 || (long long)(chunks - 1) * IT_SCAN_CHUNK < n));
    std::vector<long long> sums((size_t)chunks, 0), off((size_t)n, -1);
    std::vector<int> seen((size_t)n, 0);
    for (int c = 0; c < chunks; ++c)                                       // phase 1: chunk sums
        for (int t = 0; t < IT_SCAN_BLOCK; ++t)
            for (int e = 0; e < IT_SCAN_ITEMS; ++e) {
                const long long i = it_scan_first(c, t) + e;
                if (i < n) {
                    sums[(size_t)c] += it_scan_value(mode, val[(size_t)i]);
                    ++seen[(size_t)i];
                }
            }
    for (int s : seen) CHECK(s == 1);
    long long running = 0;                                                 // phase 2: exclusive chunk offsets
    for (int c = 0; c < chunks; ++c) {
        const long long s = sums[(size_t)c];
        sums[(size_t)c] = running;
        running += s;
    }
    for (int c = 0; c < chunks; ++c) {                                     // phase 3: offsets per value
        long long at = sums[(size_t)c];
        for (int t = 0; t < IT_SCAN_BLOCK; ++t)
            for (int e = 0; e < IT_SCAN_ITEMS; ++e) {
                const long long i = it_scan_first(c, t) + e;
                if (i < n) {
                    off[(size_t)i] = at;
                    at += it_scan_value(mode, val[(size_t)i]);
                }
            }
    }
    long long serial = 0;
    std::vector<long long> out_a((size_t)cap * 2, -1), out_b((size_t)cap, -1);
    for (long long i = 0; i < n; ++i) {
        CHECK(off[(size_t)i] == serial);
        const long long v = it_scan_value(mode, val[(size_t)i]);
        CHECK(v >= 0);
        for (long long m = 0; m < v; ++m) {                                // the writers: row off + m when below cap
            const long long r = off[(size_t)i] + m;
            if (r < cap) {
                out_a[(size_t)r * 2] = i;
                out_a[(size_t)r * 2 + 1] = i;
                CHECK(out_b[(size_t)r] == -1);                             // one writer per row
                out_b[(size_t)r] = i;
            }
        }
        serial += v;
    }
    CHECK(serial == running);
    const long long written = running < cap ? running : cap;
    for (long long r = 0; r < cap; ++r) CHECK((out_b[(size_t)r] >= 0) == (r < written));
    CHECK(it_saturate_i32(running) == running && it_saturate_i32(0x7fffffffLL + 5) == 0x7fffffff);
}

int main() {
    const int images[][2] = {{24, 40}, {7, 5}, {1, 67}, {1, 1}, {33, 16}, {16, 33}};
    for (const auto& im : images) check_image(im[0], im[1]);
    const int clouds[] = {0, 1, 63, 64, 65, 300, IT_STAGE - 1, IT_STAGE, IT_STAGE + 1, IT_SCAN_CHUNK + 1};
    for (int n : clouds) check_stages(n);
    const long long ns[] = {0, 1, 3, 4, 5, 35, 67, 960, IT_SCAN_CHUNK - 1, IT_SCAN_CHUNK, IT_SCAN_CHUNK + 1, 3 * IT_SCAN_CHUNK + 7,
                            (long long)IT_SCAN_BLOCK * IT_SCAN_CHUNK + 9};
    for (long long n : ns)
        for (int mode : {IT_SCAN_SET, IT_SCAN_SUM, IT_SCAN_POS})
            for (long long cap : {0LL, 1LL, n / 3, n, 2 * n + 3}) check_scan(n, mode, cap);
    // the carve: seven arrays in order, each on 256 bytes, none overlapping, the total covering the last
    const int carve[][3] = {{0, 0, 0}, {7, 5, 64}, {1, 67, 65}, {24, 40, 513}, {476, 630, 30000}, {1, 1, 5000}, {32768, 32768, IT_MAX_POINTS}};
    for (const auto& c : carve) {
        const ItCarve k = it_carve(c[0], c[1], c[2]);
        const size_t n = (size_t)c[2], p = (size_t)c[0] * (size_t)c[1], m = n > p ? n : p;
        CHECK(k.pts == 0 && k.win >= k.pts + n * 32 && k.rpx >= k.win + n * 16 && k.pnt >= k.rpx + n * 8 && k.pix >= k.pnt + n * 4);
        CHECK(k.off >= k.pix + p * 4 && k.sums >= k.off + m * 8 && k.bytes >= k.sums + (size_t)it_scan_chunks((long long)m) * 8);
        CHECK(k.win % 256 == 0 && k.rpx % 256 == 0 && k.pnt % 256 == 0 && k.pix % 256 == 0 && k.off % 256 == 0 && k.sums % 256 == 0);
        CHECK(sizeof(ItWindow) == 16);
    }
    CHECK(it_carve(-3, 5, -1).bytes == 0);
    std::printf("item2d3d_index_check ok: %lld window pixels walked, %lld admitted pixels contained\n", g_pixels, g_admitted);
    return 0;
}
