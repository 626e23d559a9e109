// carve_check.cpp -- host check of csrc/carve.h: the Carver and the workspace carves of the list entries that hold only plain element types.
// Build and run, on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/carve_check.cpp \
//         -o /tmp/carve_check && /tmp/carve_check
//
// Each carve is walked over extents that straddle a 256-byte boundary for every element width of its layout (4-byte arrays at 63 / 64 / 65,
// 8-byte ones at 31 / 32 / 33, 12-byte rows at 21 / 22) and a power of two (64 / 65, 1024 / 1025), plus a production-sized tuple, on a fake
// non-null base that is never dereferenced: every array starts on a 256-byte boundary, the arrays are disjoint and ascending, the last one ends
// at or before the returned size, and the null-base call (the size query) returns the same number and hands out only null pointers.
// The carves that fill a kernel's argument struct or use element types of a .hip file (collate.hip, metrics.hip, pnp.hip, procrustes.hip,
// stateops.hip, train.hip) are not compiled here; tests/test_workspace_guard_gpu.py runs each of them between guard bands.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "carve.h"

using namespace dr;

static long long g_tests = 0;

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            std::fprintf(stderr, "carve_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

static char* const FAKE = reinterpret_cast<char*>((uintptr_t)1 << 40);      // 256-byte aligned, never dereferenced

struct Region { const void* p; size_t bytes; };

// the regions of a real carve in layout order against the size it returned
static void check_regions(std::initializer_list<Region> regions, size_t total) {
    uintptr_t end = (uintptr_t)FAKE;
    for (const Region& r : regions) {
        const uintptr_t b = (uintptr_t)r.p;
        CHECK(b % 256 == 0);
        CHECK(b >= end);
        end = b + r.bytes;
        ++g_tests;
    }
    CHECK(end <= (uintptr_t)FAKE + total);
}

static const int EXTENTS[] = {1, 3, 21, 22, 31, 32, 33, 63, 64, 65, 1024, 1025, 60000};

int main() {
    CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512);
    CHECK(next_pow2(0) == 1 && next_pow2(1) == 1 && next_pow2(64) == 64 && next_pow2(65) == 128 && next_pow2(1025) == 2048 &&
          next_pow2(1 << 28) == (1 << 28));
    {   // the Carver itself: aligned starts, a null base only counts
        Carver c(FAKE), z(nullptr);
        char* a = c.take<char>(1); double* b = c.take<double>(3);
        CHECK(a == FAKE && (char*)b == FAKE + 256 && c.off == 256 + 24);
        CHECK(z.take<char>(1) == nullptr && z.take<double>(3) == nullptr && z.off == c.off);
    }
    for (int n : EXTENTS) {
        const SortWs w = sort_carve(FAKE, n), z = sort_carve(nullptr, n);
        const size_t total = w.bytes;
        CHECK(w.n_pad >= n && (w.n_pad & (w.n_pad - 1)) == 0 && (w.n_pad == 1 || w.n_pad / 2 < n));
        check_regions({{w.keys, (size_t)w.n_pad * 8}, {w.vals, (size_t)w.n_pad * 4}}, total);
        CHECK(z.bytes == total && !z.keys && !z.vals && z.n_pad == w.n_pad);
    }
    for (int M : {1, 3, 63, 64, 65, 240})
        for (int N : {1, 5, 21, 22, 64, 65, 300})
            for (int Kc : {1, 4, 64})
                for (long long cap : {1ll, 15ll, 63ll, 64ll, 65ll, 1ll << 20}) {
                    const NodeCorrWs w = node_corr_carve(FAKE, M, N, Kc, (size_t)cap), z = node_corr_carve(nullptr, M, N, Kc, (size_t)cap);
                    const size_t total = w.bytes;
                    check_regions({{w.pcd_moved, (size_t)N * Kc * 12}, {w.img_rad, (size_t)M * 4}, {w.row_count, (size_t)M * 4}, {w.pcd_rad, (size_t)N * 4},
                                   {w.cand_i, (size_t)cap * 4}, {w.cand_j, (size_t)cap * 4}, {w.ratio_img, (size_t)cap * 4}, {w.ratio_pcd, (size_t)cap * 4}},
                                  total);
                    CHECK(z.bytes == total && !z.pcd_moved && !z.ratio_pcd);
                }
    for (int ns : EXTENTS)
        for (int nt : EXTENTS) {
            const MutualNnWs w = mutual_nn_carve(FAKE, ns, nt), z = mutual_nn_carve(nullptr, ns, nt);
            const size_t total = w.bytes;
            check_regions({{w.s2t, (size_t)ns * 4}, {w.s2t_d2, (size_t)ns * 4}, {w.t2s, (size_t)nt * 4}, {w.t2s_d2, (size_t)nt * 4}}, total);
            CHECK(z.bytes == total && !z.s2t && !z.t2s_d2);
        }
    for (int ns : EXTENTS) {
        const RadiusPairsWs w = radius_pairs_carve(FAKE, ns), z = radius_pairs_carve(nullptr, ns);
        const size_t total = w.bytes;
        check_regions({{w.moved, (size_t)ns * 12}, {w.row_count, (size_t)ns * 4}}, total);
        CHECK(z.bytes == total && !z.moved && !z.row_count);
    }
    std::printf("carve_check: %lld regions ok\n", g_tests);
    return 0;
}
