// vit_index_check.cpp -- host check of csrc/vit_index.h, the only place the fp16 ViT kernels (csrc/vit.hip) compute a global offset.  Build and run
// (DESIGN 5p):
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/vit_index_check.cpp \
//         -o /tmp/vit_index_check && /tmp/vit_index_check
//
// For the production shape (448 x 616 image, patch 14, D = 1024, Dh = 4096: 1409 tokens) and every shape of tests/test_vit2d3d_gpu.py it walks what
// the kernels walk, on real allocations of exactly the documented sizes (AddressSanitizer guards their ends; every visited offset is read):
//   patch gather: every (patch, k) -- in-image offsets are a bijection onto the image, pad columns are -1;
//   rows GEMM: every workgroup tile of the three tile sizes, every LDS-DMA piece of A (ragged last row tile: rows past M clamp, whole pieces past M
//     are skipped as the kernel skips them) and of the packed weight, 8 halves per lane; the LDS image a fragment read expects is rebuilt from
//     the sources and compared with the operand, so the source-side swizzle and the read-side swizzle agree; the packer's map is a bijection;
//   rows attention: every K / V staging instruction of every key tile (ragged last tile: keys past L clamp), and the rebuilt K / V images
//     against the rows the fragment reads expect;
//   workspace: the carve's regions are disjoint, aligned and inside the total, which is what the size query reports.
// The patch and the workspace walks are tools/vit_check_common.h's, shared with tools/vit_f32_index_check.cpp.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vit_index.h"

using namespace dr;

static long long g_slots = 0;

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            std::fprintf(stderr, "vit_index_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

#include "vit_check_common.h"      // check_patches, check_carve

static void check_gemm(int M, int K, int N, int lda) {
    CHECK(K % 32 == 0 && N % 16 == 0 && lda >= K && lda % 8 == 0);
    const int KC = K / 32;
    // A holds a distinct value per (row, k / 8) so a wrong unit shows; exactly (M - 1) lda + K elements would do, the documented size is M lda
    std::vector<uint32_t> a((size_t)M * lda);
    for (int r = 0; r < M; ++r)
        for (int k = 0; k < lda; ++k) a[(size_t)r * lda + k] = (uint32_t)(r * 4096 + k);
    // packed weight: bijection of (n, k) onto [0, N K)
    std::vector<uint32_t> wp(vit_w_packed_elems(N, K), 0xffffffffu);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) {
            const size_t at = vit_w_packed_at(KC, n, k);
            CHECK(at < wp.size() && wp[at] == 0xffffffffu);
            wp[at] = (uint32_t)(n * 4096 + k);
        }
    const int tiles[3][2] = {{64, 64}, {128, 64}, {128, 128}};
    for (const auto& tl : tiles) {
        const int BM = tl[0], BN = tl[1];
        for (int bm = 0; bm < M; bm += BM)
            for (int kc = 0; kc < KC; ++kc)
                for (int pr = 0; pr < BM / 16; ++pr) {
                    const int row0 = bm + pr * 16;
                    if (row0 >= M) continue;                                     // (the kernel skips the piece)
                    uint32_t piece[512];
                    for (int lane = 0; lane < 64; ++lane) {
                        const long long s = vit_a_src(M, lda, row0, kc, lane);
                        CHECK(s >= 0 && s + 8 <= (long long)a.size() && s % 8 == 0);
                        for (int e = 0; e < 8; ++e) piece[lane * 8 + e] = a[s + e];
                        ++g_slots;
                    }
                    // what a fragment read of (row r, logical unit u) finds
                    for (int r = 0; r < 16; ++r)
                        for (int u = 0; u < 4; ++u) {
                            const int off = vit_piece_read(r, u);
                            CHECK(off >= 0 && off + 16 <= 1024 && off % 16 == 0);
                            const int row = row0 + r < M ? row0 + r : M - 1;
                            for (int e = 0; e < 8; ++e) CHECK(piece[off / 2 + e] == (uint32_t)(row * 4096 + kc * 32 + u * 8 + e));
                        }
                }
        for (int bn = 0; bn < N; bn += BN)
            for (int kc = 0; kc < KC; ++kc)
                for (int pn = 0; pn < BN / 16; ++pn) {
                    const int nt = bn / 16 + pn;
                    if (nt >= N / 16) continue;
                    const size_t base = vit_w_piece(KC, nt, kc);
                    CHECK(base + 512 <= wp.size());
                    for (int r = 0; r < 16; ++r)
                        for (int u = 0; u < 4; ++u)
                            for (int e = 0; e < 8; ++e)
                                CHECK(wp[base + vit_piece_read(r, u) / 2 + e] == (uint32_t)((nt * 16 + r) * 4096 + kc * 32 + u * 8 + e));
                    g_slots += 64;
                }
    }
}

static void check_attention(int L, int H) {
    const int ld = 3 * H * 64 + 8;                                               // a padded leading dimension
    std::vector<uint32_t> qkv((size_t)L * ld);
    for (size_t i = 0; i < qkv.size(); ++i) qkv[i] = (uint32_t)i;
    const int nkt = (L + 31) / 32;
    for (int head = 0; head < H; ++head)
        for (int which = 1; which <= 2; ++which)
            for (int kt = 0; kt < nkt; ++kt) {
                uint32_t tile[2048];
                for (int ins = 0; ins < 4; ++ins)
                    for (int lane = 0; lane < 64; ++lane) {
                        const long long s = vit_kv_src(L, ld, H, head, which, kt, ins, lane);
                        CHECK(s >= 0 && s + 8 <= (long long)qkv.size() && s % 8 == 0);
                        for (int e = 0; e < 8; ++e) tile[ins * 512 + lane * 8 + e] = qkv[s + e];
                        ++g_slots;
                    }
                for (int r = 0; r < 32; ++r) {
                    const int key = kt * 32 + r < L ? kt * 32 + r : L - 1;
                    for (int u = 0; u < 8; ++u) {
                        const int pos = u ^ (which == 1 ? vit_k_swz(r) : vit_v_swz(r));
                        CHECK(pos >= 0 && pos < 8);
                        for (int e = 0; e < 8; ++e)
                            CHECK(tile[r * 64 + pos * 8 + e] == (uint32_t)((size_t)key * ld + (which * H + head) * 64 + u * 8 + e));
                    }
                }
            }
}

int main() {
    const int images[][2] = {{448, 616}, {42, 70}, {70, 70}, {140, 182}};
    for (const auto& im : images) check_patches<uint16_t>(im[0], im[1], 14);
    const int Ms[] = {1, 15, 16, 17, 127, 128, 129, 131}, Ks[] = {32, 608, 1024}, Ns[] = {16, 112, 128, 384};
    for (int M : Ms)
        for (int K : Ks)
            for (int N : Ns) {
                check_gemm(M, K, N, K);
                check_gemm(M, K, N, K + 8);
            }
    // production: patch embedding, qkv, proj, fc1, fc2 at 1409 tokens (A walked at each K; the weight at each (N, K))
    check_gemm(1408, 608, 1024, 608);
    check_gemm(1409, 1024, 3072, 1024);
    check_gemm(1409, 1024, 1024, 1024);
    check_gemm(1409, 1024, 4096, 1024);
    check_gemm(1409, 4096, 1024, 4096);
    const int Ls[] = {1, 16, 26, 31, 32, 33, 127, 128, 129, 131};
    for (int L : Ls)
        for (int H = 1; H <= 2; ++H) check_attention(L, H);
    check_attention(1409, 16);
    check_carve(448, 616, 14, 1024, 4096, 2);
    check_carve(42, 70, 14, 128, 512, 2);
    check_carve(70, 70, 14, 128, 512, 2);
    check_carve(140, 182, 14, 128, 512, 2);
    check_carve(42, 70, 14, 1024, 4096, 2);
    std::printf("vit_index_check: ok (%lld slots)\n", g_slots);
    return 0;
}
