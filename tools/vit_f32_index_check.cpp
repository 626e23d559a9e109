// vit_f32_index_check.cpp -- host check of csrc/vit_f32_index.h, the only place the float32 ViT kernels (csrc/vit_f32.hip) compute a global or an LDS
// offset.  Build and run:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/vit_f32_index_check.cpp \
//         -o /tmp/vit_f32_index_check && /tmp/vit_f32_index_check
//
// For the production shape (476 x 630 image, patch 14, D = 1024, Dh = 4096: 1531 tokens) and every shape of tests/test_depth_encoder2d3d_gpu.py it
// walks what the kernels walk, on real allocations of exactly the documented sizes (AddressSanitizer guards their ends; every visited offset is
// read or written):
//   patch gather: every (patch, k) of the float32 rows -- vit_index.h's map, in-image offsets a bijection onto the image, pad columns -1;
//   rows GEMM, each of the three tiles: every workgroup, every chunk, every staging slot of A (ragged last row tile: rows past M clamp) and of W
//     (ragged last column tile: rows past N clamp), a float4 each, into an LDS buffer of exactly the kernel's size; every fragment read of every
//     wave, lane, tile and k group finds the four k it is meant to (and the k groups of the WK wave groups together cover a chunk once); every
//     accumulator register's store lands inside `out`, on a distinct element, and all of out[M, N] is covered exactly once; the k reduction's
//     slots are distinct and inside the kernel's LDS;
//   the tile rule: the production shapes take the tiles DESIGN 5r names;
//   workspace: the carve's regions are disjoint, aligned and inside the total, which is what the size query reports.
// The patch and the workspace walks are tools/vit_check_common.h's, shared with tools/vit_index_check.cpp.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vit_f32_index.h"

using namespace dr;

static long long g_slots = 0;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "vit_f32_index_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

#include "vit_check_common.h"      // check_patches, check_carve

// one operand's staging of one chunk by all threads of the workgroup, then what the fragment reads expect
template <class T>
static void stage_operand(const std::vector<uint32_t>& src, int rows, int ld, int row0, int BR, int slots, int chunk, uint32_t* lds_op) {
    for (int t = 0; t < T::NT; ++t)
        for (int s = 0; s < slots; ++s) {
            const int slot = t + s * T::NT;
            CHECK(slot < BR * T::C4);
            const long long g = vit_f32_src(rows, ld, row0, slot, chunk);
            CHECK(g >= 0 && g % 4 == 0 && g + 4 <= (long long)src.size());
            const int at = vit_f32_lds_at(vit_f32_slot_row(slot), vit_f32_slot_k(slot));
            CHECK(at >= 0 && at % 4 == 0 && at + 4 <= BR * T::LDT);
            for (int e = 0; e < 4; ++e) lds_op[at + e] = src.data()[g + e];
            ++g_slots;
        }
}

template <class T>
static void check_gemm_tile(int M, int K, int N, int lda, int ldw, int ldo) {
    CHECK(K % 32 == 0 && N % 16 == 0 && lda >= K && lda % 4 == 0 && ldw >= K && ldw % 4 == 0 && ldo >= N);
    // exactly the documented sizes: (rows - 1) ld + K elements of an operand, (M - 1) ldo + N of out
    std::vector<uint32_t> a((size_t)(M - 1) * lda + K), w((size_t)(N - 1) * ldw + K);
    for (int r = 0; r < M; ++r)
        for (int k = 0; k < K; ++k) a[(size_t)r * lda + k] = (uint32_t)(r * 8192 + k);
    for (int r = 0; r < N; ++r)
        for (int k = 0; k < K; ++k) w[(size_t)r * ldw + k] = (uint32_t)(r * 8192 + k);
    std::vector<unsigned char> out((size_t)(M - 1) * ldo + N, 0);
    std::vector<uint32_t> lds((size_t)T::SMEM_FLOATS);
    const int nchunks = K / 32;
    // (the chunks walk alike: the first, the second and the last one show both buffers and the end of k)
    const int chunks[3] = {0, nchunks > 1 ? 1 : 0, nchunks - 1};
    for (int bm = 0; bm < M; bm += T::BM)
        for (int bn = 0; bn < N; bn += T::BN) {
            for (int ci = 0; ci < 3; ++ci) {
                const int ch = chunks[ci];
                CHECK((ch & 1) * T::STAGE + T::STAGE <= T::SMEM_FLOATS);
                uint32_t* As = lds.data() + (ch & 1) * T::STAGE;
                uint32_t* Bs = As + T::BM * T::LDT;
                stage_operand<T>(a, M, lda, bm, T::BM, T::A_SLOTS, ch, As);
                stage_operand<T>(w, N, ldw, bn, T::BN, T::B_SLOTS, ch, Bs);
                for (int wv = 0; wv < T::NW; ++wv) {
                    const int wk = wv % T::WK, wn = (wv / T::WK) % T::WN, wm = wv / (T::WK * T::WN);
                    for (int lane = 0; lane < 64; ++lane) {
                        const int h = lane >> 5, l31 = lane & 31;
                        for (int g = 0; g < T::GROUPS; ++g) {
                            const int k0 = ch * 32 + (wk * T::GROUPS + g) * 8 + 4 * h;
                            for (int i = 0; i < T::TM; ++i) {
                                const int at = vit_f32_frag_at(wm * T::TM, i, l31, h, wk, T::GROUPS, g);
                                CHECK(at >= 0 && at % 4 == 0 && at + 4 <= T::BM * T::LDT);
                                int row = bm + (wm * T::TM + i) * 32 + l31;
                                if (row > M - 1) row = M - 1;
                                for (int e = 0; e < 4; ++e) CHECK(As[at + e] == (uint32_t)(row * 8192 + k0 + e));
                            }
                            for (int j = 0; j < T::TN; ++j) {
                                const int at = vit_f32_frag_at(wn * T::TN, j, l31, h, wk, T::GROUPS, g);
                                CHECK(at >= 0 && at % 4 == 0 && at + 4 <= T::BN * T::LDT);
                                int col = bn + (wn * T::TN + j) * 32 + l31;
                                if (col > N - 1) col = N - 1;
                                for (int e = 0; e < 4; ++e) CHECK(Bs[at + e] == (uint32_t)(col * 8192 + k0 + e));
                            }
                        }
                    }
                }
            }
            // the stores of k-group 0's waves
            for (int wv = 0; wv < T::NW; ++wv) {
                const int wk = wv % T::WK, wn = (wv / T::WK) % T::WN, wm = wv / (T::WK * T::WN);
                if (wk != 0) continue;
                for (int lane = 0; lane < 64; ++lane) {
                    const int h = lane >> 5, l31 = lane & 31;
                    for (int j = 0; j < T::TN; ++j) {
                        const int col = bn + (wn * T::TN + j) * 32 + l31;
                        if (col >= N) continue;
                        for (int i = 0; i < T::TM; ++i)
                            for (int r = 0; r < 16; ++r) {
                                const int row = bm + (wm * T::TM + i) * 32 + vit_f32_acc_row(r, h);
                                if (row >= M) continue;
                                const long long o = vit_f32_out_at(row, ldo, col);
                                CHECK(o >= 0 && o < (long long)out.size() && !out[o]);
                                out.data()[o] = 1;
                                ++g_slots;
                            }
                    }
                }
            }
        }
    for (int r = 0; r < M; ++r)
        for (int c = 0; c < ldo && (size_t)r * ldo + c < out.size(); ++c) CHECK(out[(size_t)r * ldo + c] == (c < N ? 1 : 0));
    // a tile's 32 rows: the accumulator registers of the two lane halves cover them once
    unsigned char rowseen[32] = {0};
    for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 16; ++r) {
            const int row = vit_f32_acc_row(r, h);
            CHECK(row >= 0 && row < 32 && !rowseen[row]);
            rowseen[row] = 1;
        }
    // the k reduction's slots
    if (T::WK > 1) {
        std::vector<unsigned char> red((size_t)T::SMEM_FLOATS, 0);
        for (int wv = 0; wv < T::NW; ++wv)
            for (int i = 0; i < T::TM; ++i)
                for (int j = 0; j < T::TN; ++j)
                    for (int r = 0; r < 16; ++r)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int at = vit_f32_red_at(wv, T::TM, T::TN, i, j, r, lane);
                            CHECK(at >= 0 && at < T::RED && T::RED <= T::SMEM_FLOATS && !red[at]);
                            red.data()[at] = 1;
                        }
        // k-group 0 of (wm, wn) is wave w, its partners w + 1 .. w + WK - 1: the same (wm, wn)
        for (int wv = 0; wv < T::NW; wv += T::WK)
            for (int o = 1; o < T::WK; ++o) CHECK((wv + o) / T::WK == wv / T::WK && (wv + o) % T::WK == o);
    }
}

static void check_gemm(int M, int K, int N, int lda, int ldw, int ldo) {
    check_gemm_tile<VitF32Tile0>(M, K, N, lda, ldw, ldo);
    check_gemm_tile<VitF32Tile1>(M, K, N, lda, ldw, ldo);
    check_gemm_tile<VitF32Tile2>(M, K, N, lda, ldw, ldo);
}

int main() {
    static_assert(VitF32Tile0::SMEM_FLOATS * 4 <= 160 * 1024 && VitF32Tile1::SMEM_FLOATS * 4 <= 160 * 1024 && VitF32Tile2::SMEM_FLOATS * 4 <= 160 * 1024,
                  "a tile's LDS");
    const int images[][2] = {{476, 630}, {42, 70}, {70, 70}, {140, 182}};
    for (const auto& im : images) check_patches<float>(im[0], im[1], 14);
    const int Ms[] = {1, 31, 33, 129, 131}, Ks[] = {32, 128, 608, 1024, 4096}, Ns[] = {16, 128, 384};
    for (int M : Ms)
        for (int K : Ks)
            for (int N : Ns) {
                check_gemm(M, K, N, K, K, N);
                check_gemm(M, K, N, K + 4, K + 8, N + 3);
            }
    // the fixture encoder's and the production-width test's GEMMs (16, 26, 131 tokens)
    const int Ls[] = {16, 26, 131};
    for (int L : Ls) {
        check_gemm(L - 1, 608, 128, 608, 608, 128);
        check_gemm(L, 128, 384, 128, 128, 384);
        check_gemm(L, 128, 128, 128, 128, 128);
        check_gemm(L, 128, 512, 128, 128, 512);
        check_gemm(L, 512, 128, 512, 512, 128);
    }
    check_gemm(130, 608, 1024, 608, 608, 1024);
    check_gemm(131, 1024, 3072, 1024, 1024, 3072);
    check_gemm(131, 1024, 4096, 1024, 1024, 4096);
    check_gemm(131, 4096, 1024, 4096, 4096, 1024);
    // production: patch embedding, qkv, proj, fc1, fc2 at 1531 tokens
    check_gemm(1530, 608, 1024, 608, 608, 1024);
    check_gemm(1531, 1024, 3072, 1024, 1024, 3072);
    check_gemm(1531, 1024, 1024, 1024, 1024, 1024);
    check_gemm(1531, 1024, 4096, 1024, 1024, 4096);
    check_gemm(1531, 4096, 1024, 4096, 4096, 1024);
    // the rule on those shapes
    CHECK(vit_f32_tile_rule(1530, 608, 1024) == 0);
    CHECK(vit_f32_tile_rule(1531, 1024, 3072) == 2);
    CHECK(vit_f32_tile_rule(1531, 1024, 1024) == 2);
    CHECK(vit_f32_tile_rule(1531, 1024, 4096) == 2);
    CHECK(vit_f32_tile_rule(1531, 4096, 1024) == 2);
    check_carve(476, 630, 14, 1024, 4096, 4);
    check_carve(42, 70, 14, 128, 512, 4);
    check_carve(70, 70, 14, 128, 512, 4);
    check_carve(140, 182, 14, 128, 512, 4);
    check_carve(140, 182, 14, 1024, 4096, 4);
    std::printf("vit_f32_index_check: ok (%lld slots)\n", g_slots);
    return 0;
}
