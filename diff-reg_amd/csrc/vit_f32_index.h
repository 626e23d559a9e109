// vit_f32_index.h -- the index arithmetic of the float32 ViT encoder kernels (vit_f32.hip): the tile geometries of the float32 rows GEMM, the
// global source and the LDS position of every staging slot (ragged last row tile, ragged last column tile), where a lane's accumulator registers
// land in the output and the LDS slots of the in-workgroup k reduction.  The patch gather is vit_index.h's (the same arithmetic: vit_patch_kp,
// vit_patch_src) and the workspace carve vit_forward.h's.  The kernels compute every global and LDS offset through these functions and nothing else, and
// tools/vit_f32_index_check.cpp walks the same functions on the host over the tested and the production shapes.  No HIP type in here: plain C++.
#pragma once
#include "vit_index.h"

namespace dr {

// ---- the rows GEMM's tile -----------------------------------------------------------------------------------------------------------------
// A workgroup is WM x WN x WK waves; a wave owns TM x TN MFMA tiles of 32 x 32; k is staged in chunks of 32 floats into one of two LDS buffers as
// [rows][32 k] with a row stride of 36 floats (ds_read_b128 of 32 consecutive rows at one k offset is then conflict-free).  Each of the WK k-groups
// of waves consumes 32 / WK of a chunk.
template <int TM_, int TN_, int WM_, int WN_, int WK_>
struct VitF32Tile {
    static constexpr int TM = TM_, TN = TN_, WM = WM_, WN = WN_, WK = WK_;
    static constexpr int NW = WM * WN * WK, NT = 64 * NW;
    static constexpr int BM = 32 * TM * WM, BN = 32 * TN * WN;
    static constexpr int BKC = 32, LDT = BKC + 4, C4 = BKC / 4;
    static constexpr int A_SLOTS = BM * C4 / NT, B_SLOTS = BN * C4 / NT;          // float4 slots per thread and chunk
    static constexpr int STAGE = (BM + BN) * LDT;                                   // floats per buffer
    static constexpr int RED = WK > 1 ? NW * TM * TN * 16 * 64 : 0;                 // floats of the k reduction
    static constexpr int SMEM_FLOATS = 2 * STAGE > RED ? 2 * STAGE : RED;
    static constexpr int GROUPS = BKC / WK / 8;                                     // 8-wide k groups per wave and chunk
    static constexpr int NACC = TM * TN == 1 ? 2 : 1;                               // independent accumulators per tile
    static_assert(BM * C4 % NT == 0 && BN * C4 % NT == 0, "every thread stages whole slots");
    static_assert(GROUPS >= 1 && GROUPS % NACC == 0, "k groups per chunk");
};
typedef VitF32Tile<1, 1, 2, 2, 1> VitF32Tile0;      //  64 x  64, 4 waves
typedef VitF32Tile<2, 2, 2, 2, 1> VitF32Tile1;      // 128 x 128, 4 waves
typedef VitF32Tile<1, 1, 2, 2, 2> VitF32Tile2;      //  64 x  64, 8 waves: two k-groups, reduced through LDS

// the tile of a shape: 64 x 64, with the k range split over two wave groups inside the workgroup when it is long enough to pay for the
// reduction (K >= 1024).  The shape alone decides.  The 128 x 128 tile is never chosen: at 1531 tokens it measured slower on every ViT-L/14 GEMM
// (the whole encoder 21.3 ms with it forced against 14.9 ms with the 8-wave 64 x 64 tile); it stays forceable for the tests and for wider shapes.
DR_VHD int vit_f32_tile_rule(int M, int K, int N) {
    (void)M; (void)N;
    return K >= 1024 ? 2 : 0;
}

// staging slot `slot` of a chunk (slot = thread + s NT): row `slot / 8` of the tile, k offset 4 (slot % 8) inside the chunk
DR_VHD int vit_f32_slot_row(int slot) { return slot >> 3; }
DR_VHD int vit_f32_slot_k(int slot) { return (slot & 7) * 4; }
// element offset of the float4 a slot fetches: rows past `rows - 1` clamp to the last row (never read past the edge; their products are never
// stored).  K % 32 == 0: a chunk is all inside.
DR_VHD long long vit_f32_src(int rows, int ld, int row0, int slot, int chunk) {
    int r = row0 + vit_f32_slot_row(slot);
    if (r > rows - 1) r = rows - 1;
    return (long long)r * ld + chunk * 32 + vit_f32_slot_k(slot);
}
// float offset inside an operand's LDS image [rows][36] of (tile row r, chunk k)
DR_VHD int vit_f32_lds_at(int r, int k) { return r * 36 + k; }
// the fragment a lane reads for MFMA tile t of its wave row / column block (block = wm TM or wn TN), k group g of k-group wk: four consecutive k
DR_VHD int vit_f32_frag_at(int block, int t, int l31, int h, int wk, int groups, int g) {
    return vit_f32_lds_at((block + t) * 32 + l31, (wk * groups + g) * 8 + 4 * h);
}
// C layout of v_mfma_f32_32x32x2_f32: register r of lane (h, l31) is row (r & 3) + 8 (r >> 2) + 4 h, column l31 of the 32 x 32 tile
DR_VHD int vit_f32_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
DR_VHD long long vit_f32_out_at(int row, int ld, int col) { return (long long)row * ld + col; }
// the k reduction: wave w parks register r of its tile (i, j) at this float offset; k-group 0 adds the others in the order 1 .. WK - 1
DR_VHD int vit_f32_red_at(int w, int TM, int TN, int i, int j, int r, int lane) { return (((w * TM + i) * TN + j) * 16 + r) * 64 + lane; }

}  // namespace dr
