// vit_index.h -- the index arithmetic of the fp16 ViT encoder kernels (vit.hip): the patch gather, the LDS-DMA staging of the rows GEMM's two
// operands (ragged last row tile), the packed weight image and the K / V tile staging of the rows attention (ragged last key tile).  (The
// workspace carve is vit_forward.h's, one for both precisions.)  The kernels compute every global offset through these functions and nothing
// else, and tools/vit_index_check.cpp walks the same functions on the host over the tested and the production shapes before anything runs on a
// device.  No HIP type in here: plain C++.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DR_VHD __host__ __device__ inline
#else
#define DR_VHD inline
#endif

namespace dr {

// ---- patch rows ------------------------------------------------------------------------------------------------------------------------
// nn.Conv2d(3, D, p, stride p) as a GEMM: row = patch (py Wp + px), k = (c p + dy) p + dx -- the order of the flattened [D, 3, p, p] weight --
// padded with zeros to Kp = round_up(3 p p, 32)
DR_VHD int vit_round_up(int v, int m) { return (v + m - 1) / m * m; }
DR_VHD int vit_patch_kp(int p) { return vit_round_up(3 * p * p, 32); }
// element offset inside the [3, H, W] image of (patch, k), or -1 for a pad column
DR_VHD long long vit_patch_src(int H, int W, int p, int patch, int k) {
    if (k >= 3 * p * p) return -1;
    const int Wp = W / p, py = patch / Wp, px = patch % Wp;
    const int c = k / (p * p), r = k % (p * p), dy = r / p, dx = r % p;
    return ((long long)c * H + (py * p + dy)) * W + px * p + dx;
}

// ---- the rows GEMM's operand images ---------------------------------------------------------------------------------------------------
// Both operands are staged in pieces of 16 rows x 32 k (1 KB: one LDS-DMA instruction of a wave, 16 bytes per lane).  Lane l fills LDS
// position (row l >> 2, 16-byte unit l & 3) of the piece; that position holds the LOGICAL unit (l & 3) ^ ((row >> 2) & 3), so the 16 rows a
// fragment read touches at one logical unit fall on 16 different 16-byte bank slots (rule T2 with the swizzle on the source side, rule 21).
DR_VHD int vit_piece_unit(int lane) { return (lane & 3) ^ ((lane >> 4) & 3); }           // logical unit lane `lane` fetches ((row >> 2) & 3 = lane >> 4)
DR_VHD int vit_piece_read(int row, int unit) { return row * 64 + ((unit ^ ((row >> 2) & 3)) << 4); }   // byte offset of a logical unit inside a piece
// A: element offset of the 8 halves lane `lane` fetches for the piece of rows row0 .. row0 + 15 at k-chunk kc (32 k); rows past M - 1 clamp
// to the last row (never read past the edge; their products are never stored)
DR_VHD long long vit_a_src(int M, int lda, int row0, int kc, int lane) {
    int row = row0 + (lane >> 2);
    if (row > M - 1) row = M - 1;
    return (long long)row * lda + kc * 32 + vit_piece_unit(lane) * 8;
}
// W packed: piece (n-tile nt of 16 columns, k-chunk kc) at element offset (nt KC + kc) 512, the piece's bytes already in LDS order: the source
// of a lane is the piece base + lane * 8 halves.  KC = Kp / 32.
DR_VHD size_t vit_w_piece(int KC, int nt, int kc) { return ((size_t)nt * KC + kc) * 512; }
DR_VHD size_t vit_w_packed_elems(int N, int Kp) { return (size_t)N * Kp; }
// where element (n, k) of the [N, Kp] weight sits in the packed image
DR_VHD size_t vit_w_packed_at(int KC, int n, int k) {
    const int r = n & 15, unit = (k & 31) >> 3;
    return vit_w_piece(KC, n >> 4, k >> 5) + (size_t)(vit_piece_read(r, unit) >> 1) + (k & 7);
}

// ---- the rows attention's K / V tiles ---------------------------------------------------------------------------------------------------
// A tile is 32 keys x 64 features (128-byte rows), staged by four LDS-DMA instructions of 8 keys each: lane l fills (key l >> 3, unit l & 7).
// K: position u of key r holds logical unit u ^ (r & 7) (row reads: the 16 keys of a lane group spread over 8 slots x 2 bank halves);
// V: position u holds u ^ (((r >> 1) & 1) << 2) (transposed reads: the 4 keys x 4 units of a lane group cover the 256-byte bank row once).
DR_VHD int vit_k_swz(int key) { return key & 7; }
DR_VHD int vit_v_swz(int key) { return ((key >> 1) & 1) << 2; }
// element offset inside the packed qkv rows [L, ld] of the 8 halves lane `lane` fetches for instruction `ins` (0 .. 3) of key tile kt;
// which = 1: K, 2: V; keys past L - 1 clamp to the last key (finite data; the softmax drops them)
DR_VHD long long vit_kv_src(int L, int ld, int H, int head, int which, int kt, int ins, int lane) {
    const int r = ins * 8 + (lane >> 3);
    int key = kt * 32 + r;
    if (key > L - 1) key = L - 1;
    const int unit = (lane & 7) ^ (which == 1 ? vit_k_swz(r) : vit_v_swz(r));
    return (long long)key * ld + (which * H + head) * 64 + unit * 8;
}

}  // namespace dr
