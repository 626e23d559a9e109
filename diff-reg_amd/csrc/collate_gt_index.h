// collate_gt_index.h -- every index the ground-truth collate kernels (collate_gt.hip: dr_blend_flow_knn3_f32, dr_coarse_gt_matches_f32) compute,
// stated once for the device and for the host check (tools/collate_gt_index_check.cpp): the ragged offset arrays, the mapping of a flat
// workgroup index to (pair, tile of the pair), the bounds of an LDS stage, and the carve of the workspace that the size query and the entry
// point share.  Outside hipcc the file compiles as plain C++.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif
#include <stddef.h>
#include <stdint.h>
#include "carve.h"               // align256

namespace dr {

constexpr int CG_BLOCK = 128;     // queries per workgroup (one per thread)
constexpr int CG_STAGE = 1024;    // reference points per LDS stage (float4 each: 16 KiB)

// a pair's slice [lo, hi) of a stacked array of `total` rows, read from an offset array of P + 1 entries: usable only when
// 0 <= lo <= hi <= total (anything else is reported in the pair's status word and the pair is skipped)
__host__ __device__ inline bool cg_slice_ok(int lo, int hi, int total) { return lo >= 0 && hi >= lo && hi <= total; }

// tiles of CG_BLOCK queries a pair of n queries occupies; a pair without queries keeps one tile, which writes its status / count
__host__ __device__ inline int cg_tiles(int n) { return n <= 0 ? 1 : (n + CG_BLOCK - 1) / CG_BLOCK; }

// the grid: an upper bound of sum_p cg_tiles(n_p) over P pairs whose n_p >= 0 add up to at most `total`, known without reading the offsets
__host__ __device__ inline long long cg_grid_bound(int total, int P) { return (long long)(total < 0 ? 0 : total) / CG_BLOCK + P; }

// flat workgroup b -> (pair, tile): pairs in order, cg_tiles(n_p) tiles each; false when b lies behind the last tile.  A pair whose slice is not
// usable counts as empty (one tile).  O(P) reads of the offset array: P is a batch size.
__host__ __device__ inline bool cg_tile_to_pair(int P, const int32_t* offsets, int total, long long b, int& pair, int& tile) {
    long long first = 0;
    for (int p = 0; p < P; ++p) {
        const int lo = offsets[p], hi = offsets[p + 1];
        const int t = cg_tiles(cg_slice_ok(lo, hi, total) ? hi - lo : 0);
        if (b < first + t) {
            pair = p;
            tile = (int)(b - first);
            return true;
        }
        first += t;
    }
    return false;
}

// points of the stage that starts at reference k0 of a cloud of n: min(CG_STAGE, n - k0), never negative
__host__ __device__ inline int cg_stage_count(int n, int k0) {
    const int left = n - k0;
    return left <= 0 ? 0 : (left < CG_STAGE ? left : CG_STAGE);
}

// the workspace of dr_coarse_gt_matches_f32: per source its nearest target (pair-local index, squared distance), per target its nearest source
struct CgMatchCarve {
    size_t nn_st, d2_st, nn_ts, bytes;
};
__host__ __device__ inline CgMatchCarve cg_match_carve(int ns, int nt) {
    CgMatchCarve c;
    const size_t s = ns > 0 ? (size_t)ns : 0, t = nt > 0 ? (size_t)nt : 0;
    c.nn_st = 0;
    c.d2_st = c.nn_st + align256(s * sizeof(int32_t));
    c.nn_ts = c.d2_st + align256(s * sizeof(float));
    c.bytes = c.nn_ts + align256(t * sizeof(int32_t));
    return c;
}

}  // namespace dr
