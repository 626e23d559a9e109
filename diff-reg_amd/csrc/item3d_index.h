// item3d_index.h -- every index the 3D / 4D dataset-item kernels (item3d.hip: dr_item3d_prepare_f32, dr_radius_pairs_ragged_f32) compute, stated
// once for the device and for the host check (tools/item3d_index_check.cpp): the ragged offset arrays and the row -> pair mapping, the bounds of
// a row selection, the cell coordinate and the cell key of the target grid, the 27-cell sweep as nine runs of the sorted keys, the room a pair
// has in the pair list, the saturation of its counts, and the carve of the workspace the size query and the entry point share.  Outside hipcc
// the file compiles as plain C++.
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
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "carve.h"               // align256, next_pow2

namespace dr {

constexpr int IT3_BLOCK = 256;            // rows per workgroup of the one-row-per-thread kernels
constexpr int IT3_ROWS = 4;               // source rows per workgroup of the sweep kernels (one wave each)
constexpr int IT3_KEY_PAIRS = 32767;      // the pair index takes the 15 bits above the cell coordinates of a key
constexpr int IT3_MAX_PAIRS = 256;        // pairs of one call: it3_pair_of scans the offsets, once per thread or wave (a batch size, not a dataset)
constexpr int IT3_MAX_ROWS = 1 << 28;     // stacked rows of either side
constexpr int IT3_CELL_BITS = 16;
constexpr int IT3_CELL_MAX = (1 << IT3_CELL_BITS) - 1;
constexpr unsigned long long IT3_PAD_KEY = ~0ull;      // the keys behind the last target: they sort to the end

constexpr int IT3_ST_OFFSETS = 2;         // status bit: the pair's offsets do not describe a slice of the stacked array (nothing is read)
constexpr int IT3_ST_SELECT = 4;          // status bit: a selection index outside the raw cloud was met (its row is written as zero)
constexpr int IT3_ST_FLOW = 8;            // status bit: the flow is recomputed but the pair's selected and raw source counts differ

// a pair's slice [lo, hi) of a stacked array of `total` rows: usable only when 0 <= lo <= hi <= total
__host__ __device__ inline bool it3_slice_ok(int lo, int hi, int total) { return lo >= 0 && hi >= lo && hi <= total; }

// the pair whose usable slice holds stacked row `row`, or P when none does.  O(P) reads of the offset array: P is a batch size.
__host__ __device__ inline int it3_pair_of(int P, const int32_t* offsets, int total, int row) {
    for (int p = 0; p < P; ++p) {
        const int lo = offsets[p], hi = offsets[p + 1];
        if (it3_slice_ok(lo, hi, total) && row >= lo && row < hi) return p;
    }
    return P;
}

// a selection entry addresses row `idx` of a raw cloud of n rows
__host__ __device__ inline bool it3_sel_ok(long long idx, int n) { return idx >= 0 && idx < (long long)n; }

// cell coordinate of v on an axis whose grid starts at `origin`, clamped to [0, IT3_CELL_MAX].  The clamp never moves two coordinates apart:
// points one cell apart before it are at most one cell apart after it, so the sweep of the neighbouring cells stays complete for a query
// outside the grid and for a cloud wider than the grid; it only tests more candidates there.  NaN goes to cell 0 (and passes no distance test).
__host__ __device__ inline int it3_cell(float v, float origin, float cell) {
    float f = floorf((v - origin) / cell);
    f = f > 0.f ? f : 0.f;                                  // NaN > 0 is false
    f = f < (float)IT3_CELL_MAX ? f : (float)IT3_CELL_MAX;
    return (int)f;
}

// key of (pair, cell): x in the low bits, so the cells x - 1, x, x + 1 of one (y, z) are one run of the sorted keys
__host__ __device__ inline unsigned long long it3_key(int pair, int x, int y, int z) {
    return ((unsigned long long)(unsigned)pair << (3 * IT3_CELL_BITS)) | ((unsigned long long)(unsigned)z << (2 * IT3_CELL_BITS)) |
           ((unsigned long long)(unsigned)y << IT3_CELL_BITS) | (unsigned long long)(unsigned)x;
}

// run r in [0, 9) of the sweep about cell (cx, cy, cz): the keys [first, last] of the cells (cx - 1 .. cx + 1, cy + r % 3 - 1, cz + r / 3 - 1)
// that lie inside the grid; false when the run's (y, z) lies outside it
__host__ __device__ inline bool it3_run_keys(int pair, int cx, int cy, int cz, int r, unsigned long long& first, unsigned long long& last) {
    const int y = cy + r % 3 - 1, z = cz + r / 3 - 1;
    if (y < 0 || y > IT3_CELL_MAX || z < 0 || z > IT3_CELL_MAX) return false;
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < IT3_CELL_MAX ? cx + 1 : IT3_CELL_MAX;
    first = it3_key(pair, x0, y, z);
    last = it3_key(pair, x1, y, z);
    return true;
}

// first position in [lo, hi) of the ascending keys whose key is >= v (hi when none)
__host__ __device__ inline int it3_lower_bound(const unsigned long long* keys, int lo, int hi, unsigned long long v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// rows of room pair p has in a pair list of `capacity` rows, from its slice [lo, hi) of the int64 room offsets: never negative, never past the
// end of the list; 0 when lo lies outside it
__host__ __device__ inline long long it3_room(long long lo, long long hi, long long capacity) {
    if (lo < 0 || lo > capacity) return 0;
    const long long end = hi < capacity ? hi : capacity;
    return end > lo ? end - lo : 0;
}

// a count as the int32 the caller reads: saturated at 2^31 - 1
__host__ __device__ inline int32_t it3_saturate(long long n) { return n > 0x7fffffffLL ? 0x7fffffff : (n < 0 ? 0 : (int32_t)n); }

// workgroups of a one-row-per-thread launch over n rows (at least one: it also serves an empty side)
__host__ __device__ inline unsigned it3_blocks(int n, int per) { return n <= 0 ? 1u : (unsigned)((n + per - 1) / per); }

// the workspace of dr_radius_pairs_ragged_f32: the moved sources, per source row its count and then its first rank (int64), the grid origin of
// every pair, the (key, target) list padded to a power of two for the sort, the targets in key order
struct It3PairsCarve {
    size_t moved, row_start, origin, keys, vals, sorted, bytes;
};
__host__ __device__ inline It3PairsCarve it3_pairs_carve(int P, int ns, int nt) {
    It3PairsCarve c;
    const size_t p = P > 0 ? (size_t)P : 0, s = ns > 0 ? (size_t)ns : 0, t = nt > 0 ? (size_t)nt : 0;
    const size_t pad = nt > 0 ? (size_t)next_pow2(nt) : 0;
    c.moved = 0;
    c.row_start = c.moved + align256(s * 3 * sizeof(float));
    c.origin = c.row_start + align256(s * sizeof(int64_t));
    c.keys = c.origin + align256(p * 4 * sizeof(float));
    c.vals = c.keys + align256(pad * sizeof(unsigned long long));
    c.sorted = c.vals + align256(pad * sizeof(uint32_t));
    c.bytes = c.sorted + align256(t * 4 * sizeof(float));
    return c;
}

}  // namespace dr
