// fps_index.h -- every index the furthest-point sampling kernels (fps.hip: dr_fps_nodes_f32, dr_fps_batch_f32) compute, stated once for the
// device and for the host check (tools/fps_index_check.cpp): a cloud's slice of the stacked points, the point -> (lane, slot) mapping of the
// on-chip form and the strided walk of the streaming form, the LDS exchange between the waves, the padded outputs, and the workspace that the
// size query and the entries share.  Outside hipcc the file compiles as plain C++.
#pragma once
#include "nonrigid_index.h"      // nr_slice_ok, align256

namespace dr {

constexpr int FPS_BLOCK = 1024;        // threads of the one workgroup that owns a cloud for all its iterations
constexpr int FPS_WAVE = 64;
constexpr int FPS_WAVES = FPS_BLOCK / FPS_WAVE;   // 16 partial results cross LDS per iteration
constexpr int FPS_SLOTS = 12;          // points a lane keeps in registers: x, y, z and the running distance, 48 VGPRs of the 128 a lane has
                                       // when 16 waves share a compute unit (16 slots spill: the square roots' temporaries and the
                                       // candidate need the rest; 14 is the most that compiles to 0 scratch, 12 leaves a margin)
constexpr int FPS_CAPACITY = FPS_BLOCK * FPS_SLOTS;   // 12 288 points on chip; a larger cloud takes the streaming form
constexpr int FPS_PARTIAL_WORDS = 8;   // one wave's partial: distance, index, x, y, z (+ 3 words of padding: a 32-byte row)

constexpr int FPS_ST_OFFSETS = 2;      // status bit: the cloud's offsets do not describe a slice of the stacked array: no point is read; the count is 0, the row -1 / 0
constexpr int FPS_ST_NONFINITE = 8;    // status bit: a point with a NaN or Inf coordinate was met (it is never selected)
constexpr int FPS_ST_CAP = 64;         // status bit: sample_cap nodes were taken and the stop rule had not been met
constexpr int FPS_ST_START = 128;      // status bit: point 0 has a NaN or Inf coordinate: the cloud yields 0 nodes

__host__ __device__ inline int fps_onchip_capacity() { return FPS_CAPACITY; }

// ---- on-chip form: point i of a cloud lives in slot i / FPS_BLOCK of thread i % FPS_BLOCK, so a wave's lanes read consecutive rows
__host__ __device__ inline int fps_point_thread(int i) { return i % FPS_BLOCK; }
__host__ __device__ inline int fps_point_slot(int i) { return i / FPS_BLOCK; }
__host__ __device__ inline int fps_point_of(int thread, int slot) { return slot * FPS_BLOCK + thread; }
// slots in use by a cloud of n points (uniform over the workgroup: the slot loop stops there)
__host__ __device__ inline int fps_slots_used(int n) { return n <= 0 ? 0 : (n + FPS_BLOCK - 1) / FPS_BLOCK; }
__host__ __device__ inline bool fps_fits_onchip(int n) { return n <= FPS_CAPACITY; }

// ---- streaming form: thread t visits points t, t + FPS_BLOCK, ... < n; visits of a thread
__host__ __device__ inline int fps_stream_visits(int n, int thread) { return n <= thread ? 0 : (n - thread + FPS_BLOCK - 1) / FPS_BLOCK; }

// ---- a row of the stacked coordinates / of the streaming form's distance workspace: both are indexed by the cloud's first row + i
__host__ __device__ inline size_t fps_row(int lo, int i) { return (size_t)lo + (size_t)i; }
__host__ __device__ inline size_t fps_coord(int lo, int i, int c) { return fps_row(lo, i) * 3 + (size_t)c; }
// inside a cloud the kernels add a 32-bit offset to the cloud's base (3 n < 2^31)
__host__ __device__ inline int fps_local_coord(int i, int c) { return 3 * i + c; }
// the batch form has no offset array: cloud b of [B, N, 3] starts at row b N (B N < 2^31 is checked by the entry)
__host__ __device__ inline int fps_batch_lo(int b, int N) { return b * N; }

// ---- LDS exchange: two buffers of FPS_WAVES partials, alternating by iteration parity, so ONE barrier per iteration is enough (a wave that
// writes iteration t + 2 into the buffer of iteration t has passed barrier t + 1, which every wave reaches only after reading iteration t)
constexpr int FPS_LDS_WORDS = 2 * FPS_WAVES * FPS_PARTIAL_WORDS;
__host__ __device__ inline int fps_partial_word(int parity, int wave, int word) {
    return ((parity & 1) * FPS_WAVES + wave) * FPS_PARTIAL_WORDS + word;
}

// ---- padded outputs: cloud p's node k
__host__ __device__ inline size_t fps_out(int p, int cap, int k) { return (size_t)p * (size_t)cap + (size_t)k; }
__host__ __device__ inline size_t fps_out_coord(int p, int cap, int k, int c) { return fps_out(p, cap, k) * 3 + (size_t)c; }

// ---- workspace: the streaming form's running distances, one float per stacked row; nothing when every cloud fits on chip
__host__ __device__ inline size_t fps_workspace_bytes(int n_points, int max_points, bool force_streaming) {
    if (n_points <= 0 || max_points <= 0) return 0;
    if (fps_fits_onchip(max_points) && !force_streaming) return 0;
    return align256((size_t)n_points * sizeof(float));
}

}  // namespace dr
