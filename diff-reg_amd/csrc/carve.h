// carve.h -- caller memory carved into 256-byte aligned arrays.  A workspace has ONE carve: the size query runs it on a null base, the entry
// point on the caller's pointer.  Plain C++ outside hipcc: tools/carve_check.cpp walks the Carver and the layouts below on the host.  A layout
// is an aggregate with its members in layout order and the total last (a braced list is evaluated left to right).
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

namespace dr {

__host__ __device__ inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
__host__ __device__ inline int next_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }      // (1 for n <= 1)

// hands out consecutive arrays of caller memory, each starting at a multiple of 256 bytes; a null base only counts (`off` = bytes so far)
struct Carver {
    char* base; size_t off;
    explicit Carver(void* p) : base((char*)p), off(0) {}
    template <typename T> T* take(size_t n) {
        off = align256(off);
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return r;
    }
};

struct SortWs { int n_pad; unsigned long long* keys; unsigned* vals; size_t bytes; };   // launch_bitonic_sort's rows, padded to a power of two
inline SortWs sort_carve(void* base, int n) {
    Carver c(base); const int np = next_pow2(n);
    return {np, c.take<unsigned long long>(np), c.take<unsigned>(np), align256(c.off)};
}
// dr_node_correspondences_2d3d_f32: moved patch points [N, Kc, 3], patch radii, candidates per image node, the candidate list and its ratios
struct NodeCorrWs { float *pcd_moved, *img_rad; int* row_count; float* pcd_rad; int *cand_i, *cand_j; float *ratio_img, *ratio_pcd; size_t bytes; };
inline NodeCorrWs node_corr_carve(void* base, int M, int N, int Kc, size_t cap) {
    Carver c(base); return {c.take<float>((size_t)N * Kc * 3), c.take<float>(M), c.take<int>(M), c.take<float>(N),
            c.take<int>(cap), c.take<int>(cap), c.take<float>(cap), c.take<float>(cap), align256(c.off)};
}
struct MutualNnWs { int* s2t; float* s2t_d2; int* t2s; float* t2s_d2; size_t bytes; };   // nearest partner and its squared distance, both ways
inline MutualNnWs mutual_nn_carve(void* base, int ns, int nt) {
    Carver c(base); return {c.take<int>(ns), c.take<float>(ns), c.take<int>(nt), c.take<float>(nt), align256(c.off)};
}
struct RadiusPairsWs { float* moved; int* row_count; size_t bytes; };   // dr_radius_pairs_f32: the moved sources [ns, 3], the pairs per source row
inline RadiusPairsWs radius_pairs_carve(void* base, int ns) {
    Carver c(base); return {c.take<float>((size_t)ns * 3), c.take<int>(ns), align256(c.off)};
}

}  // namespace dr
