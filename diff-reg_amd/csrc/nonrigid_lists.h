// nonrigid_lists.h -- what the two non-rigid ICP solvers (nonrigid.hip: Adam; nonrigid_gn.hip: Gauss-Newton) share on the device: the status bits,
// a pair's slices, and the set-up pass that narrows the anchors, normalises their weights and builds the node-major lists both solvers gather
// through.  Every index comes from nonrigid_index.h.
#pragma once
#include "common.h"
#include "nonrigid_index.h"
#include "../../include/diffreg_hip.h"

namespace dr {

constexpr int NR_ST_NODES = 1;    // status bit: points without nodes (graph) / more nodes than max_nodes (solver): nothing is computed
constexpr int NR_ST_OFFSETS = 2;  // status bit: the pair's offsets do not describe a slice of the stacked array: nothing is read
constexpr int NR_ST_INDEX = 4;    // status bit: an anchor / edge endpoint out of range was treated as absent
constexpr int NR_ST_NONFINITE = 8;   // status bit (graph): a non-finite coordinate left a point with fewer than min(K, M) anchors
constexpr int NR_ST_STEP = 16;       // status bit (solver): a negative resumed step count was taken as 0
constexpr double NR_WARP_EPS = 1e-6;   // apply_deformation's default eps, which compute_landmark_cost does not override

struct NrAdj {
    int other;
    float weight;
};

// what a pair's workgroup keeps in registers about its slices
struct NrPair {
    int m0, M, c0, N, e0, E, K;
};

// a pair's slices of the stacked arrays -> S; returns 0, or the status bits that keep the pair from being computed (S is then not set)
__device__ __forceinline__ int nr_pair_slices(const dr_nicp_problem& pb, int pair, NrPair& S) {
    const int ml = pb.m_offsets[pair], mh = pb.m_offsets[pair + 1], cl = pb.c_offsets[pair], ch = pb.c_offsets[pair + 1];
    const int el = pb.e_offsets[pair], eh = pb.e_offsets[pair + 1];
    if (!nr_slice_ok(ml, mh, pb.n_nodes) || !nr_slice_ok(cl, ch, pb.n_corr) || !nr_slice_ok(el, eh, pb.n_edges)) return NR_ST_OFFSETS;
    if (mh - ml > pb.max_nodes) return NR_ST_NODES;
    S.m0 = ml; S.M = mh - ml; S.c0 = cl; S.N = ch - cl; S.e0 = el; S.E = eh - el; S.K = pb.K;
    return 0;
}

// the lists of the workspace (nr_solve_carve)
struct NrLists {
    int32_t* anchor;
    float* weight;
    int32_t* lm_ptr;
    int32_t* lm_corr;
    float4* lm_pw;
    int32_t* out_ptr;
    NrAdj* out_adj;
    int32_t* in_ptr;
    NrAdj* in_adj;
};

// The set-up pass of one pair, run by all NR_SOLVER_BLOCK threads of its workgroup (three barriers inside, one at the end): anchors narrowed to
// pair-local int32 (-1 where absent or out of range) and weights normalised by sum_k w + eps into the workspace; then the node-major lists.  Node
// i's thread counts its entries, a prefix over the nodes gives the rows, the same walk fills them: every list is in ascending entry order.
// `cnt`: LDS scratch of 3 (M + 1) ints; *s_status (LDS) receives NR_ST_INDEX.  A NULL edge_weights is weight 1.
__device__ __forceinline__ void nr_setup_lists(const dr_nicp_problem& pb, const NrLists& L, const NrPair& S, int pair, int* cnt, int* s_status) {
    const int t = threadIdx.x;
    bool bad = false;
    for (int c = t; c < S.N; c += NR_SOLVER_BLOCK) {
        const size_t r = (size_t)(S.c0 + c) * S.K;
        double sum = 0.0;
        for (int k = 0; k < S.K; ++k) sum = sum + (double)pb.anchor_weights[r + k];
        sum = sum + NR_WARP_EPS;
        for (int k = 0; k < S.K; ++k) {
            const long long a = pb.anchor_indices[r + k];
            const bool ok = a >= 0 && a < S.M;
            bad = bad || (!ok && a != -1);
            L.anchor[r + k] = ok ? (int)a : -1;
            L.weight[r + k] = (float)((double)pb.anchor_weights[r + k] / sum);
        }
    }
    __syncthreads();
    const int32_t* anc = L.anchor + (size_t)S.c0 * S.K;
    const long long* edg = (const long long*)pb.edges + (size_t)S.e0 * 2;
    const size_t row0 = (size_t)S.m0 + pair;
    for (int i = t; i < S.M; i += NR_SOLVER_BLOCK) {
        int co = 0, ci = 0;
        for (int e = 0; e < S.E; ++e) {
            const long long u = edg[2 * e], v = edg[2 * e + 1];
            const bool ok = u >= 0 && u < S.M && v >= 0 && v < S.M;
            bad = bad || !ok;
            co += (ok && u == i) ? 1 : 0;
            ci += (ok && v == i) ? 1 : 0;
        }
        cnt[i] = nr_csr_count(anc, S.N * S.K, 1, i);
        cnt[(S.M + 1) + i] = co;
        cnt[2 * (S.M + 1) + i] = ci;
    }
    if (bad) atomicOr(s_status, NR_ST_INDEX);
    __syncthreads();
    if (t < 3 && S.M > 0) nr_csr_prefix(cnt + t * (S.M + 1), S.M);
    __syncthreads();
    for (int i = t; i <= S.M && S.M > 0; i += NR_SOLVER_BLOCK) {
        L.lm_ptr[row0 + i] = cnt[i];
        L.out_ptr[row0 + i] = cnt[(S.M + 1) + i];
        L.in_ptr[row0 + i] = cnt[2 * (S.M + 1) + i];
    }
    for (int i = t; i < S.M; i += NR_SOLVER_BLOCK) {
        int at = cnt[i];
        const size_t base = (size_t)S.c0 * S.K;
        for (int e = 0; e < S.N * S.K; ++e) {
            if (anc[e] != i) continue;
            const int c = e / S.K;
            const float* p = pb.src_corr + (size_t)(S.c0 + c) * 3;
            L.lm_corr[base + at] = c;
            L.lm_pw[base + at] = make_float4(p[0], p[1], p[2], L.weight[base + e]);
            ++at;
        }
        int ao = cnt[(S.M + 1) + i], ai = cnt[2 * (S.M + 1) + i];
        for (int e = 0; e < S.E; ++e) {
            const long long u = edg[2 * e], v = edg[2 * e + 1];
            if (!(u >= 0 && u < S.M && v >= 0 && v < S.M)) continue;
            const float w = pb.edge_weights ? pb.edge_weights[S.e0 + e] : 1.f;
            if (u == i) { L.out_adj[S.e0 + ao].other = (int)v; L.out_adj[S.e0 + ao].weight = w; ++ao; }
            if (v == i) { L.in_adj[S.e0 + ai].other = (int)u; L.in_adj[S.e0 + ai].weight = w; ++ai; }
        }
    }
    __syncthreads();
}

}  // namespace dr
