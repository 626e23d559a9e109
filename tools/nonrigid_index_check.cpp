// nonrigid_index_check.cpp -- host check of csrc/nonrigid_index.h, the only place the non-rigid ICP kernels (csrc/nonrigid.hip) compute an index.
// Build and run, on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/nonrigid_index_check.cpp \
//         -o /tmp/nonrigid_index_check && /tmp/nonrigid_index_check
//
// It walks, as the kernels do and on real allocations of exactly the carved sizes (AddressSanitizer guards their ends):
//   * the tile -> (pair, tile) mapping of the anchor search and the warp: every point of every pair is visited exactly once, no tile reaches
//     outside its pair, the grid bound covers all tiles;
//   * the adjacency bit map and its ordered edge scan (count pass, exclusive prefix over the rows, write pass): the edge list is row-major
//     ascending, equals the dense matrix's nonzero list, and stays inside the pair's slice of the edge arrays;
//   * the node-major CSR construction of the solver's set-up pass (anchor columns with -1 and out-of-range entries, out-edges, in-edges) inside
//     the workspace carve: every valid entry lands in exactly one row, rows are ascending, row pointers of neighbouring pairs do not overlap;
//   * the LDS carve: regions disjoint, the scratch of the prefix (3 (M + 1) ints) inside the second parameter copy, the capacity's carve inside
//     NR_LDS_BYTES and the capacity + 1 carve outside it; capacity >= 512;
// over the shapes of the GPU test: (a) M 1, N 3, K 1; (b) M 2, N 700, K 4; (c) M 40, N 120, K 4; (d) M 67, N 1, K 6; (e) -1 anchors with an all -1
// row; (f) (b) + (c) in one ragged call; (g) M = capacity.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "nonrigid_index.h"

using namespace dr;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

struct Pair {
    int M, N, K, points;     // nodes, correspondences, anchors, points of the cloud the graph is built on
    bool holes;
};

static long long g_edges = 0, g_entries = 0;

// exact-size allocation: the vector's data() ends where the carve ends
template <typename T>
static std::vector<T> exact(size_t bytes) { return std::vector<T>((bytes + sizeof(T) - 1) / sizeof(T)); }

static void walk_tiles(const std::vector<Pair>& pairs) {
    const int P = (int)pairs.size();
    std::vector<int32_t> off(P + 1, 0);
    for (int p = 0; p < P; ++p) off[p + 1] = off[p] + pairs[p].points;
    const int total = off[P];
    std::vector<int> seen(total, 0);
    const long long grid = nr_grid_bound(total, P);
    long long tiles = 0;
    for (long long b = 0; b < grid; ++b) {
        int pair = -1, tile = -1;
        if (!nr_tile_to_pair(P, off.data(), total, b, pair, tile)) continue;
        ++tiles;
        CHECK(pair >= 0 && pair < P && tile >= 0 && tile < nr_tiles(pairs[pair].points));
        for (int t = 0; t < NR_TILE; ++t) {
            const int q = tile * NR_TILE + t;
            if (q < pairs[pair].points) ++seen[off[pair] + q];
        }
    }
    int pair, tile;
    CHECK(!nr_tile_to_pair(P, off.data(), total, grid, pair, tile));
    long long want = 0;
    for (const Pair& p : pairs) want += nr_tiles(p.points);
    CHECK(tiles == want);
    for (int v : seen) CHECK(v == 1);
}

// anchors of a pair: K distinct nodes per point where M allows, -1 behind min(K, M)
static std::vector<int32_t> make_anchors(const Pair& p, int rows, std::mt19937& rng) {
    std::vector<int32_t> a((size_t)rows * p.K, -1);
    const int ke = nr_effective_k(p.K, p.M);
    for (int r = 0; r < rows; ++r) {
        const int first = (int)(rng() % (unsigned)p.M);
        for (int k = 0; k < ke; ++k) a[(size_t)r * p.K + k] = (first + k) % p.M;
    }
    return a;
}

static void walk_graph(const std::vector<Pair>& pairs, std::mt19937& rng) {
    const int P = (int)pairs.size();
    std::vector<int32_t> moff(P + 1, 0);
    for (int p = 0; p < P; ++p) moff[p + 1] = moff[p] + pairs[p].M;
    int max_nodes = 0;
    for (const Pair& p : pairs) max_nodes = p.M > max_nodes ? p.M : max_nodes;
    const int n_nodes = moff[P], words = nr_bitmap_words(max_nodes);              // the row stride the host states: the largest pair
    const NrGraphCarve c = nr_graph_carve(n_nodes, max_nodes);
    CHECK(c.bitmap == 0 && c.row_count >= (size_t)n_nodes * words * 4 && c.row_sum >= c.row_count + (size_t)n_nodes * 4 &&
          c.bytes >= c.row_sum + (size_t)n_nodes * 8);
    std::vector<uint32_t> bitmap = exact<uint32_t>((size_t)n_nodes * words * 4);
    std::vector<int32_t> row_count(n_nodes);
    std::vector<int32_t> counts(P);
    std::vector<std::vector<char>> dense(P);
    for (int p = 0; p < P; ++p) {
        const Pair& pr = pairs[p];
        const std::vector<int32_t> anc = make_anchors(pr, pr.points, rng);
        dense[p].assign((size_t)pr.M * pr.M, 0);
        const int ke = nr_effective_k(pr.K, pr.M);
        for (int r = 0; r < pr.points; ++r)
            for (int a = 0; a < ke; ++a)
                for (int b = 0; b < ke; ++b) {
                    const int ia = anc[(size_t)r * pr.K + a], ib = anc[(size_t)r * pr.K + b];
                    bitmap[nr_bitmap_word(moff[p], ia, words, ib)] |= nr_bitmap_bit(ib);
                    dense[p][(size_t)ia * pr.M + ib] = 1;
                }
        // count pass
        int total = 0;
        for (int i = 0; i < pr.M; ++i) {
            int cnt = 0;
            for (int wd = 0; wd < nr_bitmap_words(pr.M); ++wd) cnt += __builtin_popcount(bitmap[nr_bitmap_word(moff[p], i, words, wd * 32)]);
            row_count[moff[p] + i] = cnt;
            total += cnt;
        }
        counts[p] = total;
    }
    std::vector<int32_t> eoff(P + 1, 0);
    for (int p = 0; p < P; ++p) eoff[p + 1] = eoff[p] + counts[p];
    std::vector<int64_t> edges((size_t)eoff[P] * 2, -1);
    for (int p = 0; p < P; ++p) {
        const Pair& pr = pairs[p];
        long long base = eoff[p];
        for (int r0 = 0; r0 < pr.M; r0 += NR_EDGE_BLOCK) {              // the write pass: a block of rows, prefix inside the block
            long long before = 0;
            for (int t = 0; t < NR_EDGE_BLOCK; ++t) {
                const int i = r0 + t;
                if (i >= pr.M) break;
                long long e = base + before;
                for (int wd = 0; wd < nr_bitmap_words(pr.M); ++wd) {
                    uint32_t bits = bitmap[nr_bitmap_word(moff[p], i, words, wd * 32)];
                    while (bits) {
                        const int j = wd * 32 + __builtin_ctz(bits);
                        bits &= bits - 1;
                        CHECK(j < pr.M && e >= eoff[p] && e < eoff[p + 1]);
                        edges[2 * e] = i;
                        edges[2 * e + 1] = j;
                        ++e;
                    }
                }
                before += row_count[moff[p] + i];
                CHECK(e == base + before);
            }
            base += before;
        }
        CHECK(base == eoff[p + 1]);
        long long e = eoff[p];                                           // torch.nonzero of the dense matrix
        for (int i = 0; i < pr.M; ++i)
            for (int j = 0; j < pr.M; ++j)
                if (dense[p][(size_t)i * pr.M + j]) {
                    CHECK(edges[2 * e] == i && edges[2 * e + 1] == j);
                    ++e;
                }
        CHECK(e == eoff[p + 1]);
        g_edges += counts[p];
    }
}

static void walk_solver(const std::vector<Pair>& pairs, std::mt19937& rng) {
    const int P = (int)pairs.size();
    std::vector<int32_t> moff(P + 1, 0), coff(P + 1, 0), eoff(P + 1, 0);
    int K = 0;
    for (const Pair& p : pairs) K = p.K > K ? p.K : K;
    std::vector<std::vector<int32_t>> anc(P);
    std::vector<std::vector<int64_t>> edg(P);
    for (int p = 0; p < P; ++p) {
        Pair pr = pairs[p];
        pr.K = K;
        anc[p] = make_anchors(pr, pr.N, rng);
        if (pr.holes) {
            for (int r = 0; r < pr.N; r += 3) anc[p][(size_t)r * K + K - 1] = -1;
            for (int k = 0; k < K && pr.N > 5; ++k) anc[p][(size_t)5 * K + k] = -1;
            if (pr.N > 7) anc[p][(size_t)7 * K] = pr.M + 3;             // out of range: narrowed to -1 by the set-up pass
        }
        for (int i = 0; i < pr.M; ++i) {                                 // self edge, a ring edge, one long edge
            edg[p].push_back(i); edg[p].push_back(i);
            if (pr.M > 1) { edg[p].push_back(i); edg[p].push_back((i + 1) % pr.M); }
            if (pr.M > 5 && i % 3 == 0) { edg[p].push_back(i); edg[p].push_back((i * 5 + 2) % pr.M); }
        }
        moff[p + 1] = moff[p] + pr.M;
        coff[p + 1] = coff[p] + pr.N;
        eoff[p + 1] = eoff[p] + (int)(edg[p].size() / 2);
    }
    const NrSolveCarve c = nr_solve_carve(P, coff[P], moff[P], eoff[P], K);
    const size_t order[] = {c.resid, c.anchor, c.weight, c.lm_ptr, c.lm_corr, c.lm_pw, c.out_ptr, c.out_adj, c.in_ptr, c.in_adj, c.bytes};
    for (int i = 0; i + 1 < 11; ++i) CHECK(order[i] <= order[i + 1] && order[i] % 256 == 0);
    CHECK(c.anchor - c.resid >= (size_t)coff[P] * 24 && c.lm_pw - c.lm_corr >= (size_t)coff[P] * K * 4 && c.out_ptr - c.lm_pw >= (size_t)coff[P] * K * 16 &&
          c.in_ptr - c.out_adj >= (size_t)eoff[P] * 8 && c.bytes - c.in_adj >= (size_t)eoff[P] * 8);
    std::vector<int32_t> lm_ptr = exact<int32_t>((size_t)(moff[P] + P) * 4), out_ptr = lm_ptr, in_ptr = lm_ptr;
    std::vector<int32_t> lm_corr = exact<int32_t>((size_t)coff[P] * K * 4), out_adj = exact<int32_t>((size_t)eoff[P] * 4), in_adj = out_adj;
    for (int p = 0; p < P; ++p) {
        const Pair& pr = pairs[p];
        const int M = pr.M, N = pr.N, E = eoff[p + 1] - eoff[p];
        const NrLdsCarve l = nr_lds_carve(M);
        CHECK(l.param1 == M * NR_COMP && l.exp_avg == 2 * M * NR_COMP && l.exp_avg_sq == 3 * M * NR_COMP && l.node == 4 * M * NR_COMP);
        CHECK(l.reduce_byte >= (l.node + 3 * M) * 4 && l.reduce_byte % 8 == 0 && l.status_byte == l.reduce_byte + NR_REDUCE_BYTES && l.bytes == l.status_byte + 8);
        CHECK(3 * (M + 1) <= M * NR_COMP);                               // the prefix scratch inside the second parameter copy
        std::vector<int32_t> narrowed(anc[p]);
        for (int32_t& a : narrowed) a = (a >= 0 && a < M) ? a : -1;
        std::vector<int32_t> cnt = exact<int32_t>((size_t)M * NR_COMP * 4);
        std::vector<int32_t> ekey_u(E), ekey_v(E);
        for (int e = 0; e < E; ++e) { ekey_u[e] = (int32_t)edg[p][2 * e]; ekey_v[e] = (int32_t)edg[p][2 * e + 1]; }
        for (int i = 0; i < M; ++i) {
            cnt[i] = nr_csr_count(narrowed.data(), N * K, 1, i);
            cnt[(M + 1) + i] = nr_csr_count(ekey_u.data(), E, 1, i);
            cnt[2 * (M + 1) + i] = nr_csr_count(ekey_v.data(), E, 1, i);
        }
        int valid = 0;
        for (int32_t a : narrowed) valid += a >= 0;
        CHECK(nr_csr_prefix(cnt.data(), M) == valid && valid <= N * K);
        CHECK(nr_csr_prefix(cnt.data() + (M + 1), M) == E && nr_csr_prefix(cnt.data() + 2 * (M + 1), M) == E);
        const size_t row0 = (size_t)moff[p] + p;
        for (int i = 0; i <= M; ++i) {
            lm_ptr[row0 + i] = cnt[i];
            out_ptr[row0 + i] = cnt[(M + 1) + i];
            in_ptr[row0 + i] = cnt[2 * (M + 1) + i];
        }
        std::vector<int> hit((size_t)N * K, 0);
        for (int i = 0; i < M; ++i) {
            int at = cnt[i];
            int last = -1;
            for (int e = 0; e < N * K; ++e) {
                if (narrowed[e] != i) continue;
                CHECK(at < cnt[i + 1] && e > last);
                lm_corr[(size_t)coff[p] * K + at] = e / K;
                ++hit[e];
                last = e;
                ++at;
            }
            CHECK(at == cnt[i + 1]);
            int ao = cnt[(M + 1) + i], ai = cnt[2 * (M + 1) + i];
            for (int e = 0; e < E; ++e) {
                if (ekey_u[e] == i) { CHECK(ao < cnt[(M + 1) + i + 1]); out_adj[eoff[p] + ao++] = ekey_v[e]; }
                if (ekey_v[e] == i) { CHECK(ai < cnt[2 * (M + 1) + i + 1]); in_adj[eoff[p] + ai++] = ekey_u[e]; }
            }
            CHECK(ao == cnt[(M + 1) + i + 1] && ai == cnt[2 * (M + 1) + i + 1]);
        }
        for (size_t e = 0; e < hit.size(); ++e) CHECK(hit[e] == (narrowed[e] >= 0 ? 1 : 0));
        g_entries += valid + 2LL * E;
    }
}

int main() {
    std::mt19937 rng(7);
    const int cap = nr_node_capacity();
    CHECK(cap >= 512);
    CHECK(nr_lds_carve(cap).bytes <= NR_LDS_BYTES && nr_lds_carve(cap + 1).bytes > NR_LDS_BYTES);
    CHECK(nr_pow_int(0.9, 0) == 1.0 && nr_pow_int(0.9, 1) == 0.9 && nr_pow_int(0.5, 10) == 1.0 / 1024.0);
    CHECK(nr_stage_count(NR_STAGE + 3, NR_STAGE) == 3 && nr_stage_count(5, 8) == 0 && nr_effective_k(6, 2) == 2);
    const Pair a = {1, 3, 1, 3, false}, b = {2, 700, 4, 700, false}, c = {40, 120, 4, 300, false}, d = {67, 1, 6, 1, false},
               e = {40, 120, 4, 300, true}, g = {cap, 333, 6, 1100, false};
    const std::vector<std::vector<Pair>> sets = {{a}, {b}, {c}, {d}, {e}, {b, c}, {g}, {a, d, e, b}};
    for (const std::vector<Pair>& s : sets) {
        walk_tiles(s);
        walk_graph(s, rng);
        walk_solver(s, rng);
    }
    std::printf("nonrigid_index_check: %zu sets, %lld edges scanned, %lld CSR entries placed, node capacity %d (LDS %d of %d bytes): ok\n", sets.size(),
                g_edges, g_entries, cap, nr_lds_carve(cap).bytes, NR_LDS_BYTES);
    return 0;
}
