// knn_index_check.cpp -- host check of csrc/knn_index.h, the only place the non-rigid evaluation kernels (csrc/knn_points.hip) compute an index.
// Build and run, on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/knn_index_check.cpp \
//         -o /tmp/knn_index_check && /tmp/knn_index_check
//
// It walks, as the kernels do and on real allocations of exactly the sizes the entries are given (AddressSanitizer guards their ends):
//   * the ragged offsets: flat workgroup -> (pair, block) covers every block of every pair exactly once inside the grid bound, a bad slice
//     counts as empty, the first flat block of a pair is where its blocks start;
//   * the staging of every tile: each of the KNN_TILE entries is written exactly once, an entry behind the count reads row 0 of the tile;
//     every coordinate read lies inside the pair's supports;
//   * the quarters: the four waves' walks are disjoint, stay inside their quarter and the LDS tile, and together cover the tile's count;
//     every support of the pair is visited exactly once, in ascending index inside a wave;
//   * the merge rows of waves 1 .. 3 for K = 1, 4, 8, 16: disjoint, inside KNN_LDS_WORDS;
//   * the outputs [rows, k] and the partial rows of both reductions inside their workspaces;
// for Q, S in {0, 1, block - 1, block, block + 1, tile - 1, tile, tile + 1, 2 tile + 1}, alone and in ragged batches.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "knn_index.h"

using namespace dr;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

static long long g_reads = 0;

static void walk_supports(const std::vector<float>& s, int slo, int S) {
    const float* sp = s.data() + knn_coord(slo, 0, 0);
    std::vector<int> seen((size_t)S, 0);
    std::vector<float> lds(KNN_LDS_WORDS);
    CHECK(knn_tiles(S) == (S + KNN_TILE - 1) / KNN_TILE);
    for (int t = 0; t < knn_tiles(S); ++t) {
        const int count = knn_tile_count(S, t);
        CHECK(count >= 1 && count <= KNN_TILE && knn_support_of(t, 0) + count <= S);
        std::vector<int> written(KNN_TILE, 0);
        for (int tid = 0; tid < KNN_THREADS; ++tid)
            for (int e = tid; e < KNN_TILE; e += KNN_THREADS) {
                const bool in = e < count;
                const int r = knn_support_of(t, in ? e : 0);
                CHECK(r >= 0 && r < S);
                for (int c = 0; c < 3; ++c) {
                    lds[knn_lds_coord(c, e)] = sp[knn_local_coord(r, c)];
                    ++g_reads;
                }
                ++written[e];
            }
        for (int v : written) CHECK(v == 1);
        int covered = 0;
        for (int w = 0; w < KNN_WAVES; ++w) {
            const int e0 = knn_quarter_first(w), walk = knn_quarter_walk(count, w);
            CHECK(walk % KNN_VEC == 0 && walk >= 0 && walk <= KNN_QUARTER && e0 + walk <= KNN_TILE);
            int last = -1;
            for (int j = 0; j < walk; j += KNN_VEC)
                for (int c = 0; c < 3; ++c) {
                    CHECK((knn_lds_coord(c, e0 + j) % KNN_VEC) == 0);                   // the 16-byte read is aligned
                    for (int v = 0; v < KNN_VEC; ++v) {
                        volatile float x = lds[knn_lds_coord(c, e0 + j + v)];
                        (void)x;
                    }
                }
            for (int j = 0; j < walk; ++j) {
                const int e = e0 + j;
                if (e < count) {
                    const int i = knn_support_of(t, e);
                    CHECK(i > last);
                    last = i;
                    ++seen[i];
                    ++covered;
                }
            }
        }
        CHECK(covered == count);
    }
    for (int v : seen) CHECK(v == 1);
}

static void walk_batch(const std::vector<int>& ql, const std::vector<int>& sl, int k) {
    const int P = (int)ql.size();
    CHECK((int)sl.size() == P);
    std::vector<int32_t> qo(P + 1, 0), so(P + 1, 0);
    for (int p = 0; p < P; ++p) { qo[p + 1] = qo[p] + ql[p]; so[p + 1] = so[p] + sl[p]; }
    const int nq = qo[P], ns = so[P];
    std::vector<float> q((size_t)nq * 3, 1.0f), s((size_t)ns * 3, 2.0f), dist((size_t)nq * k);
    std::vector<long long> idx((size_t)nq * k);
    const long long grid = knn_grid_bound(nq, P, KNN_BLOCK);
    const size_t wsb = nn_stats_workspace_bytes(P, nq);
    CHECK(wsb >= (size_t)grid * NN_SLOTS * sizeof(double));
    std::vector<double> partials((size_t)grid * NN_SLOTS);
    std::vector<int> rows_seen((size_t)nq, 0);
    long long used = 0;
    for (long long b = 0; b < grid; ++b) {
        int p, block;
        if (!knn_block_to_pair(P, qo.data(), nq, KNN_BLOCK, b, p, block)) continue;
        ++used;
        CHECK(p >= 0 && p < P && block >= 0 && block < knn_blocks(ql[p], KNN_BLOCK));
        CHECK(knn_first_block(p, qo.data(), nq, KNN_BLOCK) + block == b);
        for (int lane = 0; lane < KNN_WAVE; ++lane) {
            const int qi = knn_query_of(block, lane);
            if (qi >= ql[p]) continue;
            volatile float v = q[knn_coord(qo[p], 0, 0) + knn_local_coord(qi, 0)] + q[knn_coord(qo[p], 0, 0) + knn_local_coord(qi, 2)];
            (void)v;
            const size_t row = knn_row(qo[p], qi);
            ++rows_seen[row];
            for (int j = 0; j < k; ++j) {
                dist[knn_out(row, k, j)] = 0.0f;
                idx[knn_out(row, k, j)] = j;
            }
        }
        for (int sl_ = 0; sl_ < NN_SLOTS; ++sl_) partials[knn_partial(b, NN_SLOTS, sl_)] = 1.0;
    }
    long long want = 0;
    for (int p = 0; p < P; ++p) want += knn_blocks(ql[p], KNN_BLOCK);
    CHECK(used == want && want <= grid);
    for (int v : rows_seen) CHECK(v == 1);
    for (int p = 0; p < P; ++p)
        if (sl[p] > 0) walk_supports(s, so[p], sl[p]);
    // the flow metrics over the query rows: one point per thread, FLOW_BLOCK per workgroup
    const long long fgrid = knn_grid_bound(nq, P, FLOW_BLOCK);
    CHECK(flow_metrics_workspace_bytes(P, nq) >= (size_t)fgrid * FLOW_SLOTS * sizeof(double));
    std::vector<double> fpart((size_t)fgrid * FLOW_SLOTS);
    std::vector<int> fseen((size_t)nq, 0);
    for (long long b = 0; b < fgrid; ++b) {
        int p, block;
        if (!knn_block_to_pair(P, qo.data(), nq, FLOW_BLOCK, b, p, block)) continue;
        for (int tid = 0; tid < FLOW_BLOCK; ++tid) {
            const int i = block * FLOW_BLOCK + tid;
            if (i < ql[p]) {
                volatile float v = q[knn_coord(qo[p], i, 2)];
                (void)v;
                ++fseen[knn_row(qo[p], i)];
            }
        }
        for (int sl_ = 0; sl_ < FLOW_SLOTS; ++sl_) fpart[knn_partial(b, FLOW_SLOTS, sl_)] = 1.0;
    }
    for (int v : fseen) CHECK(v == 1);
}

int main() {
    CHECK(KNN_THREADS == KNN_WAVES * KNN_WAVE && KNN_BLOCK == KNN_WAVE && KNN_TILE == KNN_WAVES * KNN_QUARTER && KNN_QUARTER % KNN_VEC == 0);
    CHECK(KNN_TILE % KNN_THREADS == 0 && KNN_LDS_WORDS >= KNN_TILE_WORDS && KNN_LDS_WORDS >= KNN_MERGE_WORDS);
    for (int k = 0; k <= KNN_MAX_K + 1; ++k) {
        const int K = knn_width(k);
        CHECK((k < 1 || k > KNN_MAX_K) ? K == 0 : (K >= k && (K == 1 || K == 4 || K == 8 || K == 16)));
    }
    for (int K : {1, 4, 8, 16}) {
        std::vector<int> words(KNN_LDS_WORDS, 0);
        for (int plane = 0; plane < 2; ++plane)
            for (int w = 1; w < KNN_WAVES; ++w)
                for (int j = 0; j < K; ++j)
                    for (int lane = 0; lane < KNN_WAVE; ++lane) {
                        const int a = knn_merge_word(K, plane, w, j, lane);
                        CHECK(a >= 0 && a < KNN_LDS_WORDS);
                        ++words[a];
                    }
        for (int v : words) CHECK(v <= 1);
    }
    std::vector<int> fl(FLOW_LDS_WORDS, 0);
    for (int w = 0; w < FLOW_BLOCK / KNN_WAVE; ++w)
        for (int s = 0; s < FLOW_SLOTS; ++s) ++fl[flow_lds_word(w, s)];
    for (int v : fl) CHECK(v == 1);
    const int B = KNN_BLOCK, T = KNN_TILE;
    const int sizes[] = {0, 1, B - 1, B, B + 1, T - 1, T, T + 1, 2 * T + 1};
    for (int Q : sizes)
        for (int S : sizes)
            for (int k : {1, 5, 16}) walk_batch({Q}, {S}, k);
    walk_batch({B + 1, 0, 3}, {T + 1, 0, 2}, 3);
    walk_batch({0, 0, 7}, {5, 0, 0}, 4);
    walk_batch({2 * T + 1, 1, B}, {1, 2 * T + 1, B - 1}, 16);
    // offsets that are no slices: the pair counts as empty and nothing of it is walked
    {
        const int32_t off[] = {0, 70, 60, 100};
        int p, block;
        CHECK(!nr_slice_ok(off[1], off[2], 100));
        CHECK(knn_block_to_pair(3, off, 100, KNN_BLOCK, 2, p, block) && p == 2 && block == 0);
        CHECK(knn_first_block(2, off, 100, KNN_BLOCK) == 2);
        CHECK(!knn_block_to_pair(3, off, 100, KNN_BLOCK, 3, p, block));
    }
    std::printf("knn_index_check: ok (%lld coordinate reads walked)\n", g_reads);
    return 0;
}
