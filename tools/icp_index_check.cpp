// icp_index_check.cpp -- host check of csrc/icp_index.h, the only place the point-to-point ICP kernels (csrc/icp.hip) compute an index.
// Stand-alone; built with the sanitizers and run on the host:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/icp_index_check.cpp \
//         -o /tmp/icp_index_check && /tmp/icp_index_check
//
// It allocates every array at exactly the size the entry documents (the workspace at dr_icp_p2p_workspace_bytes' carve) and walks every
// index expression of the kernels -- the block table, the rows of a wave, the partial slots, the exchange words, the nine runs of the target
// grid -- over small and edge sizes: an index outside its array is an ASan report, an overflow a UBSan report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __host__
#define __device__
#include "icp_index.h"

using namespace dr;

static long long g_visits = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("icp_index_check: FAILED %s (line %d)\n", #c, __LINE__); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

// one call: pairs under s_off / t_off (possibly bad), ns / nt stacked rows
static void walk(const std::vector<int32_t>& s_off, const std::vector<int32_t>& t_off, int ns, int nt) {
    const int P = (int)s_off.size() - 1;
    const IcpCarve c = icp_carve(P, ns, nt);
    std::vector<char> ws(c.bytes);
    for (size_t at : {c.origin, c.keys, c.vals, c.sorted, c.partial, c.done}) CHECK(at % 256 == 0 && at <= c.bytes);
    const int n_pad = nt > 0 ? next_pow2(nt) : 0;
    float* origin = (float*)(ws.data() + c.origin);
    unsigned long long* keys = (unsigned long long*)(ws.data() + c.keys);
    uint32_t* vals = (uint32_t*)(ws.data() + c.vals);
    float* sorted = (float*)(ws.data() + c.sorted);
    double* partial = (double*)(ws.data() + c.partial);
    int32_t* done = (int32_t*)(ws.data() + c.done);
    std::vector<float> src((size_t)ns * 3, 0.25f), tgt((size_t)nt * 3, 0.5f), T((size_t)P * 16), fit(P), rmse(P);
    std::vector<int32_t> corr(ns, -2), status(P), its(P);
    // set-up: one workgroup per pair
    for (int p = 0; p < P; ++p) {
        status[p] = (lgr_prefix_ok(s_off.data(), p, ns) && lgr_prefix_ok(t_off.data(), p, nt)) ? 0 : ICP_ST_OFFSETS;
        done[p] = 0;
        for (int k = 0; k < 4; ++k) origin[4 * p + k] = 0.0f;
        if (status[p]) continue;
        for (int i = 0; i < s_off[p + 1] - s_off[p]; ++i) src[knn_coord(s_off[p], i, 2)] += 0.0f;
        for (int i = 0; i < t_off[p + 1] - t_off[p]; ++i) tgt[knn_coord(t_off[p], i, 2)] += 0.0f;
        for (int k = 0; k < 16; ++k) T[lgr_transform_word(p, k)] = 0.0f;
    }
    // the grid: a key per padded row, the gathered rows
    for (int i = 0; i < n_pad; ++i) {
        vals[i] = (uint32_t)i;
        const int p = i < nt ? it3_pair_of(P, t_off.data(), nt, i) : P;
        keys[i] = i >= nt ? IT3_PAD_KEY : it3_key(p, it3_cell(tgt[(size_t)i * 3], 0.0f, 0.1f), 0, IT3_CELL_MAX);
    }
    std::sort(keys, keys + n_pad);
    for (int i = 0; i < nt; ++i) sorted[4 * (size_t)i + 3] = 0.0f;
    // (A): every block of the launched grid
    const long long grid = icp_grid(ns, P);
    CHECK(c.bytes == 0 || c.partial + (size_t)grid * ICP_SLOTS * sizeof(double) <= c.done);
    std::vector<double> ex(ICP_LDS_WORDS);
    std::vector<int> met(ns, 0);
    long long used = 0;
    for (long long b = 0; b < grid; ++b) {
        int p, block;
        if (!knn_block_to_pair(P, s_off.data(), ns, ICP_BLOCK_ROWS, b, p, block)) continue;
        ++used;
        CHECK(b == knn_first_block(p, s_off.data(), ns, ICP_BLOCK_ROWS) + block);
        if (status[p] & ICP_ST_SKIP) continue;
        const int s0 = s_off[p], n_src = s_off[p + 1] - s0, t0 = t_off[p], n_tgt = t_off[p + 1] - t0;
        for (int w = 0; w < ICP_WAVES; ++w) {
            for (int j = 0; j < ICP_ROWS_PER_WAVE; ++j) {
                const int i = icp_row_of(block, w, j);
                if (i >= n_src) break;
                met[knn_row(s0, i)] += 1;
                src[knn_coord(s0, i, 2)] += 0.0f;
                corr[knn_row(s0, i)] = -1;
                if (n_tgt > 0) {
                    for (int cx : {0, 7, IT3_CELL_MAX})
                        for (int r = 0; r < 9; ++r) {
                            unsigned long long first = 0, last = 0;
                            if (!it3_run_keys(p, cx, cx, IT3_CELL_MAX - cx, r, first, last)) continue;
                            const int lo = it3_lower_bound(keys, 0, nt, first), hi = it3_lower_bound(keys, 0, nt, last + 1);
                            CHECK(lo >= 0 && hi >= lo && hi <= nt);
                            for (int q = lo; q < hi; ++q) sorted[4 * (size_t)q + 3] += 0.0f;
                        }
                    tgt[knn_coord(t0, n_tgt - 1, 2)] += 0.0f;                          // the farthest partner a row can name
                }
                ++g_visits;
            }
            for (int k = 0; k < ICP_SLOTS; ++k) ex[icp_exchange_word(w, k)] = 0.0;
        }
        for (int k = 0; k < ICP_SLOTS; ++k) partial[knn_partial(b, ICP_SLOTS, k)] = 1.0;
    }
    // (B): one wave per pair adds the pair's partials
    long long blocks_total = 0;
    for (int p = 0; p < P; ++p) {
        if (status[p] & ICP_ST_SKIP) continue;
        const int n_src = s_off[p + 1] - s_off[p];
        const long long first = knn_first_block(p, s_off.data(), ns, ICP_BLOCK_ROWS);
        const int blocks = knn_blocks(n_src, ICP_BLOCK_ROWS);
        double s = 0.0;
        for (int k = 0; k < ICP_SLOTS; ++k)
            for (int b = 0; b < blocks; ++b) s += partial[knn_partial(first + b, ICP_SLOTS, k)];
        CHECK(s == (double)blocks * ICP_SLOTS);                                        // every slot of the pair was written by (A)
        blocks_total += blocks;
        fit[p] = rmse[p] = 0.0f;
        its[p] = 0;
        done[p] = 1;
    }
    CHECK(blocks_total <= used && used <= grid);
    for (int p = 0; p < P; ++p)
        if (!(status[p] & ICP_ST_SKIP))
            for (int i = s_off[p]; i < s_off[p + 1]; ++i) CHECK(met[i] == 1);
}

int main() {
    for (int ns : {0, 1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257, 1025})
        for (int nt : {0, 1, 64, 65, 1025}) walk({0, ns}, {0, nt}, ns, nt);
    // three pairs: an empty source, an empty target, a normal pair; then rows in front of the first pair and behind the last
    walk({0, 0, 70, 200}, {0, 90, 90, 300}, 200, 300);
    walk({5, 5, 70, 190}, {3, 90, 90, 280}, 200, 300);
    // offsets that are no slices: descending, negative, past the end -- the pair and (by the prefix rule) every later pair is skipped
    walk({0, 80, 60, 200}, {0, 90, 100, 300}, 200, 300);
    walk({-4, 80, 120, 200}, {0, 90, 100, 300}, 200, 300);
    walk({0, 80, 120, 260}, {0, 90, 100, 300}, 200, 300);
    walk({0, 80, 120, 200}, {0, 90, 100, 301}, 200, 300);
    // many short pairs: the grid bound ns / 64 + P holds when every pair rounds up
    {
        std::vector<int32_t> so = {0}, to = {0};
        for (int p = 0; p < 100; ++p) { so.push_back(so.back() + 1 + p % 3); to.push_back(to.back() + p % 2); }
        walk(so, to, so.back(), to.back());
    }
    CHECK(icp_carve(0, 10, 10).bytes == 0);
    CHECK(icp_carve(ICP_MAX_PAIRS, INT32_MAX / 3, INT32_MAX / 3).bytes > (size_t)(INT32_MAX / 3) * 16);
    CHECK(icp_grid(INT32_MAX / 3, ICP_MAX_PAIRS) < 0xffffffffLL);
    std::printf("icp_index_check: ok (%lld row visits walked)\n", g_visits);
    return 0;
}
