// lgr_index_check.cpp -- host check of csrc/lgr_index.h, the only place the rigid estimators' kernels (csrc/lgr.hip) compute an index.
// Stand-alone; built with the sanitizers and run on the host:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/lgr_index_check.cpp \
//         -o /tmp/lgr_index_check && /tmp/lgr_index_check
//
// It allocates every array at exactly the size the entries document and walks every index expression of the kernels over the small shapes
// the tests use and over the capacity edges: an index outside its array is an ASan report, an overflow a UBSan report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __host__
#define __device__
#include "lgr_index.h"

using namespace dr;

static long long g_reads = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("lgr_index_check: FAILED %s (line %d)\n", #c, __LINE__); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

// the summation order: every element of a group is met exactly once, by the slot (i / 64 % 4, i % 64), whichever team size serves it
static void walk_sum(int n) {
    std::vector<int> seen(n > 0 ? n : 0, 0);
    for (int nw : {1, LGR_VWAVES})
        for (int w = 0; w < nw; ++w)
            for (int v = 0; v < LGR_VWAVES; ++v) {
                if (!lgr_team_serves(w, nw, v)) continue;
                for (int lane = 0; lane < LGR_WAVE; ++lane) {
                    int met = 0;
                    for (int i = lgr_slot_first(v, lane); i < n; i += LGR_STRIDE) {
                        CHECK(i / LGR_WAVE % LGR_VWAVES == v && i % LGR_WAVE == lane);
                        seen[i] += 1;
                        ++met;
                        ++g_reads;
                    }
                    CHECK(met == lgr_slot_count(n, v, lane));
                }
            }
    for (int i = 0; i < n; ++i) CHECK(seen[i] == 2);             // once per team size
    std::vector<double> ex(LGR_EXCHANGE_WORDS);
    for (int N : {1, 7, 9})
        for (int v = 0; v < LGR_VWAVES; ++v)
            for (int k = 0; k < N; ++k) ex[lgr_exchange_word(N, v, k)] = 1.0;
}

// the fit's grid over G groups under `off`: every group is served once, its rows lie inside the stacked arrays, its transform inside [G, 16]
static void walk_fit(const std::vector<int32_t>& off, int n, int wave_limit) {
    const long long G = (long long)off.size() - 1;
    std::vector<float> pts((size_t)n * 3), T((size_t)G * 16);
    std::vector<int> served(G, 0);
    for (long long b = 0; b < lgr_fit_blocks(G); ++b)
        for (int s = 0; s < LGR_GROUPS_PER_BLOCK; ++s) {
            const long long g = lgr_fit_group(b, s);
            if (g >= G) break;
            served[g] += 1;
            const int lo = off[g], hi = off[g + 1];
            if (!nr_slice_ok(lo, hi, n)) continue;
            (void)lgr_uses_wave(hi - lo, wave_limit);
            for (int i = 0; i < hi - lo; ++i)
                for (int c = 0; c < 3; ++c) {
                    pts[knn_coord(lo, 0, 0) + knn_local_coord(i, c)] = 0.0f;
                    ++g_reads;
                }
            for (int k = 0; k < 16; ++k) T[lgr_transform_word(g, k)] = 0.0f;
        }
    for (long long g = 0; g < G; ++g) CHECK(served[g] == 1);
}

// the chunk scan of one call: the lists of every usable problem stay inside its slice, the dense list inside [n_corr]
static void walk_lgr(const std::vector<int32_t>& off, const std::vector<int32_t>& ids, int min_local) {
    const int P = (int)off.size() - 1, n = (int)ids.size();
    const LgrCarve c = lgr_carve(P, n);
    std::vector<char> ws(c.total);
    CHECK(c.starts % 256 == 0 && c.chunk_lo % 256 == 0 && c.transforms % 256 == 0 && c.transforms + (size_t)n * 64 <= c.total);
    int32_t* starts = (int32_t*)(ws.data() + c.starts);
    int32_t* clo = (int32_t*)(ws.data() + c.chunk_lo);
    int32_t* chi = (int32_t*)(ws.data() + c.chunk_hi);
    int32_t* nch = (int32_t*)(ws.data() + c.n_chunks);
    int32_t* coff = (int32_t*)(ws.data() + c.chunk_off);
    int32_t* dlo = (int32_t*)(ws.data() + c.dense_lo);
    int32_t* dp = (int32_t*)(ws.data() + c.dense_p);
    int32_t* counts = (int32_t*)(ws.data() + c.counts);
    float* T = (float*)(ws.data() + c.transforms);
    int acc = 0;
    for (int p = 0; p < P; ++p) {
        nch[p] = 0;
        coff[p] = acc;
        if (!lgr_prefix_ok(off.data(), p, n)) continue;
        const int lo = off[p], nc = off[p + 1] - lo;
        int runs = 0;
        for (int i = 0; i < nc; ++i)
            if (lgr_is_run_start(ids.data() + knn_row(lo, 0), i)) starts[lgr_list_slot(lo, runs++)] = i;
        for (int r = 0; r < runs; ++r) {
            const int s = starts[lgr_list_slot(lo, r)], e = r + 1 < runs ? starts[lgr_list_slot(lo, r + 1)] : nc;
            if (e - s >= min_local) {
                clo[lgr_list_slot(lo, nch[p])] = lo + s;
                chi[lgr_list_slot(lo, nch[p])] = lo + e;
                nch[p] += 1;
            }
            g_reads += e - s;
        }
        for (int j = 0; j < nch[p]; ++j) {
            dlo[acc + j] = clo[lgr_list_slot(lo, j)];
            dp[acc + j] = p;
            counts[acc + j] = 0;
            for (int k = 0; k < 16; ++k) T[lgr_transform_word(acc + j, k)] = 0.0f;
        }
        acc += nch[p];
    }
    coff[P] = acc;
    CHECK(acc <= lgr_chunk_bound(n, min_local));
    CHECK(lgr_fit_blocks(lgr_chunk_bound(n, min_local)) * LGR_GROUPS_PER_BLOCK >= acc);
}

// the row sums and the dense matrix of one problem of Q queries and S supports
static void walk_sc(int Q, int S) {
    std::vector<float> lds(SC_LDS_WORDS), q((size_t)Q * 3), s((size_t)S * 3), out(Q), mat((size_t)Q * S);
    const int32_t qo[2] = {0, Q};
    const long long grid = knn_grid_bound(Q, 1, SC_BLOCK);
    std::vector<int> rows(Q, 0);
    for (long long b = 0; b < grid; ++b) {
        int p, block;
        if (!knn_block_to_pair(1, qo, Q, SC_BLOCK, b, p, block)) continue;
        for (int lane = 0; lane < SC_BLOCK; ++lane) {
            const int qi = sc_query_of(block, lane);
            if (qi < Q) {
                q[knn_coord(0, qi, 2)] = 0.0f;
                out[knn_row(0, qi)] = 0.0f;
                rows[qi] += 1;
            }
        }
        int total = 0;
        for (int t = 0; t < sc_tiles(S); ++t) {
            const int count = sc_tile_count(S, t);
            for (int e = 0; e < count; ++e) {
                const int r = sc_support_of(t, e);
                s[knn_local_coord(r, 2)] = 0.0f;
                for (int c = 0; c < SC_PLANES; ++c) lds[sc_lds_word(c, e)] = 0.0f;
                ++g_reads;
            }
            total += count;
        }
        CHECK(total == S);
        const int nr = sc_block_rows(Q, block);
        for (long long e = 0; e < (long long)nr * S; ++e) {
            const int r = (int)(e / S), j = (int)(e - (long long)r * S);
            mat[sc_dense_at(0, S, sc_query_of(block, r), j)] = 0.0f;
        }
    }
    for (int i = 0; i < Q; ++i) CHECK(rows[i] == 1);
    const EigCarve c = eig_carve(3, Q);
    CHECK(c.done >= (size_t)Q * 4 && c.total >= c.done + 12 && c.y % 256 == 0 && c.done % 256 == 0);
    for (int b = 0; b < knn_blocks(Q, EIG_ROWS_PER_BLOCK); ++b)
        for (int w = 0; w < EIG_ROWS_PER_BLOCK; ++w)
            if (eig_row_of(b, w) < Q) out[eig_row_of(b, w)] = 0.0f;
}

int main() {
    for (int n : {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099}) walk_sum(n);
    // groups of every length the tests use, G = 1 and G beyond one workgroup's four; bad groups among them
    walk_fit({0, 5}, 5, LGR_WAVE_LIMIT);
    {
        std::vector<int32_t> off = {0};
        for (int len : {1, 2, 3, 63, 64, 65, LGR_WAVE_LIMIT, LGR_WAVE_LIMIT + 1, 0, 700}) off.push_back(off.back() + len);
        for (int limit : {0, LGR_WAVE_LIMIT, 1 << 30}) walk_fit(off, off.back(), limit);
        std::vector<int32_t> bad = off;
        bad[3] = -4;
        bad[5] = off.back() + 9;
        walk_fit(bad, off.back(), LGR_WAVE_LIMIT);
    }
    // chunk scans: runs on both sides of min_local and of the wave, empty problems, a problem behind bad offsets, min_local = 1 (capacity edge)
    for (int min_local : {1, 2, 3, 4}) {
        std::vector<int32_t> ids, off = {0};
        int id = 0;
        for (int len : {2, 3, 4, 1, 63, 64, 65, 300}) {
            for (int i = 0; i < len; ++i) ids.push_back(id);
            ++id;
            if (len == 4 || len == 65) off.push_back((int32_t)ids.size());
        }
        off.push_back((int32_t)ids.size());
        off.push_back((int32_t)ids.size());                      // an empty problem
        walk_lgr(off, ids, min_local);
        std::vector<int32_t> every(ids.size());
        for (size_t i = 0; i < every.size(); ++i) every[i] = (int32_t)i;     // every row a run of its own
        walk_lgr(off, every, min_local);
        std::vector<int32_t> bad = off;
        bad[2] = bad[1] - 1;                                     // descending: this problem and every later one are skipped
        walk_lgr(bad, ids, min_local);
        walk_lgr({0, 0}, {}, min_local);
    }
    for (int Q : {1, SC_BLOCK - 1, SC_BLOCK, SC_BLOCK + 1, 2 * SC_TILE + 3})
        for (int S : {1, SC_TILE - 1, SC_TILE, SC_TILE + 1, 2 * SC_TILE + 3}) walk_sc(Q, S);
    CHECK(lgr_carve(0, 100).total == 0 && eig_carve(0, 10).total == 0);
    CHECK(lgr_carve(65535, INT32_MAX / 16).total > 0);
    std::printf("lgr_index_check: ok (%lld element visits walked)\n", g_reads);
    return 0;
}
