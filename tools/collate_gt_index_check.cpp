// collate_gt_index_check.cpp -- host check of csrc/collate_gt_index.h, the only place dr_blend_flow_knn3_f32 and dr_coarse_gt_matches_f32
// compute an index.  Build and run, on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/collate_gt_index_check.cpp \
//         -o /tmp/collate_gt_index_check && /tmp/collate_gt_index_check
//
// For ragged batches of P = 1 .. 5 pairs with clouds of 0, 1, 2, 3, 63, 64, 65, CG_BLOCK +- 1, CG_STAGE +- 1 and 2 CG_STAGE + 5 points it walks
// the launch as the kernels do: every workgroup of the grid bound maps to (pair, tile) or to nothing, every tile of every pair is reached exactly
// once, every query row a thread would touch and every reference row a stage would load is read from real allocations of exactly the stacked
// size (AddressSanitizer guards their ends), the stages of a cloud tile it without gap or overlap, and the compaction's output rows stay inside
// the pair's slice.  Offsets that do not describe a slice (negative, decreasing, past the end) make the pair empty and are never dereferenced.
// The workspace carve is checked for order, alignment and size.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "collate_gt_index.h"

using namespace dr;

static long long g_rows = 0;
static bool g_disjoint = true;      // the pairs' slices do not overlap (false for the decreasing-offset case, whose neighbours share rows)

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "collate_gt_index_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

// one launch: queries at q_off over nq rows, references at r_off over nr rows
static void walk(const std::vector<int32_t>& q_off, int nq, const std::vector<int32_t>& r_off, int nr) {
    const int P = (int)q_off.size() - 1;
    std::vector<float> query((size_t)nq * 3, 1.f), ref((size_t)nr * 3, 2.f), out((size_t)nq * 3, 0.f);
    std::vector<int> seen((size_t)nq, 0);
    std::vector<std::vector<int>> tiles_seen(P);
    for (int p = 0; p < P; ++p) tiles_seen[p].assign(cg_tiles(cg_slice_ok(q_off[p], q_off[p + 1], nq) ? q_off[p + 1] - q_off[p] : 0), 0);
    const long long grid = cg_grid_bound(nq, P);
    long long mapped = 0;
    volatile float sink = 0.f;
    for (long long b = 0; b < grid; ++b) {
        int pair = -1, tile = -1;
        if (!cg_tile_to_pair(P, q_off.data(), nq, b, pair, tile)) continue;
        ++mapped;
        CHECK(pair >= 0 && pair < P && tile >= 0 && tile < (int)tiles_seen[pair].size());
        CHECK(tiles_seen[pair][tile]++ == 0);
        const int q0 = q_off[pair], q1 = q_off[pair + 1], r0 = r_off[pair], r1 = r_off[pair + 1];
        if (!cg_slice_ok(q0, q1, nq) || !cg_slice_ok(r0, r1, nr)) continue;          // status bit 1: nothing is read
        const int Q = q1 - q0, K = r1 - r0;
        int covered = 0;
        for (int k0 = 0; k0 < K; k0 += CG_STAGE) {                                    // the staging loop of one workgroup
            const int nk = cg_stage_count(K, k0);
            CHECK(nk >= 1 && nk <= CG_STAGE && k0 + nk <= K);
            for (int t = 0; t < CG_BLOCK; ++t)
                for (int k = t; k < nk; k += CG_BLOCK) {
                    const float* p = ref.data() + (size_t)(r0 + k0 + k) * 3;
                    sink = sink + p[0] + p[1] + p[2];
                    ++g_rows;
                }
            covered += nk;
        }
        CHECK(covered == K && cg_stage_count(K, K) == 0);
        for (int t = 0; t < CG_BLOCK; ++t) {
            const int q = tile * CG_BLOCK + t;
            if (q >= Q) continue;
            const float* p = query.data() + (size_t)(q0 + q) * 3;
            sink = sink + p[0] + p[1] + p[2];
            float* o = out.data() + (size_t)(q0 + q) * 3;
            o[0] = o[1] = o[2] = 1.f;
            CHECK(seen[(size_t)(q0 + q)]++ == 0 || !g_disjoint);
            // the compaction writes rank <= q of the pair at row q0 + rank: inside the pair's slice of the [nq] outputs
            CHECK(q0 + q < q1);
        }
    }
    for (int p = 0; p < P; ++p) {
        for (int s : tiles_seen[p]) CHECK(s == 1);
        if (cg_slice_ok(q_off[p], q_off[p + 1], nq) && cg_slice_ok(r_off[p], r_off[p + 1], nr))
            for (int i = q_off[p]; i < q_off[p + 1]; ++i) CHECK(seen[(size_t)i] == 1 || (!g_disjoint && seen[(size_t)i] > 1));
    }
    long long want = 0;
    for (int p = 0; p < P; ++p) want += (long long)tiles_seen[p].size();
    CHECK(mapped == want && want <= grid);
    (void)sink;
}

static std::vector<int32_t> prefix(const std::vector<int>& n) {
    std::vector<int32_t> o(n.size() + 1, 0);
    for (size_t i = 0; i < n.size(); ++i) o[i + 1] = o[i] + n[i];
    return o;
}

int main() {
    const int sizes[] = {0, 1, 2, 3, 4, 63, 64, 65, CG_BLOCK - 1, CG_BLOCK, CG_BLOCK + 1, CG_STAGE - 1, CG_STAGE, CG_STAGE + 1, 2 * CG_STAGE + 5};
    const int S = (int)(sizeof(sizes) / sizeof(sizes[0]));
    // single pairs: every query size against every reference size
    for (int a = 0; a < S; ++a)
        for (int b = 0; b < S; ++b) walk(prefix({sizes[a]}), sizes[a], prefix({sizes[b]}), sizes[b]);
    // ragged batches: sliding windows of 2 .. 5 sizes, queries and references out of step
    for (int P = 2; P <= 5; ++P)
        for (int a = 0; a + P <= S; ++a)
            for (int b = 0; b + P <= S; b += 3) {
                std::vector<int> nq(sizes + a, sizes + a + P), nr(sizes + b, sizes + b + P);
                const std::vector<int32_t> qo = prefix(nq), ro = prefix(nr);
                walk(qo, qo.back(), ro, ro.back());
                // the stacked arrays may be longer than the last offset
                walk(qo, qo.back() + 7, ro, ro.back() + 3);
            }
    // offsets that do not describe a slice: the pair is empty (one tile), nothing of it is dereferenced, its neighbours are walked as usual
    {
        const std::vector<int32_t> good = prefix({65, 130, 3});
        std::vector<int32_t> bad = good;
        bad[2] = bad[1] - 4;                                   // decreasing
        g_disjoint = false;
        walk(bad, good.back(), good, good.back());
        g_disjoint = true;
        walk(good, good.back(), bad, good.back());
        bad = good;
        bad[3] = good.back() + 1000;                           // past the end
        walk(bad, good.back(), good, good.back());
        bad = good;
        bad[0] = -5;                                           // negative
        walk(bad, good.back(), good, good.back());
        CHECK(!cg_slice_ok(-1, 3, 10) && !cg_slice_ok(4, 3, 10) && !cg_slice_ok(0, 11, 10) && cg_slice_ok(0, 0, 0) && cg_slice_ok(10, 10, 10));
    }
    // the grid bound at the int limits
    CHECK(cg_grid_bound(0x7fffffff / 3, 64) < 0x7fffffffLL && cg_grid_bound(-1, 3) == 3 && cg_tiles(0) == 1 && cg_tiles(CG_BLOCK + 1) == 2);
    // the workspace carve: three arrays in order, each on 256 bytes, none overlapping, the total covering the last
    const int carve[][2] = {{0, 0}, {1, 1}, {63, 65}, {64, 64}, {65, 63}, {1025, 2}, {2, 1025}, {715827882, 715827882}};
    for (const auto& c : carve) {
        const CgMatchCarve k = cg_match_carve(c[0], c[1]);
        CHECK(k.nn_st == 0 && k.nn_st % 256 == 0 && k.d2_st % 256 == 0 && k.nn_ts % 256 == 0);
        CHECK(k.d2_st >= k.nn_st + (size_t)c[0] * 4 && k.nn_ts >= k.d2_st + (size_t)c[0] * 4 && k.bytes >= k.nn_ts + (size_t)c[1] * 4);
        if (c[0] <= 2048) {
            std::vector<char> ws(k.bytes + 1);
            for (int i = 0; i < c[0]; ++i) {
                ((int32_t*)(ws.data() + k.nn_st))[i] = i;
                ((float*)(ws.data() + k.d2_st))[i] = 1.f;
            }
            for (int i = 0; i < c[1]; ++i) ((int32_t*)(ws.data() + k.nn_ts))[i] = i;
            for (int i = 0; i < c[0]; ++i) CHECK(((int32_t*)(ws.data() + k.nn_st))[i] == i);
        }
    }
    CHECK(cg_match_carve(-4, -4).bytes == 0);
    std::printf("collate_gt_index_check ok: %lld reference rows walked\n", g_rows);
    return 0;
}
