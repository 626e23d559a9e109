// item3d_index_check.cpp -- host check of csrc/item3d_index.h, the only place dr_item3d_prepare_f32 and dr_radius_pairs_ragged_f32 compute an
// index.  Build and run, on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/item3d_index_check.cpp \
//         -o /tmp/item3d_index_check && /tmp/item3d_index_check
//
// For ragged batches of 1 .. 4 pairs with clouds of 0, 1, 3, 63, 64, 65, 255, 256, 257 and 300 points it walks the launches as the kernels do, on
// real allocations of exactly the stacked sizes (AddressSanitizer guards their ends): every output row maps to one pair or to none; a selection
// entry is read only inside the raw cloud; the nine runs of a row's sweep, searched over all sorted (pair, cell) keys, hold only targets of the row's pair (also when rows of
// no pair lie in front of offsets[0]), do not overlap, and together hold every target within one cell of the row on every axis (so every partner);
// the ranks of a row's partners are a permutation of 0 .. count - 1; every write of the pair list lands inside the pair's room and inside the
// list; offsets that do not describe a slice make the pair empty and are never dereferenced.  The cell coordinate is walked at the grid's ends,
// at NaN and at the float limits, the room and the count saturation at the int limits, and the workspace carve for order, alignment and size.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "item3d_index.h"

using namespace dr;

static long long g_tests = 0;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "item3d_index_check: %s failed at line %d\n", #c, __LINE__); \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

static std::vector<int32_t> prefix(const std::vector<int>& n) {
    std::vector<int32_t> o(n.size() + 1, 0);
    for (size_t i = 0; i < n.size(); ++i) o[i + 1] = o[i] + n[i];
    return o;
}

// the selection stage of one side: rows [off[p], off[p + 1]) read raw rows sel[row] of [raw_off[p], raw_off[p + 1])
static void walk_select(const std::vector<int32_t>& raw_off, const std::vector<int32_t>& off, const std::vector<long long>& sel) {
    const int P = (int)off.size() - 1, n = off.back() < 0 ? 0 : (int)sel.size(), n_raw = raw_off.back();
    std::vector<float> raw((size_t)std::max(n_raw, 0) * 3, 1.f), out((size_t)n * 3, 0.f);
    for (int row = 0; row < n; ++row) {
        const int p = it3_pair_of(P, off.data(), n, row);
        if (p >= P) continue;
        CHECK(row >= off[p] && row < off[p + 1]);
        const int lo = raw_off[p], hi = raw_off[p + 1];
        if (!it3_slice_ok(lo, hi, n_raw)) continue;
        const long long r = sel[row];
        if (!it3_sel_ok(r, hi - lo)) continue;
        const float* x = raw.data() + ((size_t)lo + (size_t)r) * 3;
        out[(size_t)row * 3] = x[0] + x[1] + x[2];
        ++g_tests;
    }
}

// the pair list of one batch with room `room[p]` per pair in a list of `capacity` rows
static void walk_pairs(const std::vector<int>& ns_, const std::vector<int>& nt_, float radius, const std::vector<long long>& room, long long capacity,
                       unsigned seed, float spread, int lead = 0) {
    const int P = (int)ns_.size();
    std::vector<int32_t> s_off = prefix(ns_), t_off = prefix(nt_);
    for (auto& o : s_off) o += lead;                           // `lead` rows of no pair in front of offsets[0], 3 behind the last
    for (auto& o : t_off) o += lead;
    const int ns = s_off.back() + (lead ? 3 : 0), nt = t_off.back() + (lead ? 3 : 0), n_pad = nt > 0 ? next_pow2(nt) : 0;
    CHECK(n_pad >= nt && (n_pad & (n_pad - 1)) == 0);
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(-spread, spread);
    std::vector<float> src((size_t)ns * 3), tgt((size_t)nt * 3);
    for (auto& v : src) v = U(rng) * 1.5f;                     // some sources lie outside the target's grid
    for (auto& v : tgt) v = U(rng);
    const float cell = radius * (1.0f + 1.0f / 128.0f), r2 = radius * radius;
    std::vector<float> origin((size_t)P * 3, std::numeric_limits<float>::infinity());
    for (int p = 0; p < P; ++p)
        for (int i = t_off[p]; i < t_off[p + 1]; ++i)
            for (int c = 0; c < 3; ++c) origin[(size_t)p * 3 + c] = std::fmin(origin[(size_t)p * 3 + c], tgt[(size_t)i * 3 + c]);
    std::vector<std::pair<unsigned long long, unsigned>> kv((size_t)n_pad);
    for (int i = 0; i < n_pad; ++i) {
        kv[i].second = (unsigned)i;
        if (i >= nt) { kv[i].first = IT3_PAD_KEY; continue; }
        const int p = it3_pair_of(P, t_off.data(), nt, i);
        CHECK(p < P || lead);
        if (p >= P) { kv[i].first = it3_key(P, 0, 0, 0); continue; }
        const float* o = origin.data() + (size_t)p * 3;
        kv[i].first = it3_key(p, it3_cell(tgt[(size_t)i * 3], o[0], cell), it3_cell(tgt[(size_t)i * 3 + 1], o[1], cell), it3_cell(tgt[(size_t)i * 3 + 2], o[2], cell));
        CHECK(kv[i].first < it3_key(p + 1, 0, 0, 0) && kv[i].first >= it3_key(p, 0, 0, 0));
    }
    std::sort(kv.begin(), kv.end());                           // ascending by (key, value): what the device sort leaves
    std::vector<unsigned long long> keys((size_t)n_pad);
    std::vector<unsigned> vals((size_t)n_pad);
    for (int i = 0; i < n_pad; ++i) { keys[i] = kv[i].first; vals[i] = kv[i].second; }
    for (int i = 0; i < nt; ++i) CHECK(vals[i] < (unsigned)nt);   // the real keys sort in front of the padding
    std::vector<long long> c_off((size_t)P + 1, 0);
    for (int p = 0; p < P; ++p) c_off[p + 1] = c_off[p] + room[p];
    std::vector<long long> out_src((size_t)capacity, -1), out_tgt((size_t)capacity, -1);
    for (int i = 0; i < ns; ++i) {
        const int p = it3_pair_of(P, s_off.data(), ns, i);
        CHECK(p < P || lead);
        if (p >= P) continue;
        const int t0 = t_off[p], t1 = t_off[p + 1];
        if (t1 <= t0) continue;
        const float* q = src.data() + (size_t)i * 3;
        const float* o = origin.data() + (size_t)p * 3;
        const int cx = it3_cell(q[0], o[0], cell), cy = it3_cell(q[1], o[1], cell), cz = it3_cell(q[2], o[2], cell);
        int lo[9], hi[9];
        int prev_hi = 0;
        for (int r = 0; r < 9; ++r) {
            unsigned long long first, last;
            lo[r] = hi[r] = 0;
            if (!it3_run_keys(p, cx, cy, cz, r, first, last)) continue;
            CHECK(first <= last);
            lo[r] = it3_lower_bound(keys.data(), 0, nt, first);               // over all sorted targets: the pair is in the key
            hi[r] = it3_lower_bound(keys.data(), 0, nt, last + 1);
            CHECK(lo[r] >= prev_hi && hi[r] >= lo[r] && hi[r] <= nt);        // inside the sorted targets, in order, no overlap
            prev_hi = hi[r];
        }
        // every partner (by the float32 predicate) is inside some run, and its key belongs to the pair
        std::vector<unsigned> hits;
        for (int r = 0; r < 9; ++r)
            for (int j = lo[r]; j < hi[r]; ++j) {
                const float* t = tgt.data() + (size_t)vals[j] * 3;
                const float dx = q[0] - t[0], dy = q[1] - t[1], dz = q[2] - t[2];
                CHECK(vals[j] >= (unsigned)t0 && vals[j] < (unsigned)t1);
                if (dx * dx + dy * dy + dz * dz < r2) hits.push_back(vals[j]);
                ++g_tests;
            }
        size_t brute = 0;
        for (int j = t0; j < t1; ++j) {
            const float* t = tgt.data() + (size_t)j * 3;
            const float dx = q[0] - t[0], dy = q[1] - t[1], dz = q[2] - t[2];
            brute += dx * dx + dy * dy + dz * dz < r2 ? 1 : 0;
        }
        CHECK(hits.size() == brute);
        // ranks: a permutation of 0 .. count - 1; the writes stay inside the room
        std::vector<int> seen(hits.size(), 0);
        const long long base = c_off[p], rm = it3_room(base, c_off[p + 1], capacity);
        CHECK(rm >= 0 && (rm == 0 || (base >= 0 && base + rm <= capacity)));
        for (unsigned id : hits) {
            int rank = 0;
            for (unsigned other : hits) rank += other < id ? 1 : 0;
            CHECK(seen[(size_t)rank]++ == 0);
            if (rank < rm) { out_src[(size_t)(base + rank)] = i - s_off[p]; out_tgt[(size_t)(base + rank)] = (long long)id - t0; }
        }
    }
}

int main() {
    const int sizes[] = {0, 1, 3, 63, 64, 65, 255, 256, 257, 300};
    const int S = (int)(sizeof(sizes) / sizeof(sizes[0]));
    // selections: identity, reversed, out of range on either side
    for (int P = 1; P <= 4; ++P)
        for (int a = 0; a + P <= S; ++a) {
            std::vector<int> raw(sizes + a, sizes + a + P), out;
            for (int n : raw) out.push_back(n > 64 ? 64 : n);
            const std::vector<int32_t> raw_off = prefix(raw), off = prefix(out);
            std::vector<long long> sel;
            for (int p = 0; p < P; ++p)
                for (int i = 0; i < out[p]; ++i) sel.push_back(raw[p] - 1 - i);
            walk_select(raw_off, off, sel);
            for (size_t i = 0; i < sel.size(); i += 7) sel[i] = (i % 2) ? -1 - (long long)i : (long long)raw[0] + 1000000007LL * (long long)i + 300;
            walk_select(raw_off, off, sel);
            std::vector<int32_t> bad = raw_off;
            bad[P] = raw_off[P] + 1000;                                    // past the end: the pair is skipped
            walk_select(bad, off, std::vector<long long>(sel.size(), 0));
        }
    CHECK(it3_sel_ok(0, 1) && !it3_sel_ok(1, 1) && !it3_sel_ok(-1, 5) && !it3_sel_ok(0, 0) && !it3_sel_ok(1LL << 40, 0x7fffffff));
    CHECK(!it3_slice_ok(-1, 3, 10) && !it3_slice_ok(4, 3, 10) && !it3_slice_ok(0, 11, 10) && it3_slice_ok(0, 0, 0) && it3_slice_ok(10, 10, 10));
    {
        const int32_t off[] = {0, 5, 5, 9};
        CHECK(it3_pair_of(3, off, 9, 0) == 0 && it3_pair_of(3, off, 9, 4) == 0 && it3_pair_of(3, off, 9, 5) == 2 && it3_pair_of(3, off, 9, 9) == 3);
        const int32_t bad[] = {0, -4, 5, 20};
        CHECK(it3_pair_of(3, bad, 9, 2) == 3 && it3_pair_of(3, bad, 9, 7) == 3);      // (0, -4), (-4, 5), (5, 20) are no slices of 9 rows
    }
    // cell coordinates: the ends of the grid, NaN, the float limits; the clamp never moves two coordinates apart
    {
        const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), big = std::numeric_limits<float>::max();
        CHECK(it3_cell(0.f, 0.f, 1.f) == 0 && it3_cell(-5.f, 0.f, 1.f) == 0 && it3_cell(0.999f, 0.f, 1.f) == 0 && it3_cell(1.f, 0.f, 1.f) == 1);
        CHECK(it3_cell(65535.5f, 0.f, 1.f) == IT3_CELL_MAX && it3_cell(1e9f, 0.f, 1.f) == IT3_CELL_MAX && it3_cell(big, -big, 1e-30f) == IT3_CELL_MAX);
        CHECK(it3_cell(inf, 0.f, 1.f) == IT3_CELL_MAX && it3_cell(-inf, 0.f, 1.f) == 0 && it3_cell(nan, 0.f, 1.f) == 0 && it3_cell(1.f, inf, 1.f) == 0);
        CHECK(it3_cell(1.f, nan, 1.f) == 0 && it3_cell(1.f, 0.f, 0.f) == IT3_CELL_MAX);
        for (float v = -3.f; v < 70000.f; v += 0.37f) {
            const int a = it3_cell(v, 0.f, 1.f), b = it3_cell(v + 0.99f, 0.f, 1.f);
            CHECK(a >= 0 && b <= IT3_CELL_MAX && b - a >= 0 && b - a <= 1);
        }
        unsigned long long first, last;
        CHECK(!it3_run_keys(0, 0, 0, 0, 0, first, last) && it3_run_keys(0, 0, 0, 0, 4, first, last) && first == it3_key(0, 0, 0, 0) && last == it3_key(0, 1, 0, 0));
        CHECK(it3_run_keys(IT3_KEY_PAIRS, IT3_CELL_MAX, IT3_CELL_MAX, IT3_CELL_MAX, 4, first, last) && last == it3_key(IT3_KEY_PAIRS, IT3_CELL_MAX, IT3_CELL_MAX, IT3_CELL_MAX));
        CHECK(last + 1 < IT3_PAD_KEY && !it3_run_keys(0, 5, IT3_CELL_MAX, 5, 5, first, last) && !it3_run_keys(0, 5, 5, IT3_CELL_MAX, 8, first, last));
        CHECK(it3_key(IT3_MAX_PAIRS + 1, 0, 0, 0) < IT3_PAD_KEY);                                    // the key of a row that belongs to no pair
    }
    // the pair list: ragged batches, dense and sparse clouds, room below / equal / above what is found, a list shorter than the rooms add up to
    for (int P = 1; P <= 4; ++P)
        for (int a = 0; a + P <= S; a += 2)
            for (int b = 0; b + P <= S; b += 3) {
                std::vector<int> ns(sizes + a, sizes + a + P), nt(sizes + b, sizes + b + P);
                std::vector<long long> room((size_t)P);
                for (int p = 0; p < P; ++p) room[p] = (p % 3 == 0) ? 7 : (p % 3 == 1 ? 100000 : 0);
                walk_pairs(ns, nt, 0.0375f, room, 100007 * (long long)P, (unsigned)(a * 31 + b), 0.2f);      // sparse
                walk_pairs(ns, nt, 0.0375f, room, 50, (unsigned)(a * 31 + b + 1), 0.02f);                    // dense: rows with > 64 partners
            }
    walk_pairs({65, 3, 130}, {130, 64, 7}, 0.0375f, {100000, 100000, 100000}, 300000, 77u, 0.1f, 5);   // offsets[0] = 5: rows of no pair in front
    walk_pairs({300}, {300}, 1e-6f, {10}, 10, 5u, 1.0f);        // a cloud wider than the grid: the cells clamp, the sweep stays complete
    CHECK(it3_room(0, 10, 5) == 5 && it3_room(3, 10, 20) == 7 && it3_room(10, 3, 20) == 0 && it3_room(-1, 10, 20) == 0 && it3_room(21, 30, 20) == 0);
    CHECK(it3_room(20, 30, 20) == 0 && it3_room(0, 1LL << 40, 1LL << 30) == (1LL << 30));
    CHECK(it3_saturate(-5) == 0 && it3_saturate(0x7fffffffLL) == 0x7fffffff && it3_saturate(1LL << 40) == 0x7fffffff && it3_saturate(12) == 12);
    CHECK(next_pow2(0) == 1 && next_pow2(1) == 1 && next_pow2(257) == 512 && next_pow2(IT3_MAX_ROWS) == IT3_MAX_ROWS);
    CHECK(it3_blocks(0, 256) == 1 && it3_blocks(256, 256) == 1 && it3_blocks(257, 256) == 2 && it3_blocks(IT3_MAX_ROWS, IT3_ROWS) == (unsigned)(IT3_MAX_ROWS / IT3_ROWS));
    // the workspace carve: six arrays in order, each on 256 bytes, none overlapping, the total covering the last
    const int carve[][3] = {{1, 0, 0}, {1, 1, 1}, {3, 63, 65}, {2, 300, 257}, {IT3_MAX_PAIRS, IT3_MAX_ROWS, IT3_MAX_ROWS}, {-1, -4, -4}};
    for (const auto& c : carve) {
        const It3PairsCarve k = it3_pairs_carve(c[0], c[1], c[2]);
        const size_t p = c[0] > 0 ? c[0] : 0, s = c[1] > 0 ? c[1] : 0, t = c[2] > 0 ? c[2] : 0, pad = c[2] > 0 ? (size_t)next_pow2(c[2]) : 0;
        CHECK(k.moved == 0 && k.row_start % 256 == 0 && k.origin % 256 == 0 && k.keys % 256 == 0 && k.vals % 256 == 0 && k.sorted % 256 == 0);
        CHECK(k.row_start >= k.moved + s * 12 && k.origin >= k.row_start + s * 8 && k.keys >= k.origin + p * 16 && k.vals >= k.keys + pad * 8);
        CHECK(k.sorted >= k.vals + pad * 4 && k.bytes >= k.sorted + t * 16);
    }
    CHECK(it3_pairs_carve(-1, -4, -4).bytes == 0);
    std::printf("item3d_index_check ok: %lld rows and candidates walked\n", g_tests);
    return 0;
}
