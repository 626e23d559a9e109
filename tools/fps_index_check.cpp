// fps_index_check.cpp -- host check of csrc/fps_index.h, the only place the furthest-point sampling kernels (csrc/fps.hip) compute an index.
// Build and run, on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/fps_index_check.cpp \
//         -o /tmp/fps_index_check && /tmp/fps_index_check
//
// It walks, as the kernels do and on real allocations of exactly the sizes the entries are given (AddressSanitizer guards their ends):
//   * the ragged offsets: every cloud's slice lies inside the stacked array, bad offsets are refused;
//   * the on-chip form: (thread, slot) -> point is a bijection onto [0, slots FPS_BLOCK) that covers the cloud, for every compile-time slot
//     count the kernel dispatches to; a slot behind the cloud reads row 0; every coordinate read lies inside the cloud's rows;
//   * the streaming form: the threads' strided walks visit every point of the cloud exactly once and touch only the cloud's own floats of
//     the workspace, whose size is the size query's;
//   * the LDS exchange: the two parity buffers of FPS_WAVES rows are disjoint and inside FPS_LDS_WORDS;
//   * the padded outputs: node k of cloud p, for k < sample_cap, inside [P, sample_cap] (x 3);
// over the shapes of the GPU tests: n = 0, 1, 2, 5, 9, 63, 64, 65, 75, 1023, 1024, 1025, 9000, the capacity and capacity + 1, alone and in
// ragged batches, and the batch form's (B, N).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fps_index.h"

using namespace dr;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

static long long g_reads = 0;
static const int SLOT_FORMS[] = {1, 2, 4, 9, FPS_SLOTS};     // fps_kernel's dispatch

static int slots_form(int n) {
    const int used = fps_slots_used(n);
    for (int s : SLOT_FORMS)
        if (used <= s) return s;
    return -1;
}

static void walk_cloud(const std::vector<float>& pts, std::vector<float>& work, int lo, int n, bool streaming) {
    const float* base = pts.data() + fps_coord(lo, 0, 0);
    std::vector<int> seen((size_t)n, 0);
    if (!streaming) {
        CHECK(fps_fits_onchip(n));
        const int S = slots_form(n);
        CHECK(S >= 1 && S <= FPS_SLOTS && (long long)S * FPS_BLOCK >= n);
        for (int t = 0; t < FPS_BLOCK; ++t)
            for (int k = 0; k < S; ++k) {
                const int i = fps_point_of(t, k);
                CHECK(fps_point_thread(i) == t && fps_point_slot(i) == k);
                const int r = i < n ? i : 0;
                volatile float v = base[fps_local_coord(r, 0)] + base[fps_local_coord(r, 1)] + base[fps_local_coord(r, 2)];
                (void)v;
                g_reads += 3;
                if (i < n) ++seen[i];
            }
    } else {
        float* w = work.data() + fps_row(lo, 0);
        for (int t = 0; t < FPS_BLOCK; ++t) {
            int visits = 0;
            for (int i = t; i < n; i += FPS_BLOCK, ++visits) {
                w[i] = base[fps_local_coord(i, 0)] + base[fps_local_coord(i, 1)] + base[fps_local_coord(i, 2)];
                g_reads += 3;
                ++seen[i];
            }
            CHECK(visits == fps_stream_visits(n, t));
        }
    }
    for (int v : seen) CHECK(v == 1);
}

static void walk_batch(const std::vector<int>& lens, int cap, bool force_streaming) {
    const int P = (int)lens.size();
    std::vector<int> off(P + 1, 0);
    int mx = 0;
    for (int p = 0; p < P; ++p) { off[p + 1] = off[p] + lens[p]; mx = lens[p] > mx ? lens[p] : mx; }
    const int n_points = off[P];
    std::vector<float> pts((size_t)n_points * 3, 1.0f);
    const size_t wsb = fps_workspace_bytes(n_points, mx, force_streaming);
    CHECK((wsb == 0) == (n_points == 0 || (fps_fits_onchip(mx) && !force_streaming)));
    CHECK(wsb == 0 || wsb >= (size_t)n_points * sizeof(float));
    std::vector<float> work(wsb ? (size_t)n_points : 0);      // exactly the floats the kernel may touch
    std::vector<long long> out_idx((size_t)P * cap);
    std::vector<float> out_pts((size_t)P * cap * 3), out_dist((size_t)P * cap);
    for (int p = 0; p < P; ++p) {
        CHECK(nr_slice_ok(off[p], off[p + 1], n_points));
        const int n = off[p + 1] - off[p];
        if (n > 0) walk_cloud(pts, work, off[p], n, force_streaming || !fps_fits_onchip(n));
        for (int k = 0; k < cap; ++k) {
            out_idx[fps_out(p, cap, k)] = k;
            out_dist[fps_out(p, cap, k)] = 0.0f;
            for (int c = 0; c < 3; ++c) out_pts[fps_out_coord(p, cap, k, c)] = 0.0f;
        }
    }
    CHECK(!nr_slice_ok(-1, 0, n_points) && !nr_slice_ok(1, 0, n_points) && !nr_slice_ok(0, n_points + 1, n_points));
}

int main() {
    CHECK(FPS_WAVES == 16 && FPS_BLOCK == FPS_WAVES * FPS_WAVE);       // one DPP row holds every wave's partial
    CHECK(fps_onchip_capacity() == FPS_BLOCK * FPS_SLOTS);
    std::vector<int> lds(FPS_LDS_WORDS, 0);
    for (int parity = 0; parity < 4; ++parity)
        for (int w = 0; w < FPS_WAVES; ++w)
            for (int word = 0; word < 5; ++word) {
                const int a = fps_partial_word(parity, w, word);
                CHECK(a >= 0 && a < FPS_LDS_WORDS);
                CHECK(fps_partial_word(parity + 2, w, word) == a && fps_partial_word(parity + 1, w, word) != a);
                ++lds[a];
            }
    for (int v : lds) CHECK(v == 0 || v == 2);
    const int cap = fps_onchip_capacity();
    for (int n : {0, 1, 2, 5, 9, 63, 64, 65, 75, 1023, 1024, 1025, 9000, cap, cap + 1})
        for (int force = 0; force < 2; ++force) walk_batch({n}, n > 512 ? 512 : (n > 0 ? n : 1), force != 0);
    walk_batch({0, 70, 5}, 16, false);
    walk_batch({70, 0, 5}, 16, false);
    walk_batch({70, 5, 0}, 16, true);
    walk_batch({1025, 100, 0, 75}, 300, false);
    walk_batch({1025, 100, 0, 75}, 300, true);
    walk_batch({cap + 1, 7}, 12, false);
    walk_batch({1, 2, 63, 64, 65, 1023, 1024, 1025, 9000}, 512, false);
    for (auto bn : {std::pair<int, int>{1, 1}, {3, 64}, {2, 65}, {2, 1025}, {1, 5}}) {
        std::vector<int> lens((size_t)bn.first, bn.second);
        for (int b = 0; b < bn.first; ++b) CHECK(fps_batch_lo(b, bn.second) == b * bn.second);
        walk_batch(lens, 33, false);
        walk_batch(lens, 33, true);
    }
    std::printf("fps_index_check: ok (%lld coordinate reads walked)\n", g_reads);
    return 0;
}
