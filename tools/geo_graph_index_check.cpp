// geo_graph_index_check.cpp -- host check of csrc/geo_graph_index.h, the only place the geodesic deformation-graph kernels (csrc/geo_graph.hip)
// compute an index.  Build and run, on the host only:
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I diff-reg_amd/csrc tools/geo_graph_index_check.cpp \
//         -o /tmp/geo_graph_index_check && /tmp/geo_graph_index_check
//
// It walks, as the kernels do and on real allocations of exactly the sizes the entries are given (AddressSanitizer guards their ends):
//   * the offsets: which clouds are usable, and that geo_locate hands every tile of every usable cloud (unit NR_TILE) and every node (unit 1)
//     to exactly one flat workgroup index below the launch's grid, and nothing from the first unusable cloud on;
//   * the workspace carve: the mark and degree words of every point, every adjacency slot, every word of the reach table, inside the bytes the
//     size query reports, the four parts disjoint;
//   * the LDS carve of the relaxation, on chip (the cloud's two distance words per point) and streamed, with the nodes' keys and the counter,
//     inside the bytes the launch asks for and inside the compute unit's LDS at the capacity;
//   * the padded tables [rows, K];
//   * the edge list: the chunked count-and-scan places every edge of a random neighbour table where the plain row-major statement puts it,
//     and never at or behind min(e_offsets[p + 1], edge_cap);
// over the shapes of the GPU tests: n = 0, 1, 40, 63, 64, 65, 127, 128, 129, 800, 1800, M = 0, 1, 3, 255, 256, 257, alone and in ragged calls,
// a forced capacity below and at the cloud size, and the capacity and capacity + 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "geo_graph_index.h"

using namespace dr;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

static long long g_walked = 0;

static std::vector<int32_t> offsets(const std::vector<int>& lens) {
    std::vector<int32_t> o(lens.size() + 1, 0);
    for (size_t p = 0; p < lens.size(); ++p) o[p + 1] = o[p] + lens[p];
    return o;
}

// every (cloud, tile) of the usable clouds is hit exactly once by b in [0, grid)
static void walk_locate(const std::vector<int32_t>& off, int total, int unit, long long grid) {
    const int P = (int)off.size() - 1;
    std::vector<std::vector<int>> hit(P);
    int usable = 0;
    while (usable < P && geo_cloud_ok(off.data(), usable, total)) ++usable;
    for (int p = usable; p < P; ++p) CHECK(!geo_cloud_ok(off.data(), p, total));      // usable clouds are a prefix
    for (int p = 0; p < usable; ++p) hit[p].assign((size_t)((off[p + 1] - off[p] + unit - 1) / unit), 0);
    for (long long b = 0; b < grid; ++b) {
        int p = -1, t = -1;
        if (!geo_locate(P, off.data(), total, unit, b, p, t)) continue;
        CHECK(p >= 0 && p < usable && t >= 0 && t < (int)hit[p].size());
        ++hit[p][t];
        ++g_walked;
    }
    for (int p = 0; p < usable; ++p)
        for (int v : hit[p]) CHECK(v == 1);
    int p, t;
    CHECK(!geo_locate(P, off.data(), total, unit, grid, p, t));          // nothing behind the grid: the launch covers every tile
}

static void walk_call(const std::vector<int>& plens, const std::vector<int>& mlens, int Kn, int Ka, int D, int cap_override) {
    const int P = (int)plens.size();
    CHECK((int)mlens.size() == P);
    const std::vector<int32_t> po = offsets(plens), mo = offsets(mlens);
    const int n_points = po[P], n_nodes = mo[P];
    int mxp = 0, mxn = 0;
    for (int v : plens) mxp = v > mxp ? v : mxp;
    for (int v : mlens) mxn = v > mxn ? v : mxn;
    walk_locate(po, n_points, NR_TILE, nr_grid_bound(n_points, P));
    walk_locate(mo, n_nodes, 1, n_nodes);

    const GeoCarve c = geo_carve(n_points, n_nodes, mxp, D);
    CHECK(c.mark % 16 == 0 && c.deg % 16 == 0 && c.adj % 16 == 0 && c.reach % 16 == 0);
    CHECK(c.deg >= c.mark + (size_t)n_points * 4 && c.adj >= c.deg + (size_t)n_points * 4);
    CHECK(c.reach >= c.adj + (size_t)n_points * D * sizeof(GeoAdj) && c.bytes >= c.reach + (size_t)n_nodes * mxp * 4);
    std::vector<char> ws(c.bytes);                                    // exactly the bytes the size query reports
    int32_t* mark = (int32_t*)(ws.data() + c.mark);
    int32_t* deg = (int32_t*)(ws.data() + c.deg);
    GeoAdj* adj = (GeoAdj*)(ws.data() + c.adj);
    uint32_t* reach = (uint32_t*)(ws.data() + c.reach);
    std::vector<long long> nbr((size_t)n_nodes * Kn), anc((size_t)n_points * Ka);

    const int cap = geo_effective_capacity(cap_override);
    CHECK(cap >= 1 && cap <= GEO_ONCHIP_CAPACITY);
    const GeoLdsCarve on = geo_lds_carve(geo_lds_points(mxp, cap), mxn), off = geo_lds_carve(0, mxn);
    CHECK(on.bytes <= NR_LDS_BYTES && off.bytes <= on.bytes);
    std::vector<uint32_t> lds_on((size_t)on.bytes / 4), lds_off((size_t)off.bytes / 4);

    for (int p = 0; p < P; ++p) {
        CHECK(geo_cloud_ok(po.data(), p, n_points) && geo_cloud_ok(mo.data(), p, n_nodes));
        const int lo = po[p], n = po[p + 1] - lo, m0 = mo[p], M = mo[p + 1] - m0;
        for (int x = 0; x < n; ++x) {
            mark[lo + x] = 0;
            deg[lo + x] = D;
            for (int e = 0; e < D; ++e) {
                adj[geo_adj_slot(lo, x, D, e)].y = x;
                ++g_walked;
            }
            for (int k = 0; k < Ka; ++k) anc[geo_table(lo + x, Ka, k)] = -1;
        }
        const bool onchip = n <= cap;
        const GeoLdsCarve& L = onchip ? on : off;
        std::vector<uint32_t>& lds = onchip ? lds_on : lds_off;
        for (int i = 0; i < M; ++i) {
            const int row = m0 + i;
            for (int x = 0; x < n; ++x) {
                if (onchip) {
                    lds[L.g + x] = GEO_UNREACHED;
                    lds[L.done + x] = GEO_UNREACHED;
                }
                reach[geo_reach(row, mxp, x)] = GEO_UNREACHED;
            }
            for (int j = 0; j < M; ++j) {
                lds[L.node_g + j] = 0;
                lds[L.node_pt + j] = (uint32_t)j;
            }
            lds[L.count] = 0;
            for (int k = 0; k < Kn; ++k) nbr[geo_table(row, Kn, k)] = -1;
            ++g_walked;
        }
    }
    // the carve's parts do not overlap: what the walk wrote last into each part is still there
    if (n_points > 0) CHECK(mark[0] == 0 && deg[0] == D);
}

// the edge kernel's chunked scan against the plain statement
static void walk_edges(const std::vector<int>& mlens, int Kn, unsigned seed, long long cap_cut) {
    const int P = (int)mlens.size();
    const std::vector<int32_t> mo = offsets(mlens);
    const int n_nodes = mo[P];
    std::vector<long long> nbr((size_t)n_nodes * Kn);
    for (auto& v : nbr) {
        seed = seed * 1664525u + 1013904223u;
        v = (long long)((seed >> 16) % 14) - 2;                          // -2 .. 11: absent, out of range, selves, repeats
    }
    std::vector<int32_t> counts(P), eo(P + 1, 0);
    std::vector<std::pair<long long, long long>> plain;
    for (int p = 0; p < P; ++p) {
        const int m0 = mo[p], M = mo[p + 1] - m0;
        int base = 0;
        CHECK(geo_edge_chunks(M) * GEO_EDGE_BLOCK >= M && (geo_edge_chunks(M) - 1) * GEO_EDGE_BLOCK < (M > 0 ? M : 1));
        for (int c = 0; c < geo_edge_chunks(M); ++c)
            for (int t = 0; t < GEO_EDGE_BLOCK; ++t) {
                const int i = c * GEO_EDGE_BLOCK + t;
                if (i >= M) continue;
                for (int k = 0; k < Kn; ++k) base += geo_is_edge(nbr[geo_table(m0 + i, Kn, k)], i, M) ? 1 : 0;
            }
        counts[p] = base;
        eo[p + 1] = eo[p] + base;
        for (int i = 0; i < M; ++i)
            for (int k = 0; k < Kn; ++k) {
                const long long j = nbr[geo_table(m0 + i, Kn, k)];
                if (j >= 0 && j < M && j != i) plain.push_back({i, j});
            }
    }
    const long long E = eo[P], edge_cap = cap_cut >= 0 && cap_cut < E ? cap_cut : E;
    CHECK((long long)plain.size() == E);
    std::vector<long long> out((size_t)edge_cap * 2, -7);                // exactly edge_cap rows
    for (int p = 0; p < P; ++p) {
        const int m0 = mo[p], M = mo[p + 1] - m0;
        const long long lo = eo[p], hi = eo[p + 1] < edge_cap ? eo[p + 1] : edge_cap;
        int base = 0;
        for (int c = 0; c < geo_edge_chunks(M); ++c) {
            int scan[GEO_EDGE_BLOCK], mine[GEO_EDGE_BLOCK];
            for (int t = 0; t < GEO_EDGE_BLOCK; ++t) {
                const int i = c * GEO_EDGE_BLOCK + t;
                mine[t] = 0;
                if (i < M)
                    for (int k = 0; k < Kn; ++k) mine[t] += geo_is_edge(nbr[geo_table(m0 + i, Kn, k)], i, M) ? 1 : 0;
                scan[t] = mine[t] + (t ? scan[t - 1] : 0);
            }
            for (int t = 0; t < GEO_EDGE_BLOCK; ++t) {
                const int i = c * GEO_EDGE_BLOCK + t;
                if (i >= M) continue;
                long long at = lo + base + scan[t] - mine[t];
                for (int k = 0; k < Kn; ++k) {
                    const long long j = nbr[geo_table(m0 + i, Kn, k)];
                    if (!geo_is_edge(j, i, M)) continue;
                    if (at < hi) {
                        out[2 * at] = i;
                        out[2 * at + 1] = j;
                        ++g_walked;
                    }
                    ++at;
                }
            }
            base += scan[GEO_EDGE_BLOCK - 1];
        }
        CHECK(base == counts[p]);
    }
    for (long long e = 0; e < edge_cap; ++e) CHECK(out[2 * e] == plain[e].first && out[2 * e + 1] == plain[e].second);
}

int main() {
    CHECK(geo_lds_carve(GEO_ONCHIP_CAPACITY, GEO_MAX_NODES).bytes <= NR_LDS_BYTES);
    CHECK(geo_effective_capacity(0) == GEO_ONCHIP_CAPACITY && geo_effective_capacity(40) == 40 &&
          geo_effective_capacity(GEO_ONCHIP_CAPACITY + 5) == GEO_ONCHIP_CAPACITY);
    CHECK(sizeof(GeoAdj) == 8);
    // offsets that are none: everything from the first break on is refused
    {
        const std::vector<int32_t> bad = {0, 10, 5, 10};
        CHECK(geo_cloud_ok(bad.data(), 0, 10) && !geo_cloud_ok(bad.data(), 1, 10) && !geo_cloud_ok(bad.data(), 2, 10));
        walk_locate(bad, 10, 1, 10);
        walk_locate(bad, 10, NR_TILE, nr_grid_bound(10, 3));
        const std::vector<int32_t> neg = {-1, 4}, over = {0, 11};
        CHECK(!geo_cloud_ok(neg.data(), 0, 10) && !geo_cloud_ok(over.data(), 0, 10));
        walk_locate(neg, 10, 1, 10);
        walk_locate(over, 10, 1, 10);
    }
    for (int n : {0, 1, 40, 63, 64, 65, 127, 128, 129, 800, 1800})
        for (int M : {0, 1, 3, 76})
            for (int cap : {0, 8, n > 1 ? n - 1 : 1, n > 0 ? n : 1}) walk_call({n}, {M > n ? n : M}, 8, 6, n > 200 ? 16 : 64, cap);
    walk_call({65, 130, 200}, {5, 0, 3}, 8, 6, 64, 0);
    walk_call({65, 130, 200}, {5, 0, 3}, 8, 6, 64, 100);
    walk_call({0, 0, 7}, {0, 0, 7}, 1, 1, 1, 0);
    walk_call({1}, {1}, 3, 2, 64, 0);
    walk_call({GEO_ONCHIP_CAPACITY}, {4}, 8, 8, 2, 0);
    walk_call({GEO_ONCHIP_CAPACITY + 1, 9}, {4, 2}, 8, 8, 2, 0);
    walk_call({300}, {GEO_MAX_NODES > 300 ? 300 : GEO_MAX_NODES}, 8, 8, 4, 0);
    for (int M : {0, 1, 3, 255, 256, 257, 600})
        for (int Kn : {1, 4, 8}) walk_edges({M}, Kn, 17u * (unsigned)M + (unsigned)Kn, -1);
    walk_edges({300, 0, 5, 257}, 4, 99u, -1);
    walk_edges({300, 0, 5, 257}, 4, 99u, 10);
    walk_edges({300, 0, 5, 257}, 8, 7u, 0);
    std::printf("geo_graph_index_check: ok (%lld indices walked)\n", g_walked);
    return 0;
}
