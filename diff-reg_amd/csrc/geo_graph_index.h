// geo_graph_index.h -- every index the geodesic deformation-graph kernels (geo_graph.hip: dr_geo_graph_f32, dr_geo_graph_edges) compute, stated
// once for the device and for the host check (tools/geo_graph_index_check.cpp): which clouds of a call are usable, the mapping of a flat
// workgroup index to (cloud, tile) and to (cloud, node), the fixed-width adjacency rows, the dense reach table, the LDS carve that fixes the
// on-chip capacity, the padded output tables, the chunked scan of the edge list, and the workspace that the size query and the entry share.
// Outside hipcc the file compiles as plain C++.
#pragma once
#include "nonrigid_index.h"      // NR_TILE, NR_LDS_BYTES, align256, nr_grid_bound

namespace dr {

constexpr int GEO_BLOCK = 1024;            // threads of the workgroup that relaxes one node's distances to a fixed point
constexpr int GEO_MAX_K = 8;               // compiled limit of num_neighbors and of num_anchors
constexpr int GEO_MAX_NODES = 2048;        // nodes of one cloud: their (distance, point) keys are staged in LDS for the neighbour selection
constexpr int GEO_ONCHIP_CAPACITY = 16384; // points of one cloud whose two distance words stay in LDS; a larger cloud relaxes in the workspace
constexpr int GEO_MAX_DEGREE = 1024;       // upper limit of the adjacency row width a caller may ask for
constexpr int GEO_EDGE_BLOCK = 256;        // threads (= neighbour rows per chunk) of the edge-list kernel
constexpr uint32_t GEO_UNREACHED = 0x7f800000u;   // +inf: non-negative float32 order as unsigned integers, so min() on the bits is min() on the values

constexpr int GEO_ST_SIZE = 1;             // status bit: more points than max_points or more nodes than max_nodes: padding only
constexpr int GEO_ST_OFFSETS = 2;          // status bit: the offsets up to this cloud are not 0 <= o[0] <= ... <= o[p + 1] <= total: nothing is written
constexpr int GEO_ST_INDEX = 4;            // status bit: a node index outside [0, n) was met and treated as absent
constexpr int GEO_ST_NONFINITE = 8;        // status bit: a point with a NaN or Inf coordinate was met (it has no edges)
constexpr int GEO_ST_DUPLICATE = 256;      // status bit: two nodes name the same point; the cloud's results are only guaranteed to be in range
constexpr int GEO_ST_DEGREE = 512;         // status bit: a point has more than max_degree points closer than max_distance: padding only

struct GeoAdj {
    int32_t y;                             // the other end, cloud-local
    float d;                               // the edge's float32 length
};

__host__ __device__ inline int geo_onchip_capacity() { return GEO_ONCHIP_CAPACITY; }
// the capacity a call uses: the default, or a smaller one a test asks for
__host__ __device__ inline int geo_effective_capacity(int override_cap) {
    return (override_cap > 0 && override_cap < GEO_ONCHIP_CAPACITY) ? override_cap : GEO_ONCHIP_CAPACITY;
}

// cloud p is usable iff the offsets up to it ascend inside [0, total]: usable clouds then own disjoint slices, in order
__host__ __device__ inline bool geo_cloud_ok(const int32_t* off, int p, int total) {
    int prev = 0;
    for (int q = 0; q <= p + 1; ++q) {
        const int o = off[q];
        if (o < prev || o > total) return false;
        prev = o;
    }
    return true;
}

// flat workgroup b -> (cloud, tile) with ceil(n_p / unit) tiles per usable cloud, clouds in order; false behind the last tile and from the
// first unusable cloud on.  unit = 1 maps a flat node index to (cloud, node).  O(P) reads: P is a batch size.
__host__ __device__ inline bool geo_locate(int P, const int32_t* off, int total, int unit, long long b, int& cloud, int& tile) {
    long long first = 0;
    int prev = 0;
    if (P > 0 && (off[0] < 0 || off[0] > total)) return false;
    prev = P > 0 ? off[0] : 0;
    for (int p = 0; p < P; ++p) {
        const int hi = off[p + 1];
        if (hi < prev || hi > total) return false;
        const long long t = ((long long)(hi - prev) + unit - 1) / unit;
        if (b < first + t) {
            cloud = p;
            tile = (int)(b - first);
            return true;
        }
        first += t;
        prev = hi;
    }
    return false;
}

// ---- adjacency: point x of the cloud that starts at stacked row lo owns `degree` slots; slot e
__host__ __device__ inline size_t geo_adj_slot(int lo, int x, int degree, int e) { return ((size_t)lo + (size_t)x) * (size_t)degree + (size_t)e; }

// ---- reach table: one row of `stride` (= max_points) words per stacked node row; word x is the node's path length to point x of its cloud
__host__ __device__ inline size_t geo_reach(int node_row, int stride, int x) { return (size_t)node_row * (size_t)stride + (size_t)x; }

// ---- padded outputs: column k of stacked row r of a table K wide
__host__ __device__ inline size_t geo_table(int row, int K, int k) { return (size_t)row * (size_t)K + (size_t)k; }

// ---- LDS of the relaxation workgroup, in 32-bit words: the distance of every point of the cloud and the distance at which it was last
// expanded (on-chip form only: `points` = 0 otherwise), the nodes' keys, one counter
struct GeoLdsCarve {
    int g, done, node_g, node_pt, count, bytes;
};
__host__ __device__ inline GeoLdsCarve geo_lds_carve(int points, int max_nodes) {
    GeoLdsCarve c;
    const int n = points > 0 ? points : 0, m = max_nodes > 0 ? max_nodes : 0;
    c.g = 0;
    c.done = c.g + n;
    c.node_g = c.done + n;
    c.node_pt = c.node_g + m;
    c.count = c.node_pt + m;
    c.bytes = (c.count + 4) * 4;
    return c;
}
// points the on-chip launch of a call carves for
__host__ __device__ inline int geo_lds_points(int max_points, int cap) { return max_points < cap ? max_points : cap; }

// ---- edge list: rows are walked in chunks of GEO_EDGE_BLOCK; chunks of a cloud of M nodes
__host__ __device__ inline int geo_edge_chunks(int M) { return M <= 0 ? 0 : (M + GEO_EDGE_BLOCK - 1) / GEO_EDGE_BLOCK; }
// neighbour j of node i makes an edge
__host__ __device__ inline bool geo_is_edge(long long j, int i, int M) { return j >= 0 && j < M && j != i; }

// ---- workspace
struct GeoCarve {
    size_t mark, deg, adj, reach, bytes;
};
__host__ __device__ inline GeoCarve geo_carve(int n_points, int n_nodes, int max_points, int max_degree) {
    GeoCarve c;
    const size_t n = n_points > 0 ? (size_t)n_points : 0, m = n_nodes > 0 ? (size_t)n_nodes : 0;
    const size_t s = max_points > 0 ? (size_t)max_points : 0, d = max_degree > 0 ? (size_t)max_degree : 0;
    c.mark = 0;
    c.deg = c.mark + align256(n * sizeof(int32_t));
    c.adj = c.deg + align256(n * sizeof(int32_t));
    c.reach = c.adj + align256(n * d * sizeof(GeoAdj));
    c.bytes = c.reach + align256(m * s * sizeof(uint32_t));
    return c;
}

}  // namespace dr
