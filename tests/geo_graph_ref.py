"""A numpy float32 statement of vision3d's build_deformation_graph_from_point_cloud (2D-3D vision3d/csrc/cpu/deformation_graph/
deformation_graph.cpp:13-180), in two forms that must agree bit for bit:

  * heap_reach: the reference's procedure -- a bounded Dijkstra from every node with its max-heap of (-g, point) and its pruning;
  * fixed_point_reach: what the device does -- relax g(y) = min(g(y), fl(g(x) + d(x, y))) over all edges until nothing changes.

Both produce the reach table G [M, n] (float32 path lengths, +inf where node i does not reach point x); tables() turns it into the six
arrays under the stated orders: neighbours by (g ascending, point index descending), anchors by (g ascending, node index ascending).
Float32 addition is monotone (a <= b implies fl(a + d) <= fl(b + d)), so the least fixed point of the relaxation is what Dijkstra settles,
whatever the order of relaxations: tests/test_geo_graph_cpu.py holds that on random graphs.

SCENES and scene() also define the fixture's inputs (tools/golden/make_golden_geo_graph.py mints tests/golden/geo_graph.npz from them by
running the reference's C++)."""
import heapq

import numpy as np

from tests import fps_ref

ST_INDEX, ST_NONFINITE, ST_DUPLICATE, ST_DEGREE = 4, 8, 256, 512
KEYS = ("neighbor_indices", "neighbor_distances", "neighbor_weights", "anchor_indices", "anchor_distances", "anchor_weights")

# name, kind, size, num_neighbors, num_anchors, max_distance, node_coverage, node rule
#   node rule: ("fps", min_distance) over the whole cloud, ("fps_head", min_distance, k) over the first k points, ("list", [...])
SCENES = [
    ("sheets", "sheets", 20, 8, 6, 0.035, 0.05, ("fps", 0.05)),          # two sheets 0.06 apart: above max_distance, below 2 c
    ("ustrip", "ustrip", 60, 8, 6, 0.035, 0.05, ("fps", 0.05)),          # the arms of the U are 0.05 apart
    ("nonode", "blobs", 300, 8, 6, 0.05, 0.08, ("fps_head", 0.08, 300)),  # the second blob has no node: rows of -1
    ("sparse", "patch", 200, 8, 6, 0.05, 0.08, ("list", [5, 90, 150])),  # fewer reachable nodes than Kn and than Ka
    ("isolated", "outlier", 200, 4, 3, 0.05, 0.08, ("list", [200, 10, 60, 120, 180])),   # node 0 is a point far from every other
    ("m1", "patch", 150, 8, 6, 0.05, 0.08, ("list", [17])),
    ("n1", "patch", 1, 3, 2, 0.05, 0.08, ("list", [0])),
    ("n63", "patch", 63, 8, 6, 0.08, 0.1, ("fps", 0.1)),
    ("n64", "patch", 64, 8, 6, 0.08, 0.1, ("fps", 0.1)),
    ("n65", "patch", 65, 8, 6, 0.08, 0.1, ("fps", 0.1)),
    ("big", "wave", 1800, 8, 6, 0.03, 0.06, ("fps", 0.06)),              # more than one block of every kernel, a curved surface
]


def scene(name, seed):
    """-> (points [n, 3] float32, node_indices [M] int64, Kn, Ka, max_distance, node_coverage)"""
    _, kind, size, Kn, Ka, maxd, c, rule = next(s for s in SCENES if s[0] == name)
    rng = np.random.default_rng(seed)
    jit = lambda shape, s: rng.uniform(-s, s, shape)
    if kind == "sheets":
        u, v = np.meshgrid(np.arange(size) * 0.02, np.arange(size) * 0.02, indexing="ij")
        one = np.stack([u.ravel(), v.ravel(), np.zeros(u.size)], 1)
        pts = np.concatenate([one, one + [0.0, 0.0, 0.06]]) + jit((2 * u.size, 3), 0.004)
        pts = pts[rng.permutation(len(pts))]
    elif kind == "ustrip":
        s = np.arange(size) * 0.015                       # arc length along the U: down one arm, round a half circle, up the other
        arm, r = 0.35, 0.025
        x = np.where(s < arm, 0.0, np.where(s < arm + np.pi * r, r - r * np.cos((s - arm) / r), 2 * r))
        y = np.where(s < arm, arm - s, np.where(s < arm + np.pi * r, -r * np.sin((s - arm) / r), s - arm - np.pi * r))
        w = np.arange(5) * 0.015
        pts = np.stack([np.repeat(x, 5), np.repeat(y, 5), np.tile(w, size)], 1) + jit((size * 5, 3), 0.003)
    elif kind == "blobs":
        a = rng.uniform(0, 0.4, (size, 3)) * [1, 1, 0.05]
        b = rng.uniform(0, 0.15, (size // 5, 3)) * [1, 1, 0.05] + [2.0, 0, 0]
        pts = np.concatenate([a, b])
    elif kind == "outlier":
        pts = np.concatenate([rng.uniform(0, 0.4, (size, 3)) * [1, 1, 0.05], [[5.0, 5.0, 5.0]]])
    elif kind == "wave":
        uv = rng.uniform(0, 0.6, (size, 2))
        pts = np.stack([uv[:, 0], uv[:, 1], 0.05 * np.sin(uv[:, 0] * 12) + jit(size, 0.002)], 1)
    else:
        side = max(0.4 * np.sqrt(size / 200.0), 0.01)
        pts = rng.uniform(0, side, (size, 3)) * [1, 1, 0.05]
    pts = np.ascontiguousarray(pts, np.float32)
    if rule[0] == "fps":
        nodes = fps_ref.nodes(pts, rule[1], None)[0]
    elif rule[0] == "fps_head":
        nodes = fps_ref.nodes(pts[:rule[2]], rule[1], None)[0]
    else:
        nodes = np.asarray(rule[1])
    return pts, np.asarray(nodes, np.int64), Kn, Ka, np.float32(maxd), np.float32(c)


# ------------------------------------------------------------------------------------------------ the point graph
def pair_distances(points):
    """[n, n] float32: sqrt((dx dx + dy dy) + dz dz), every operation rounded to float32 (cloud.h:46, .cpp:62)"""
    p = np.asarray(points, np.float32)
    d = p[:, None, :] - p[None, :, :]
    s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    with np.errstate(invalid="ignore"):
        return np.sqrt(s)


def edges(points, max_distance):
    """-> (src, dst, length): every ordered pair i != k with d(i, k) < max_distance, ascending in (i, k)"""
    d = pair_distances(points)
    with np.errstate(invalid="ignore"):
        adj = d < np.float32(max_distance)
    np.fill_diagonal(adj, False)
    src, dst = np.nonzero(adj)
    return src, dst, d[src, dst]


def _limit(node_coverage):
    return 2.0 * float(np.float32(node_coverage))             # .cpp:137: a double


def heap_reach(points, node_indices, max_distance, node_coverage):
    """the reference's loop (.cpp:102-143) -> G [M, n] float32"""
    n = len(points)
    src, dst, length = edges(points, max_distance)
    start = np.searchsorted(src, np.arange(n + 1))
    lim = _limit(node_coverage)
    G = np.full((len(node_indices), n), np.inf, np.float32)
    for i, node in enumerate(node_indices):
        if not 0 <= node < n:
            continue
        heap, seen = [(np.float32(0.0), -int(node))], np.zeros(n, bool)       # min-heap of (g, -point) = max-heap of (-g, point)
        while heap:
            g, x = heapq.heappop(heap)
            x = -x
            if seen[x]:
                continue
            seen[x] = True
            G[i, x] = g
            for e in range(start[x], start[x + 1]):
                y = dst[e]
                if seen[y]:
                    continue
                nxt = np.float32(g + length[e])
                if float(nxt) > lim:
                    continue
                heapq.heappush(heap, (nxt, -int(y)))
    return G


def fixed_point_reach(points, node_indices, max_distance, node_coverage, order=None, in_place=False):
    """relaxation to the least fixed point -> G [M, n] float32.  order: a permutation of the edges to relax in; in_place: relax edge by edge
    in that order, each relaxation seeing the ones before it (Gauss-Seidel), instead of all edges at once from the last round's lengths
    (Jacobi).  The result must depend on neither."""
    n = len(points)
    src, dst, length = edges(points, max_distance)
    if order is not None:
        src, dst, length = src[order], dst[order], length[order]
    lim = _limit(node_coverage)
    G = np.full((len(node_indices), n), np.inf, np.float32)
    for i, node in enumerate(node_indices):
        if not 0 <= node < n:
            continue
        g = G[i]
        g[node] = 0.0
        while in_place:
            changed = False
            for x, y, d in zip(src, dst, length):
                if np.isfinite(g[x]):
                    cand = np.float32(g[x] + d)
                    if float(cand) <= lim and cand < g[y]:
                        g[y], changed = cand, True
            if not changed:
                break
        while not in_place:
            cand = (g[src] + length).astype(np.float32)
            ok = np.isfinite(g[src]) & (cand.astype(np.float64) <= lim)
            new = g.copy()
            np.minimum.at(new, dst[ok], cand[ok])
            if np.array_equal(new, g):
                break
            g[:] = new
    return G


# ------------------------------------------------------------------------------------------------ the six arrays
def weight(g, node_coverage):
    """compute_skinning_weight (.cpp:9-11): g g in float32, the rest in double, rounded once"""
    g = np.asarray(g, np.float32)
    c = np.float64(np.float32(node_coverage))
    return np.exp(-(g * g).astype(np.float64) / (2.0 * c * c)).astype(np.float32)


def weight_f64(g, node_coverage):
    """the same formula with g g in double as well: what the float32 weights are measured against"""
    g = np.asarray(g, np.float64)
    c = np.float64(np.float32(node_coverage))
    return np.exp(-(g * g) / (2.0 * c * c))


def weight_bar(want, dev):
    """per element: one float32 ulp of the expected weight, or 4 x the recorded deviation of the reference's float32 weights from float64"""
    return np.maximum(np.spacing(np.abs(np.asarray(want, np.float32))).astype(np.float64), 4.0 * float(dev))


def tables(G, node_indices, num_neighbors, num_anchors, node_coverage, margins=None):
    """-> dict of the six arrays.  margins: a list that receives the relative gaps between consecutive entries of every sorted reach list through
    position K + 1 (the node's own 0 excepted), and the gaps of every g to the bound 2 c"""
    M, n = G.shape
    Kn, Ka = int(num_neighbors), int(num_anchors)
    node_indices = np.asarray(node_indices, np.int64)
    out = dict(neighbor_indices=np.full((M, Kn), -1, np.int64), neighbor_distances=np.zeros((M, Kn), np.float32),
               neighbor_weights=np.zeros((M, Kn), np.float32), anchor_indices=np.full((n, Ka), -1, np.int64),
               anchor_distances=np.zeros((n, Ka), np.float32), anchor_weights=np.zeros((n, Ka), np.float32))
    valid = (node_indices >= 0) & (node_indices < n)

    def gaps(sorted_g, K):
        if margins is None:
            return
        s = np.asarray(sorted_g[:K + 1], np.float64)
        for a, b in zip(s[:-1], s[1:]):
            if b > 0:
                margins.append((b - a) / b)

    for i in range(M):
        cand = [(G[i, node_indices[j]], -int(node_indices[j]), j) for j in range(M) if valid[j] and np.isfinite(G[i, node_indices[j]])]
        cand.sort()
        gaps([c[0] for c in cand], Kn)
        for k, (g, _, j) in enumerate(cand[:Kn]):
            out["neighbor_indices"][i, k], out["neighbor_distances"][i, k] = j, g
            out["neighbor_weights"][i, k] = weight(g, node_coverage)
    for x in range(n):
        col = G[:, x]
        who = np.nonzero(np.isfinite(col))[0]
        who = who[np.argsort(col[who], kind="stable")]                    # stable: equal g keep the ascending node order
        gaps(col[who], Ka)
        who = who[:Ka]
        if len(who) == 0:
            continue
        w = weight(col[who], node_coverage)
        total = np.float32(0.0)
        for v in w:
            total = np.float32(total + v)
        w = (w / total).astype(np.float32) if total > 0 else np.full(len(who), np.float32(1.0 / float(np.float32(len(who)))), np.float32)
        out["anchor_indices"][x, :len(who)], out["anchor_distances"][x, :len(who)], out["anchor_weights"][x, :len(who)] = who, col[who], w
    if margins is not None:
        fin = G[np.isfinite(G)].astype(np.float64)
        lim = _limit(node_coverage)
        margins.append(float(np.min(np.abs(fin / lim - 1.0), initial=np.inf)))
    return out


def geo_graph(points, node_indices, num_neighbors, num_anchors, max_distance, node_coverage, form="fixed_point"):
    reach = heap_reach if form == "heap" else fixed_point_reach
    return tables(reach(points, node_indices, max_distance, node_coverage), node_indices, num_neighbors, num_anchors, node_coverage)


def edge_list(neighbor_indices, neighbor_weights):
    """edge (i, j) for every valid neighbour j != i of node i, row-major -> ([E, 2] int64, [E] float32)"""
    M = neighbor_indices.shape[0]
    e = [(i, int(j), w) for i in range(M) for j, w in zip(neighbor_indices[i], neighbor_weights[i]) if 0 <= j < M and j != i]
    return (np.asarray([(a, b) for a, b, _ in e], np.int64).reshape(-1, 2), np.asarray([w for _, _, w in e], np.float32))


def screen(points, node_indices, Kn, Ka, max_distance, node_coverage):
    """the fixture's screen -> (pair margin, bound margin, list margin, G): the smallest relative distance of a pair length to max_distance, of a
    path length to 2 c, and between consecutive entries of a sorted reach list through position K + 1"""
    d = pair_distances(points).astype(np.float64)
    np.fill_diagonal(d, np.inf)
    pair = float(np.min(np.abs(d / float(max_distance) - 1.0), initial=np.inf))
    G = heap_reach(points, node_indices, max_distance, node_coverage)
    m = []
    tables(G, node_indices, Kn, Ka, node_coverage, margins=m)
    bound = m.pop()
    return pair, bound, (min(m) if m else np.inf), G
