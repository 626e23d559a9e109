"""CPU checks of tests/geo_graph_ref.py, the float32 statement of vision3d's build_deformation_graph_from_point_cloud that the GPU tests lean
on: both of its forms (the reference's heap procedure, and the relaxation to a fixed point that the device runs) have to reproduce every array
the reference's own program produced (tests/golden/geo_graph.npz) and each other on random unscreened graphs in any relaxation order; the
edge-list rule is held against a plain statement; and the library has to refuse what it documents -- the refusals come before any launch, so
they need no GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import geo_graph_ref as R
from tests.conftest import GOLDEN

NAMES = [s[0] for s in R.SCENES]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "geo_graph.npz"))


def test_fixture_is_screened_and_covers_the_cases(gold):
    for name in NAMES:
        assert np.all(gold[name + "/margins"] > 1e-5), (name, gold[name + "/margins"])
        pts, nodes, Kn, Ka, maxd, c = R.scene(name, int(gold[name + "/seed"]))
        assert np.array_equal(pts, gold[name + "/points"]) and np.array_equal(nodes, gold[name + "/node_indices"])
        assert list(gold[name + "/params"]) == [Kn, Ka, float(maxd), float(c)]
    ai = gold["nonode/anchor_indices"]
    assert np.all(ai[300:] == -1) and np.any(ai[:300] >= 0)                   # a component with no node: rows of -1
    assert np.all(gold["sparse/neighbor_indices"][:, 3:] == -1) and np.all(gold["sparse/anchor_indices"][:, 3:] == -1)
    assert list(gold["isolated/neighbor_indices"][0]) == [0, -1, -1, -1]      # an isolated node: only itself
    assert np.array_equal(gold["isolated/anchor_indices"][200], [0, -1, -1])
    assert gold["m1/neighbor_indices"].shape == (1, 8) and gold["n1/anchor_indices"].shape == (1, 2)


@pytest.mark.parametrize("form", ["heap", "fixed_point"])
@pytest.mark.parametrize("name", NAMES)
def test_statement_reproduces_the_reference(gold, name, form):
    Kn, Ka, maxd, c = gold[name + "/params"]
    got = R.geo_graph(gold[name + "/points"], gold[name + "/node_indices"], int(Kn), int(Ka), np.float32(maxd), np.float32(c), form=form)
    for key in R.KEYS:
        want = gold[name + "/" + key]
        if "weights" in key:      # numpy's exp against the C library's: exact, or within the GPU tests' bar
            bar = R.weight_bar(want, gold[name + "/weight_dev"][int("anchor" in key)])
            assert np.all(np.abs(got[key].astype(np.float64) - want) <= bar), (key,)
        else:
            assert got[key].dtype == want.dtype and np.array_equal(got[key], want), (key,)


@pytest.mark.parametrize("seed", range(4))
def test_relaxation_in_any_order_is_the_heap_procedure(seed):
    """the fixed-point argument: float32 addition is monotone, so Dijkstra with the reference's pruning settles the least fixed point of
    g(y) = min(g(y), fl(g(x) + d(x, y))), whatever order the relaxations run in -- on unscreened graphs, quantised so that ties are common"""
    rng = np.random.default_rng(seed)
    n = 120
    pts = (np.round(rng.uniform(0, 0.5, (n, 3)) * [1, 1, 0.1] * 64) / 64).astype(np.float32)       # a lattice: many equal lengths and sums
    nodes = rng.choice(n, 9, replace=False)
    maxd, c = np.float32(0.09), np.float32(0.11)
    heap = R.heap_reach(pts, nodes, maxd, c)
    E = len(R.edges(pts, maxd)[0])
    assert E > 4 * n and np.isfinite(heap).sum() > 3 * len(nodes)
    for order, in_place in ((None, False), (None, True), (rng.permutation(E), True), (np.arange(E)[::-1], True)):
        G = R.fixed_point_reach(pts, nodes, maxd, c, order=order, in_place=in_place)
        assert np.array_equal(G.view(np.uint32), heap.view(np.uint32)), in_place
    assert np.all(heap[np.isfinite(heap)].astype(np.float64) <= 2.0 * float(c)) and np.all(heap[np.arange(9), nodes] == 0)


def test_edge_list_rule():
    ni = np.array([[0, 2, 1, -1], [1, 0, -1, -1], [2, 2, 0, 7], [3, -1, -1, -1]], np.int64)      # a repeated self, an index out of range
    nw = np.arange(16, dtype=np.float32).reshape(4, 4)
    e, w = R.edge_list(ni, nw)
    assert e.tolist() == [[0, 2], [0, 1], [1, 0], [2, 0]] and w.tolist() == [1.0, 2.0, 5.0, 10.0]
    e, w = R.edge_list(np.full((3, 2), -1, np.int64), np.zeros((3, 2), np.float32))
    assert e.shape == (0, 2) and w.shape == (0,)


def test_library_has_the_entries_and_refuses_before_any_launch():
    from diffreg_hip import lib
    raw = lib.raw()
    for name in ("dr_geo_graph_f32", "dr_geo_graph_edges", "dr_geo_graph_workspace_bytes", "dr_geo_graph_onchip_capacity"):
        assert hasattr(raw, name), name
    cap = raw.dr_geo_graph_onchip_capacity()
    assert cap >= 9000
    assert raw.dr_geo_graph_workspace_bytes(0, 10, 2, 10, 8) == 0
    assert raw.dr_geo_graph_workspace_bytes(1, 100, 7, 100, 16) >= 100 * 8 * (1 + 16) + 7 * 100 * 4
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call below is refused on the host
    EINVAL, ENOSUP, EWORKSPACE = -1, -3, -4

    def graph(P=1, n=10, m=2, mxp=10, mxn=2, pts=fake, po=fake, ni=fake, no=fake, Kn=4, Ka=3, maxd=0.1, c=0.2, D=8, ov=0, out=fake, st=fake,
              ws=fake, wsb=1 << 20, op=True):
        o = lib.GeoGraphOptions(Kn, Ka, maxd, c, D, ov)
        return raw.dr_geo_graph_f32(P, n, m, mxp, mxn, pts, po, ni, no, ctypes.byref(o) if op else None, out, out, out, out, out, out, st, ws, wsb,
                                    None)
    assert graph(P=0) == 0
    for kw in (dict(P=-1), dict(n=-1), dict(m=-1), dict(mxp=11), dict(mxn=3), dict(pts=None), dict(po=None), dict(ni=None), dict(no=None),
               dict(out=None), dict(st=None), dict(op=False), dict(Kn=0), dict(Ka=0), dict(Kn=9), dict(Ka=9), dict(maxd=0.0),
               dict(maxd=float("nan")), dict(c=-1.0), dict(c=float("inf")), dict(D=0), dict(ov=-1), dict(ws=ctypes.c_void_p(4100))):
        assert graph(**kw) == EINVAL, kw
    for kw in (dict(P=70000), dict(m=3000, mxn=2049), dict(D=1025)):
        assert graph(**kw) == ENOSUP, kw
    assert graph(ws=None) == EWORKSPACE and graph(wsb=16) == EWORKSPACE

    def edges(P=1, m=4, Kn=4, ni=fake, nw=fake, no=fake, cnt=fake, eo=None, cap_=0, ei=None, ew=None):
        return raw.dr_geo_graph_edges(P, m, Kn, ni, nw, no, cnt, eo, cap_, ei, ew, None)
    assert edges(P=0) == 0
    for kw in (dict(P=-1), dict(m=-1), dict(Kn=0), dict(Kn=9), dict(ni=None), dict(no=None), dict(cnt=None), dict(cap_=-1),
               dict(eo=fake, cap_=5, ei=None), dict(eo=fake, cap_=5, ei=fake, ew=fake, nw=None)):
        assert edges(**kw) == EINVAL, kw
    assert edges(P=70000) == ENOSUP


def test_python_refusals():
    import torch
    from diffreg_hip import nonrigid
    pts, idx = torch.zeros(6, 3), torch.zeros(2, dtype=torch.int64)
    for kw in (dict(num_neighbors=0), dict(num_neighbors=9), dict(num_anchors=0), dict(num_anchors=9), dict(max_distance=0.0),
               dict(node_coverage=-1.0), dict(max_degree=0), dict(onchip_cap_override=-1), dict(point_lengths=[5]),
               dict(point_lengths=[3, 3], node_lengths=[2])):
        a = dict(num_neighbors=4, num_anchors=3, max_distance=0.1, node_coverage=0.2)
        a.update(kw)
        with pytest.raises(ValueError):
            nonrigid.geo_graph(pts, idx, **a)
    with pytest.raises(TypeError):
        nonrigid.geo_graph(pts.double(), idx, 4, 3, 0.1, 0.2)
    with pytest.raises(TypeError):
        nonrigid.geo_graph(pts, idx.int(), 4, 3, 0.1, 0.2)
    for call in (lambda: nonrigid.geo_graph(pts, idx, 4, 3, 0.1, 0.2),
                 lambda: nonrigid.build_deformation_graph_from_point_cloud(pts, idx, 4, 3, 0.1, 0.2),
                 lambda: nonrigid.geo_graph_edges(torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 4))):
        with pytest.raises(TypeError, match="on the GPU"):   # a host tensor's pointer is never handed to a kernel
            call()
    with pytest.raises(ValueError, match="node_sampler='fps'"):
        nonrigid.NonRigidRegistration(graph="geodesic")                       # the grid sampler's nodes are no points of the cloud
    for kw in (dict(graph="mesh"), dict(graph="geodesic", node_sampler="fps", num_neighbors=9),
               dict(graph="geodesic", node_sampler="fps", max_distance=0.0)):
        with pytest.raises(ValueError):
            nonrigid.NonRigidRegistration(**kw)
    reg = nonrigid.NonRigidRegistration()
    assert reg.graph == "euclidean" and reg.node_sampler == "grid"
    assert nonrigid.NonRigidRegistration(graph="geodesic", node_sampler="fps", node_coverage=0.08).max_distance == 0.04
