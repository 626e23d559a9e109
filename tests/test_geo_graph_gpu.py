"""dr_geo_graph_f32 / dr_geo_graph_edges on the GPU against tests/golden/geo_graph.npz, which the reference's own program produced
(tools/golden/make_golden_geo_graph.py): indices and distances bit for bit, weights per element within max(one float32 ulp, 4 x the deviation
of the reference's float32 weights from the float64 formula, recorded in the fixture).  Every call is made twice and compared bit-equal."""
import os

import numpy as np
import pytest
import torch

from tests import geo_graph_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
NAMES = [s[0] for s in R.SCENES]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "geo_graph.npz"))


@pytest.fixture(scope="module")
def N():
    from diffreg_hip import nonrigid
    return nonrigid


def inputs(gold, name):
    Kn, Ka, maxd, c = gold[name + "/params"]
    return (torch.from_numpy(gold[name + "/points"]).to(DEV), torch.from_numpy(gold[name + "/node_indices"]).to(DEV), int(Kn), int(Ka),
            float(maxd), float(c))


def twice(N, *a, **kw):
    """the call made twice: the six arrays and the status must be bit-equal"""
    g1, g2 = N.geo_graph(*a, **kw), N.geo_graph(*a, **kw)
    for key in R.KEYS + ("status",):
        assert torch.equal(g1[key], g2[key]), key
    return g1


def check_scene(got, gold, name, rows=None, nrows=None):
    """got: the call's dict; rows / nrows: the slices of the stacked point / node rows that hold this scene"""
    worst = 0.0
    for key in R.KEYS:
        want = gold[name + "/" + key]
        sl = (rows if "anchor" in key else nrows) or slice(None)
        g = got[key][sl].cpu().numpy()
        assert g.shape == want.shape and g.dtype == want.dtype, (name, key)
        if "weights" in key:
            bar = R.weight_bar(want, gold[name + "/weight_dev"][int("anchor" in key)])
            err = np.abs(g.astype(np.float64) - want)
            worst = max(worst, float((err / bar).max(initial=0.0)))
            print("%s %s: largest error / bar %.3f" % (name, key, float((err / bar).max(initial=0.0))))
            assert np.all(err <= bar), (name, key, float((err / bar).max()))
        else:
            # torch.equal's comparison: by value.  The one entry whose bits differ is a node's own distance: the reference pops -(0.) = -0.0
            # from its heap (.cpp:106, :113), the device returns +0.0
            assert torch.equal(torch.from_numpy(g), torch.from_numpy(want)), (name, key)
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_fixture_scene(N, gold, name):
    pts, idx, Kn, Ka, maxd, c = inputs(gold, name)
    g = twice(N, pts, idx, Kn, Ka, maxd, c)
    assert int(g["status"][0]) == 0
    check_scene(g, gold, name)
    d = N.build_deformation_graph_from_point_cloud(pts, idx, Kn, Ka, maxd, c)
    assert tuple(d) == R.KEYS and all(torch.equal(d[k], g[k]) for k in R.KEYS)


def test_sheets_do_not_share_nodes_where_the_euclidean_graph_does(N, gold):
    pts, idx, Kn, Ka, maxd, c = inputs(gold, "sheets")
    upper = pts[:, 2] > 0.03                              # the sheets lie at z = 0 and z = 0.06, jittered by 0.004
    node_upper = upper[idx]
    g = N.geo_graph(pts, idx, Kn, Ka, maxd, c)
    ai = g["anchor_indices"]
    assert bool((ai >= 0).any(1).all())
    crosses = lambda a: ((a >= 0) & (node_upper[a.clamp(min=0)] != upper[:, None])).any()
    assert not bool(crosses(ai))
    ni = g["neighbor_indices"]
    assert not bool(((ni >= 0) & (node_upper[ni.clamp(min=0)] != node_upper[:, None])).any())
    e = N.ed_graph(pts, pts[idx].contiguous(), Ka, c)
    assert bool(crosses(e["anchor_indices"]))            # the gap (0.06) is below 2 c (0.1): nodes of the other sheet are among the nearest in space


def test_ragged_call_of_three_clouds_one_without_nodes(N, gold):
    names = ("n65", "ustrip", "sparse")
    ins = [inputs(gold, n) for n in names]
    pts = torch.cat([ins[0][0], ins[1][0][:130], ins[2][0]])          # the middle cloud has points and no node
    idx = torch.cat([ins[0][1], ins[2][1]])
    pl, ml = [65, 130, 200], [len(ins[0][1]), 0, 3]
    maxd, c = ins[2][4], ins[2][5]
    g = twice(N, pts, idx, 8, 6, maxd, c, point_lengths=pl, node_lengths=ml)
    assert g["status"].tolist() == [0, 0, 0]
    assert bool((g["anchor_indices"][65:195] == -1).all()) and bool((g["anchor_weights"][65:195] == 0).all())
    check_scene(g, gold, "sparse", rows=slice(195, 395), nrows=slice(ml[0], ml[0] + 3))
    one = N.geo_graph(ins[0][0], ins[0][1], 8, 6, maxd, c)            # n65 under the call's parameters, alone
    for key in R.KEYS:
        sl = slice(0, 65) if "anchor" in key else slice(0, ml[0])
        assert torch.equal(g[key][sl], one[key]), key


@pytest.mark.parametrize("name,n", [("ustrip", 40), ("n65", 65), ("sheets", 800)])
def test_streamed_form_equals_the_onchip_form(N, gold, name, n):
    pts, idx, Kn, Ka, maxd, c = inputs(gold, name)
    pts = pts[:n].contiguous()
    idx = idx[idx < n].contiguous()
    assert len(idx) >= 1
    on = N.geo_graph(pts, idx, Kn, Ka, maxd, c)
    for cap in (n - 1, 8) if n > 40 else (39, 8):                     # one past the forced capacity, and far past it
        st = twice(N, pts, idx, Kn, Ka, maxd, c, onchip_cap_override=cap)
        for key in R.KEYS + ("status",):
            assert torch.equal(on[key], st[key]), (key, cap)
    at = N.geo_graph(pts, idx, Kn, Ka, maxd, c, onchip_cap_override=n)    # exactly at the forced capacity: still on chip
    assert all(torch.equal(on[k], at[k]) for k in R.KEYS)


def test_status_bits_and_ranges(N, gold):
    pts, idx, Kn, Ka, maxd, c = inputs(gold, "n65")
    M = len(idx)

    def in_range(g, n=65):
        assert bool(((g["neighbor_indices"] >= -1) & (g["neighbor_indices"] < M)).all())
        assert bool(((g["anchor_indices"] >= -1) & (g["anchor_indices"] < M)).all())
        for k in ("neighbor_distances", "neighbor_weights", "anchor_distances", "anchor_weights"):
            assert bool(torch.isfinite(g[k]).all()), k
    clean = N.geo_graph(pts, idx, Kn, Ka, maxd, c)
    bad = idx.clone()
    bad[1] = 65                                                       # out of range: an absent node
    g = twice(N, pts, bad, Kn, Ka, maxd, c)
    assert int(g["status"][0]) == R.ST_INDEX
    in_range(g)
    assert bool((g["neighbor_indices"][1] == -1).all()) and not bool((g["neighbor_indices"] == 1).any())
    assert not bool((g["anchor_indices"] == 1).any())
    want = R.geo_graph(pts.cpu().numpy(), bad.cpu().numpy(), Kn, Ka, np.float32(maxd), np.float32(c))
    assert np.array_equal(g["anchor_indices"].cpu().numpy(), want["anchor_indices"])
    assert np.array_equal(g["neighbor_indices"].cpu().numpy(), want["neighbor_indices"])
    nan = pts.clone()
    victim = int((torch.arange(65, device=DEV)[:, None] != idx[None]).all(1).nonzero()[0])      # a point that is no node
    nan[victim, 1] = float("nan")
    g = twice(N, nan, idx, Kn, Ka, maxd, c)
    assert int(g["status"][0]) == R.ST_NONFINITE
    in_range(g)
    assert bool((g["anchor_indices"][victim] == -1).all())            # no edges: nothing reaches it
    dup = idx.clone()
    dup[2] = dup[0]
    g = twice(N, pts, dup, Kn, Ka, maxd, c)
    assert int(g["status"][0]) == R.ST_DUPLICATE
    in_range(g)
    g = N.geo_graph(pts, idx, Kn, Ka, maxd, c, max_degree=1)          # denser than the adjacency row: flagged, padding only, never cut silently
    assert int(g["status"][0]) == R.ST_DEGREE
    assert bool((g["anchor_indices"] == -1).all()) and bool((g["neighbor_indices"] == -1).all())
    again = N.geo_graph(pts, idx, Kn, Ka, maxd, c)
    assert all(torch.equal(clean[k], again[k]) for k in R.KEYS) and int(again["status"][0]) == 0


def test_edge_list_against_the_plain_statement(N, gold):
    for name in ("sheets", "sparse", "isolated", "m1"):
        pts, idx, Kn, Ka, maxd, c = inputs(gold, name)
        g = N.geo_graph(pts, idx, Kn, Ka, maxd, c)
        ei, ew, el = N.geo_graph_edges(g["neighbor_indices"], g["neighbor_weights"])
        e, w = R.edge_list(g["neighbor_indices"].cpu().numpy(), g["neighbor_weights"].cpu().numpy())
        assert el == [len(e)] and np.array_equal(ei.cpu().numpy(), e) and np.array_equal(ew.cpu().numpy(), w), name
    # ragged, more rows than one chunk of the edge kernel, indices out of range and repeated selves
    rng = np.random.default_rng(3)
    ml = [300, 0, 5, 257]
    ni = torch.from_numpy(rng.integers(-1, 12, (sum(ml), 4))).to(DEV)
    nw = torch.from_numpy(rng.uniform(0, 1, (sum(ml), 4)).astype(np.float32)).to(DEV)
    ei, ew, el = N.geo_graph_edges(ni, nw, node_lengths=ml)
    ei2, ew2, _ = N.geo_graph_edges(ni, nw, node_lengths=ml)
    assert torch.equal(ei, ei2) and torch.equal(ew, ew2)
    lo = eo = 0
    for m, cnt in zip(ml, el):
        e, w = R.edge_list(ni[lo:lo + m].cpu().numpy(), nw[lo:lo + m].cpu().numpy())
        assert cnt == len(e) and np.array_equal(ei[eo:eo + cnt].cpu().numpy(), e) and np.array_equal(ew[eo:eo + cnt].cpu().numpy(), w)
        lo, eo = lo + m, eo + cnt


def test_capture_and_replay(N, gold):
    pts, idx, Kn, Ka, maxd, c = inputs(gold, "ustrip")
    eager = N.geo_graph(pts, idx, Kn, Ka, maxd, c)
    out = N.geo_graph(pts, idx, Kn, Ka, maxd, c)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for k in R.KEYS:
            out[k].fill_(7)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            N.geo_graph(pts, idx, Kn, Ka, maxd, c, out=out)
        graph.replay()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for k in R.KEYS + ("status",):
        assert torch.equal(out[k], eager[k]), k


def test_registration_moves_one_sheet_only(N, gold):
    """Matches translate the upper sheet by 0.03 along x and leave no match on the lower one.  Geodesic graph: no node of the lower sheet is
    tied to the upper one, so the lower sheet's points stay where they were to float32 rounding.  Euclidean graph: the lower sheet is skinned
    to the upper sheet's nodes as well and is dragged along.  Observed on one MI355X: the lower sheet moves by 0 (geodesic) and by 2.9e-2
    (euclidean); the upper sheet follows its matches by 0.0300 of 0.03."""
    pts = torch.from_numpy(gold["sheets/points"]).to(DEV)
    upper = pts[:, 2] > 0.03
    rows = upper.nonzero()[:, 0]
    tgt = pts.clone()
    tgt[upper, 0] += 0.03
    matches = torch.stack([rows, rows], 1).contiguous()
    # eps=0: the warp divides by (weight sum + eps), and the default 1e-6 alone would shrink an unmoved point by |p| 1e-6, above rounding
    kw = dict(num_anchors=6, node_coverage=0.05, node_sampler="fps", solver="gauss_newton", num_iterations=5, eps=0.0)
    geo = N.NonRigidRegistration(graph="geodesic", num_neighbors=8, max_distance=0.035, **kw)
    wg, _, gg = geo(pts, tgt, matches)
    wg2, _, _ = geo(pts, tgt, matches)
    assert torch.equal(wg, wg2)
    assert int(gg["status"]) == 0 and gg["edge_indices"].shape[1] == 2
    moved_geo = float((wg[~upper] - pts[~upper]).norm(dim=1).max())
    pulled = float((wg[upper] - pts[upper])[:, 0].mean())
    we, _, _ = N.NonRigidRegistration(graph="euclidean", **kw)(pts, tgt, matches)
    moved_euc = float((we[~upper] - pts[~upper]).norm(dim=1).max())
    print("lower sheet: geodesic moves it by %.3e, euclidean by %.3e; upper sheet follows its matches by %.4f of 0.03" % (moved_geo, moved_euc, pulled))
    assert moved_geo <= 8 * float(np.spacing(np.float32(0.4)))        # rounding of the warp's float64 sum to float32 at coordinates below 0.4
    assert pulled > 0.02
    assert moved_euc > 1e-3                                           # three orders above rounding: the Euclidean graph drags the other sheet
