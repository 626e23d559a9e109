"""GPU checks of the furthest-point sampling entries (csrc/fps.hip) against the reference's recorded lists (tests/golden/fps.npz: vision3d's
native_furthest_point_sample and sample_nodes_with_fps) and, at the edges the fixture cannot hold, against tests/fps_ref.py, which states the
device's tie rule (lowest index) and non-finite rule.  Every comparison is torch.equal / array_equal on indices, counts and bit patterns: there
is no tolerance.  Every call is made twice and must be bit-equal."""
import os

import numpy as np
import pytest
import torch

from tests import fps_ref as F
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "fps.npz"))


@pytest.fixture(scope="module")
def nr():
    from diffreg_hip import nonrigid
    return nonrigid


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def run_nodes(nr, clouds, md, ns, cap=None):
    """the ragged call, twice, bit-equal -> dict of host arrays"""
    lens = [len(c) for c in clouds]
    pts = dev(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds]) if clouds else np.zeros((0, 3)))
    a = nr.fps_nodes(pts, md, ns, lengths=lens, sample_cap=cap, return_distance=True)
    b = nr.fps_nodes(pts, md, ns, lengths=lens, sample_cap=cap, return_distance=True)
    for k in ("indices", "points", "distances", "counts", "status"):
        assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                           b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), k
    return {k: a[k].cpu().numpy() for k in ("indices", "points", "distances", "counts", "status")}


def check_against_statement(got, clouds, md, ns, cap=None):
    for p, c in enumerate(clouds):
        c = np.asarray(c, np.float32).reshape(-1, 3)
        idx, dist, st = F.nodes(c, md, ns, sample_cap=got["indices"].shape[1])
        k = len(idx)
        assert got["counts"][p] == k and got["status"][p] == st, (p, got["counts"][p], k, got["status"][p], st)
        assert np.array_equal(got["indices"][p, :k], idx) and np.all(got["indices"][p, k:] == -1), p
        assert np.array_equal(got["points"][p, :k].view(np.uint32), c[idx].view(np.uint32)) and np.all(got["points"][p, k:] == 0), p
        assert np.array_equal(got["distances"][p, :k].view(np.uint32), dist.view(np.uint32)) and np.all(got["distances"][p, k:] == 0), p


@pytest.mark.parametrize("scene", [s[0] for s in F.SCENES])
def test_fixture_scene(nr, gold, scene):
    _, n, _, md, ns = next(s for s in F.SCENES if s[0] == scene)
    pts = gold[scene + "/points"]
    got = run_nodes(nr, [pts], md, ns)
    want = gold[scene + "/indices"]
    k = len(want)
    assert got["counts"][0] == k and got["status"][0] == 0
    assert np.array_equal(got["indices"][0, :k], want) and np.all(got["indices"][0, k:] == -1)
    assert np.array_equal(got["points"][0, :k].view(np.uint32), pts[want].view(np.uint32))
    assert np.array_equal(got["distances"][0, :k].view(np.uint32), gold[scene + "/distances"].view(np.uint32))
    one = nr.furthest_point_sample_nodes(dev(pts), md, ns)
    assert one.dtype == torch.int64 and np.array_equal(one.cpu().numpy(), want)


def test_all_scenes_in_one_ragged_call(nr, gold):
    """clouds of different sizes side by side, with the stop rules of the last scene"""
    clouds = [gold[s[0] + "/points"] for s in F.SCENES]
    check_against_statement(run_nodes(nr, clouds, 0.06, 512), clouds, 0.06, 512)


@pytest.mark.parametrize("B,N,M", [(1, 1, 1), (3, 64, 64), (2, 65, 7), (2, 1025, 33), (1, 5, 9)])
def test_batch_form(nr, B, N, M):
    rng = np.random.default_rng(7 * N + M)
    pts = rng.uniform(-1, 1, (B, N, 3)).astype(np.float32)
    want = F.batch(pts, M)
    a = nr.furthest_point_sample(dev(pts), M, gather_points=False)
    b = nr.furthest_point_sample(dev(pts), M, gather_points=False)
    assert a.dtype == torch.int64 and tuple(a.shape) == (B, M) and torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), want)
    feats = torch.arange(B * 4 * N, dtype=torch.float32, device=DEV).reshape(B, 4, N)
    sp, sf = nr.furthest_point_sample(dev(pts), M, feats)
    assert np.array_equal(sp.cpu().numpy(), np.take_along_axis(pts, want[:, :, None], 1))
    assert np.array_equal(sf.cpu().numpy(), np.take_along_axis(feats.cpu().numpy(), want[:, None, :].repeat(4, 1), 2))
    spt, = nr.furthest_point_sample(dev(pts).transpose(1, 2).contiguous(), M, transposed=True)
    assert torch.equal(spt, sp.transpose(1, 2))


def lattice():
    return np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), np.arange(3.0), indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * 0.25


def test_edges(nr):
    rng = np.random.default_rng(3)
    u = lambda n: rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    empty = np.zeros((0, 3), np.float32)
    for clouds in ([empty, u(70), u(5)], [u(70), empty, u(5)], [u(70), u(5), empty], [empty]):
        check_against_statement(run_nodes(nr, clouds, 0.2, 16), clouds, 0.2, 16)
    assert nr.fps_nodes(torch.zeros(0, 3, device=DEV), 0.1, lengths=[])["indices"].shape[0] == 0          # P = 0
    same = np.tile(u(1), (40, 1))
    got = run_nodes(nr, [same], 0.1, None)
    assert got["counts"][0] == 1
    check_against_statement(got, [same], 0.1, None)
    got = run_nodes(nr, [same], None, 5)                    # no stop rule bites: the cloud is used up after its one distinct point
    assert got["counts"][0] == 1
    lat = lattice()
    for md, ns in ((None, 40), (0.3, None), (0.26, 75)):    # exact ties at every selection: the lowest index wins
        check_against_statement(run_nodes(nr, [lat, lat[::-1].copy()], md, ns), [lat, lat[::-1].copy()], md, ns)
    small = u(9)
    got = run_nodes(nr, [small], None, 20)                  # num_samples >= N
    assert got["counts"][0] == 9 and sorted(got["indices"][0, :9]) == list(range(9))
    check_against_statement(got, [small], None, 20)
    got = run_nodes(nr, [u(200), u(3)], 0.05, None, cap=8)  # the sample_cap bit: the first cloud is cut, the second is not
    assert list(got["status"]) == [F.ST_CAP, 0] and list(got["counts"]) == [8, 3]
    got = run_nodes(nr, [u(200)], 0.05, 8, cap=8)           # cut by num_samples: no bit
    assert got["status"][0] == 0 and got["counts"][0] == 8
    bad = u(130)
    bad[64] = [np.nan, 0, 0]
    bad[129] = [0, np.inf, 0]
    other = u(10)
    got = run_nodes(nr, [bad, other], None, 130)
    assert list(got["status"]) == [F.ST_NONFINITE, 0] and got["counts"][0] == 128
    assert 64 not in got["indices"][0] and 129 not in got["indices"][0]
    check_against_statement(got, [bad, other], None, 130)
    bad0 = u(20)
    bad0[0, 2] = np.nan
    got = run_nodes(nr, [bad0, other], 0.1, None)
    assert got["status"][0] == F.ST_NONFINITE | F.ST_START and got["counts"][0] == 0 and np.all(got["indices"][0] == -1)
    check_against_statement(got, [bad0, other], 0.1, None)
    bpts = u(12)[None].copy()
    bpts[0, 5, 1] = np.nan
    assert np.array_equal(nr.furthest_point_sample(dev(bpts), 14, gather_points=False).cpu().numpy(), F.batch(bpts, 14))


def test_refusals_leave_outputs_untouched(nr):
    from diffreg_hip.lib import ptr, raw, stream_of
    pts = dev(np.random.default_rng(0).uniform(-1, 1, (50, 3)))
    off = torch.tensor([0, 50], dtype=torch.int32, device=DEV)
    idx = torch.full((1, 8), 77, dtype=torch.int64, device=DEV)
    out_p, out_d = torch.full((1, 8, 3), 5.0, device=DEV), torch.full((1, 8), 5.0, device=DEV)
    cnt, st = torch.full((1,), 77, dtype=torch.int32, device=DEV), torch.full((1,), 77, dtype=torch.int32, device=DEV)
    cap = nr.fps_onchip_capacity()
    call = lambda P=1, n=50, mx=50, md=0.1, ns=-1, c=8, o=off, ws=None, wsb=0: raw().dr_fps_nodes_f32(
        P, n, mx, ptr(pts), ptr(o) if o is not None else None, md, ns, c, ptr(idx), ptr(out_p), ptr(out_d), ptr(cnt), ptr(st), ws, wsb,
        stream_of(pts))
    assert call(md=-1.0) == -1 and call(md=0.0) == -1 and call(c=0) == -1 and call(mx=51) == -1 and call(o=None) == -1 and call(n=-1) == -1
    assert call(P=70000) == -3
    raw().dr_debug_fps_force_streaming(1)
    try:
        assert raw().dr_fps_workspace_bytes(1, 50, 50) >= 200
        assert call() == -4 and call(ws=ptr(pts), wsb=16) == -4
    finally:
        raw().dr_debug_fps_force_streaming(0)
    bidx = torch.full((2, 4), 77, dtype=torch.int64, device=DEV)
    assert raw().dr_fps_batch_f32(2, 0, 4, ptr(pts), ptr(bidx), None, 0, stream_of(pts)) == -1
    assert raw().dr_fps_batch_f32(2, cap + 1, 4, ptr(pts), ptr(bidx), None, 0, stream_of(pts)) == -4
    torch.cuda.synchronize()
    assert torch.all(idx == 77) and torch.all(out_p == 5) and torch.all(out_d == 5) and torch.all(cnt == 77) and torch.all(st == 77)
    assert torch.all(bidx == 77)


def test_streaming_form_agrees_entry_for_entry(nr, gold):
    """both instantiations on the 1 025-point scene, on a ragged batch, and on the batch form: the typed debug setter forces the streaming
    one (a cloud of dr_fps_onchip_capacity() + 1 points would take many seconds of sampling to reach)"""
    from diffreg_hip.lib import raw
    pts = gold["n1025/points"]
    clouds = [pts, pts[:100], np.zeros((0, 3), np.float32), lattice()]
    bp = np.random.default_rng(11).uniform(-1, 1, (2, 1025, 3)).astype(np.float32)
    chip = run_nodes(nr, clouds, 0.1, 300)
    chip_b = nr.furthest_point_sample(dev(bp), 33, gather_points=False)
    raw().dr_debug_fps_force_streaming(1)
    try:
        assert raw().dr_fps_workspace_bytes(4, 2200, 1025) >= 4 * 2200
        stream = run_nodes(nr, clouds, 0.1, 300)
        stream_b = nr.furthest_point_sample(dev(bp), 33, gather_points=False)
    finally:
        raw().dr_debug_fps_force_streaming(0)
    for k in chip:
        assert np.array_equal(chip[k].view(np.uint32) if chip[k].dtype == np.float32 else chip[k],
                              stream[k].view(np.uint32) if stream[k].dtype == np.float32 else stream[k]), k
    assert torch.equal(chip_b, stream_b)
    check_against_statement(stream, clouds, 0.1, 300)


def test_capacity_and_one_more(nr):
    """a cloud of exactly the on-chip capacity and one of capacity + 1 points (which streams by itself), a few selections each"""
    cap = nr.fps_onchip_capacity()
    rng = np.random.default_rng(5)
    for n in (cap, cap + 1):
        pts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
        check_against_statement(run_nodes(nr, [pts, pts[:7]], None, 12), [pts, pts[:7]], None, 12)


def test_graph_capture_replays_equal_the_eager_result(nr, gold):
    pts = dev(gold["n1025/points"])
    eager = nr.fps_nodes(pts, 0.25, 64, return_distance=True)
    out = nr.fps_nodes(pts, 0.25, 64, return_distance=True)      # the buffers the captured call writes into
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        for k in ("indices", "points", "distances", "counts", "status"):
            out[k].zero_()
        with torch.cuda.graph(g, stream=s):
            nr.fps_nodes(pts, 0.25, 64, return_distance=True, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        for k in ("indices", "points", "distances", "counts", "status"):
            out[k].zero_()
        g.replay()
        torch.cuda.synchronize()
        for k in ("indices", "points", "distances", "counts", "status"):
            assert torch.equal(out[k], eager[k]), k


def test_registration_with_fps_nodes(nr):
    from diffreg_hip import synth
    torch.manual_seed(0)
    src_l, tgt_l, mat_l = [], [], []
    for seed, n in ((1, 1500), (2, 1100)):
        p = torch.from_numpy(F.scene_points(n, "surface", seed)).to(DEV)
        src_l.append(p)
        tgt_l.append((p + torch.tensor([0.02, -0.01, 0.03], device=DEV)).contiguous())
        rows = torch.arange(0, n, 3, device=DEV)
        mat_l.append(torch.stack([rows, rows], 1).contiguous())
    md = 0.12
    reg = nr.NonRigidRegistration(node_coverage=md, num_iterations=20, node_sampler="fps")
    warped, T, graphs = reg(src_l, tgt_l, mat_l)
    for src, w, g in zip(src_l, warped, graphs):
        nodes = g["nodes"]
        M = nodes.shape[0]
        assert 1 < M <= nr.node_capacity() and int(g["status"]) == 0
        assert (nodes[:, None, :] == src[None]).all(-1).any(1).all()                  # every node is a row of the source cloud, bit for bit
        dist64 = lambda a, b: (a.double()[:, None, :] - b.double()[None]).norm(dim=-1)   # by differences: exact to float64 rounding
        d_ps = dist64(src, nodes)
        d_nn = dist64(nodes, nodes) + torch.eye(M, device=DEV, dtype=torch.float64) * 10
        assert d_nn.min() >= np.float32(md) - 1e-7                                    # the float32 stop test, seen in float64
        assert d_ps.min(dim=1).values.max() < np.float32(md) + 1e-7                   # covering: every point within min_distance of a node
        assert w.shape == src.shape and torch.isfinite(w).all()
    grid = nr.NonRigidRegistration(node_coverage=md, num_iterations=20)
    grid2 = nr.NonRigidRegistration(node_coverage=md, num_iterations=20, node_sampler="grid")
    wa, Ta, _ = grid(src_l, tgt_l, mat_l)
    wb, Tb, _ = grid2(src_l, tgt_l, mat_l)
    assert all(torch.equal(a, b) for a, b in zip(wa, wb)) and all(torch.equal(a, b) for a, b in zip(Ta, Tb))
    capped = nr.NonRigidRegistration(node_coverage=md, node_min_distance=0.004, num_iterations=2, node_sampler="fps")
    _, _, gc = capped(src_l[1], tgt_l[1], mat_l[1])
    assert gc["nodes"].shape[0] == nr.node_capacity() and int(gc["status"]) & nr.FPS_CAP_REACHED
