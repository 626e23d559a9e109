"""GPU checks of the non-rigid ICP entries (csrc/nonrigid.hip) through the C ABI, against the reference's recorded float64 outputs
(tests/golden/nonrigid.npz).

The bar (tests/nonrigid_ref.ratio <= 1): per tensor, the deviation from the reference's float64 is at most max(one float32 ulp at the tensor's largest
magnitude, 4 x the reference's own recorded float32 deviation); integer outputs are equal.  Every comparison prints its ratio before it asserts."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import nonrigid_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("rot", "trn", "m_rot", "m_trn", "v_rot", "v_trn")
STATE_OF = dict(rot="rotations", trn="translations", m_rot="exp_avg_rot", m_trn="exp_avg_trn", v_rot="exp_avg_sq_rot", v_trn="exp_avg_sq_trn")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "nonrigid.npz"))


@pytest.fixture(scope="module")
def nr():
    from diffreg_hip import nonrigid
    return nonrigid


def dev(a):
    a = np.asarray(a)
    return torch.from_numpy(a.astype(np.float32) if a.dtype.kind == "f" else a.astype(np.int64)).to(DEV).contiguous()


def host(t):
    return t.detach().cpu().numpy()


def held(what, got, ref64, dev32=None):
    r = R.ratio(host(got) if isinstance(got, torch.Tensor) else got, ref64, dev32)
    print("%-44s deviation / bar = %.3f" % (what, r))
    assert r <= 1.0, (what, r)
    return r


def problem_of(nr, gold, name):
    s = R.scene_inputs(gold, name)
    return nr.Problem(dev(s["nodes"]), dev(s["src"]), dev(s["tgt"]), dev(s["ai"]), dev(s["aw"]), dev(s["edges"]), dev(s["ew"])), s


@pytest.fixture(scope="module")
def runs(nr, gold):
    """the free-running device solver on every scene, once: {name: {n: (state dict, trace or None)}}"""
    out = {}
    for name in R.SCENES:
        pb, _ = problem_of(nr, gold, name)
        out[name] = {}
        for n in R.STEPS:
            st = nr.new_state(pb)
            T, cost, tr, status = nr.nicp_adam(pb, num_iterations=n, state=st, trace=(n == R.STEPS[-1]))
            assert int(status.abs().sum()) == 0
            out[name][n] = (st, T, tr)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------------------------------------ graph
@pytest.mark.parametrize("name", ("a", "b", "c", "d"))
def test_graph(nr, gold, name):
    sc = R.make_scene(name)
    g = nr.ed_graph(dev(sc["cloud"]), dev(sc["nodes"]), sc["K"], sc["coverage"], return_distance=True)
    assert int(g["status"].abs().sum()) == 0
    ke = min(sc["K"], sc["nodes"].shape[0])
    assert np.array_equal(host(g["anchor_indices"])[:, :ke], gold[name + "_graph_anchor_indices"])
    assert (host(g["anchor_indices"])[:, ke:] == -1).all() and (host(g["anchor_weights"])[:, ke:] == 0).all()
    assert np.array_equal(host(g["edge_indices"]), gold[name + "_graph_edge_indices"])
    for k in ("anchor_weights", "anchor_distances"):
        held("%s graph %s" % (name, k), g[k][:, :ke], gold["%s_graph_%s" % (name, k)], gold["%s_graph_%s_dev32" % (name, k)])
    for k in ("edge_weights", "edge_distances"):
        held("%s graph %s" % (name, k), g[k], gold["%s_graph_%s" % (name, k)], gold["%s_graph_%s_dev32" % (name, k)])
    # the drop-in name returns the reference's tuple, with min(K, M) columns
    t = nr.build_euclidean_deformation_graph(dev(sc["cloud"]), dev(sc["nodes"]), sc["K"], sc["coverage"])
    assert len(t) == 4 and t[0].shape[1] == ke and torch.equal(t[0], g["anchor_indices"][:, :ke]) and torch.equal(t[3], g["edge_weights"])


def test_graph_with_non_finite_coordinates(nr):
    """a NaN / Inf coordinate anchors nothing and touches no bit of the map: the other rows and the edge list equal the clean run's"""
    sc = R.make_scene("c")
    clean = nr.ed_graph(dev(sc["cloud"]), dev(sc["nodes"]), sc["K"], sc["coverage"], return_distance=True)
    assert int(clean["status"][0]) == 0
    # (1) one NaN point and one Inf point added to the cloud, as pair 1 of a batch whose pair 0 is clean (a stray bit would land in pair 0's rows)
    bad = np.concatenate([sc["cloud"][:150], [[np.nan, 0.0, 0.0]], sc["cloud"][150:], [[0.0, np.inf, 0.0]]]).astype(np.float32)
    g = nr.ed_graph(dev(np.concatenate([sc["cloud"], bad])), dev(np.concatenate([sc["nodes"], sc["nodes"]])), sc["K"], sc["coverage"],
                    point_lengths=[300, 302], node_lengths=[40, 40], return_distance=True)
    assert g["status"].tolist() == [0, 8] and g["edge_lengths"] == clean["edge_lengths"] * 2
    keep = torch.tensor([i for i in range(302) if i not in (150, 301)], device=DEV) + 300
    E = clean["edge_lengths"][0]
    for k in ("anchor_indices", "anchor_weights", "anchor_distances"):
        assert torch.equal(g[k][:300], clean[k]) and torch.equal(g[k][keep], clean[k]), k
    for k in ("edge_indices", "edge_weights", "edge_distances"):
        assert torch.equal(g[k][:E], clean[k]) and torch.equal(g[k][E:], clean[k]), k
    for row in (300 + 150, 300 + 301):
        assert (g["anchor_indices"][row] == -1).all() and (g["anchor_weights"][row] == 0).all() and (g["anchor_distances"][row] == 0).all()
    # the same cloud alone, as pair 0: the unfilled slots must not reach in front of the workspace
    g0 = nr.ed_graph(dev(bad), dev(sc["nodes"]), sc["K"], sc["coverage"])
    assert int(g0["status"][0]) == 8 and torch.equal(g0["edge_indices"], clean["edge_indices"]) and torch.equal(g0["edge_weights"], clean["edge_weights"])
    # (2) M <= K with a non-finite node: scene (b)'s two nodes, the second NaN -- one anchor per point, weight 1, one self edge
    sb = R.make_scene("b")
    nodes = sb["nodes"].copy()
    nodes[1, 2] = np.nan
    gb = nr.ed_graph(dev(sb["cloud"]), dev(nodes), sb["K"], sb["coverage"])
    assert int(gb["status"][0]) == 8
    assert (gb["anchor_indices"][:, 0] == 0).all() and (gb["anchor_indices"][:, 1:] == -1).all()
    assert (gb["anchor_weights"][:, 0] == 1).all() and (gb["anchor_weights"][:, 1:] == 0).all()
    assert gb["edge_indices"].tolist() == [[0, 0]] and torch.isfinite(gb["edge_weights"]).all()


# ------------------------------------------------------------------------------------------------ warp, cost and gradient at the recorded states
@pytest.mark.parametrize("name", R.SCENES)
def test_warp_cost_gradient(nr, gold, name):
    pb, s = problem_of(nr, gold, name)
    M = s["nodes"].shape[0]
    for n in R.STATES:
        rot = np.tile(np.eye(3), (M, 1, 1)) if n == 0 else gold["%s_adam%d_rot" % (name, n)]
        trn = np.zeros((M, 3)) if n == 0 else gold["%s_adam%d_trn" % (name, n)]
        g = lambda k: (gold["%s_state%d_%s" % (name, n, k)], gold["%s_state%d_%s_dev32" % (name, n, k)])
        cost, g_r, g_t, status = nr.nicp_cost_grad(pb, dev(rot), dev(trn))
        assert int(status.abs().sum()) == 0
        held("%s state %d cost" % (name, n), cost[0], *g("cost"))
        held("%s state %d grad_rot" % (name, n), g_r, *g("grad_rot"))
        held("%s state %d grad_trn" % (name, n), g_t, *g("grad_trn"))
        T = dev(R.to_transforms(rot, trn))
        w, st = nr.ed_warp(dev(s["cloud"]), dev(s["nodes"]), T, dev(s["all_ai"]), dev(s["all_aw"]))
        held("%s state %d warp" % (name, n), w, *g("warp"))
        wc = nr.apply_deformation(dev(s["src"]), dev(s["nodes"]), T, dev(s["ai"]), dev(s["aw"]))
        held("%s state %d warp of correspondences" % (name, n), wc, *g("warp_corr"))
        if name == "e":
            assert (host(wc)[5] == 0).all()


# ------------------------------------------------------------------------------------------------ solver
@pytest.mark.parametrize("name", R.SCENES)
def test_solver_teacher_forced(nr, gold, name):
    """from the reference's float64 state after 1 and after 10 iterations, one device iteration lands on the reference's state after 2 and 11"""
    pb, s = problem_of(nr, gold, name)
    for n in (1, 10):
        st = {STATE_OF[k]: dev(gold["%s_adam%d_%s" % (name, n, k)]) for k in KEYS}
        st["step"] = torch.full((1,), n, dtype=torch.int32, device=DEV)
        nr.nicp_adam(pb, num_iterations=1, state=st, resume=True)
        assert int(st["step"][0]) == n + 1
        for k in KEYS:
            held("%s teacher-forced %d -> %d %s" % (name, n, n + 1, k), st[STATE_OF[k]], gold["%s_adam%d_%s" % (name, n + 1, k)],
                 gold["%s_adam%d_%s_dev32" % (name, n + 1, k)])


@pytest.mark.parametrize("name", R.SCENES)
def test_solver_free_running(nr, gold, runs, name):
    for n in R.STEPS:
        st, T, tr = runs[name][n]
        for k in KEYS:
            held("%s free-running %d %s" % (name, n, k), st[STATE_OF[k]], gold["%s_adam%d_%s" % (name, n, k)], gold["%s_adam%d_%s_dev32" % (name, n, k)])
        assert torch.equal(T[:, :3, :3], st["rotations"]) and torch.equal(T[:, :3, 3], st["translations"])
        assert torch.equal(T[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV).expand(T.shape[0], 4))
    held("%s cost trace" % name, runs[name][R.STEPS[-1]][2][0], gold[name + "_trace"], gold[name + "_trace_dev32"])


def test_resume_is_bit_equal(nr, gold, runs):
    pb, _ = problem_of(nr, gold, "c")
    st = nr.new_state(pb)
    nr.nicp_adam(pb, num_iterations=10, state=st)
    T, _, _, _ = nr.nicp_adam(pb, num_iterations=40, state=st, resume=True)
    ref, Tr, _ = runs["c"][50]
    assert int(st["step"][0]) == 50 and torch.equal(T, Tr)
    for k in STATE_OF.values():
        assert torch.equal(st[k], ref[k]), k
    # a negative resumed step count is taken as 0 and reported (status bit 16), not turned into a zero bias correction
    neg = nr.new_state(pb)
    neg["step"].fill_(-3)
    Tn, _, _, status = nr.nicp_adam(pb, num_iterations=50, state=neg, resume=True)
    assert int(status[0]) == 16 and int(neg["step"][0]) == 50 and torch.equal(Tn, Tr)


def test_two_runs_and_a_graph_replay_are_bit_equal(nr, gold, runs):
    pb, _ = problem_of(nr, gold, "c")
    T1, c1, _, _ = nr.nicp_adam(pb, num_iterations=50)
    assert torch.equal(T1, runs["c"][50][1])
    out = pb.last_out
    T2, c1 = T1.clone(), c1.clone()                         # T1 and c1 are the buffers the replay writes into
    for t in out[:2]:
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nr.nicp_adam(pb, num_iterations=50, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], T2) and torch.equal(out[1], c1)


def test_batch_equals_single_pairs(nr, gold, runs):
    """scene (f): (b) + (c) in one ragged call, graph, solver and warp"""
    sb, sc = R.make_scene("b"), R.make_scene("c")
    cloud = dev(np.concatenate([sb["cloud"], sc["cloud"]]))
    nodes = dev(np.concatenate([sb["nodes"], sc["nodes"]]))
    pl, ml = [sb["cloud"].shape[0], sc["cloud"].shape[0]], [sb["nodes"].shape[0], sc["nodes"].shape[0]]
    g = nr.ed_graph(cloud, nodes, 4, sc["coverage"], point_lengths=pl, node_lengths=ml, return_distance=True)
    gc = nr.ed_graph(dev(sc["cloud"]), dev(sc["nodes"]), 4, sc["coverage"], return_distance=True)
    assert g["edge_lengths"][1] == gc["edge_lengths"][0]
    for k in ("anchor_indices", "anchor_weights", "anchor_distances"):
        assert torch.equal(g[k][pl[0]:], gc[k]), k
    for k in ("edge_indices", "edge_weights", "edge_distances"):
        assert torch.equal(g[k][g["edge_lengths"][0]:], gc[k]), k
    ins = [R.scene_inputs(gold, n) for n in ("b", "c")]
    cat = lambda k: dev(np.concatenate([s[k] for s in ins]))
    ai = np.concatenate([np.pad(ins[0]["ai"], ((0, 0), (0, 2)), constant_values=-1), ins[1]["ai"]])      # (b) has min(4, 2) = 2 columns
    aw = np.concatenate([np.pad(ins[0]["aw"], ((0, 0), (0, 2))), ins[1]["aw"]])
    pb = nr.Problem(cat("nodes"), cat("src"), cat("tgt"), dev(ai), dev(aw), cat("edges"), cat("ew"), node_lengths=ml,
                    corr_lengths=[s["src"].shape[0] for s in ins], edge_lengths=[s["edges"].shape[0] for s in ins])
    st = nr.new_state(pb)
    T, cost, _, status = nr.nicp_adam(pb, num_iterations=50, state=st)
    assert int(status.abs().sum()) == 0 and st["step"].tolist() == [50, 50]
    assert torch.equal(T[:ml[0]], runs["b"][50][1]) and torch.equal(T[ml[0]:], runs["c"][50][1])
    for k in STATE_OF.values():
        assert torch.equal(st[k][:ml[0]], runs["b"][50][0][k]) and torch.equal(st[k][ml[0]:], runs["c"][50][0][k]), k
    w, _ = nr.ed_warp(cat("src"), cat("nodes"), T, dev(ai), dev(aw), point_lengths=pb.cl, node_lengths=ml)
    wc = nr.apply_deformation(dev(ins[1]["src"]), dev(ins[1]["nodes"]), runs["c"][50][1], dev(ins[1]["ai"]), dev(ins[1]["aw"]))
    assert torch.equal(w[pb.cl[0]:], wc)


def raw_adam(nr, pb, n, T, wsb_delta=0, max_nodes=None):
    """dr_nicp_adam_f32 itself, with a workspace size or a max_nodes the wrapper would not pass -> the entry's return code"""
    from diffreg_hip import lib
    s = pb.struct()
    if max_nodes is not None:
        s = type(s).from_buffer_copy(s)
        s.max_nodes = max_nodes
    ws, wsb = pb.workspace()
    op = lib.NicpOptions(n, 0.5, 0.999, 0.9, 0.999, 1e-8, 1.0, 0.1, 0.1)
    status = torch.zeros(pb.P, dtype=torch.int32, device=DEV)
    return lib.raw().dr_nicp_adam_f32(ctypes.byref(s), ctypes.byref(op), None, 0, lib.ptr(T), None, None, lib.ptr(status), lib.ptr(ws),
                                      wsb + wsb_delta, lib.stream_of(T))


def test_plumbing(nr, gold, runs):
    pb, s = problem_of(nr, gold, "c")
    M = s["nodes"].shape[0]
    T = torch.full((M, 4, 4), 7.0, device=DEV)
    assert raw_adam(nr, pb, 50, T, wsb_delta=-1) == -4                                                      # DR_EWORKSPACE
    assert raw_adam(nr, pb, 50, T, max_nodes=nr.node_capacity() + 1) == -1                                  # DR_EINVAL
    torch.cuda.synchronize()
    assert (T == 7.0).all()                                 # a refused call leaves a poisoned output as it was
    assert raw_adam(nr, pb, 50, T) == 0                     # the size the query states is sufficient
    assert torch.equal(T, runs["c"][50][1])
    T0, cost0, _, _ = nr.nicp_adam(pb, num_iterations=0)
    assert torch.equal(T0, torch.eye(4, device=DEV).expand(M, 4, 4))
    held("c cost at identity (0 iterations)", cost0[0], gold["c_state0_cost"], gold["c_state0_cost_dev32"])
    assert torch.equal(nr.non_rigid_icp_adam(pb.nodes, pb.src, pb.tgt, pb.ai, pb.aw, pb.edges, pb.ew, num_iterations=50), runs["c"][50][1])


# ------------------------------------------------------------------------------------------------ scene (g): the capacity
def test_capacity(nr):
    """M = capacity runs: its gradient is float64 autograd's within the bar (the reference's float32 deviation here is float32 autograd's, computed
    below), four solver iterations equal Adam applied to the unfused gradient in all six state tensors, a captured graph replays them;
    M = capacity + 1 is refused"""
    cap = nr.node_capacity()
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-1, 1, (1100, 3)).astype(np.float32)
    nodes = cloud[rng.choice(1100, cap, replace=False)].copy()
    corr = np.sort(rng.choice(1100, 333, replace=False))
    tgt = (cloud[corr] + 0.1 * rng.standard_normal((333, 3))).astype(np.float32)
    g = nr.ed_graph(dev(cloud), dev(nodes), 6, 0.25)
    ai, aw = g["anchor_indices"][dev(corr)].contiguous(), g["anchor_weights"][dev(corr)].contiguous()
    pb = nr.Problem(dev(nodes), dev(cloud[corr]), dev(tgt), ai, aw, g["edge_indices"], g["edge_weights"])
    rot = (np.tile(np.eye(3), (cap, 1, 1)) + 0.05 * rng.standard_normal((cap, 3, 3))).astype(np.float32)
    trn = (0.05 * rng.standard_normal((cap, 3))).astype(np.float32)
    cost, g_r, g_t, status = nr.nicp_cost_grad(pb, dev(rot), dev(trn))
    assert int(status.abs().sum()) == 0
    grads = {}
    for dt in (torch.float64, torch.float32):
        c = lambda t: (t.detach().cpu().to(dt) if t.dtype.is_floating_point else t.detach().cpu())
        r, t = torch.from_numpy(rot).to(dt).requires_grad_(True), torch.from_numpy(trn).to(dt).requires_grad_(True)
        R.torch_cost(r, t, c(pb.nodes), c(pb.src), c(pb.tgt), c(ai), c(aw), c(pb.edges), c(pb.ew)).backward()
        grads[dt] = (r.grad.numpy().astype(np.float64), t.grad.numpy().astype(np.float64))
    held("capacity grad_rot vs float64 autograd", g_r, grads[torch.float64][0], grads[torch.float32][0] - grads[torch.float64][0])
    held("capacity grad_trn vs float64 autograd", g_t, grads[torch.float64][1], grads[torch.float32][1] - grads[torch.float64][1])
    # the fused solver EQUALS the unfused path: four iterations, each held to torch's Adam step in float64 (the statement of tests/nonrigid_ref.adam_run)
    # applied to dr_nicp_cost_grad_f32's gradient at the float32 state the fused run started that iteration from.  All six state tensors; bar: one
    # float32 ulp at the tensor's largest magnitude (both sides round a float64 value once; they may differ where it sits on a rounding boundary).
    st = nr.new_state(pb)
    st["rotations"].copy_(dev(rot)); st["translations"].copy_(dev(trn))
    start = {k: v.clone() for k, v in st.items()}
    lr, iters = R.ADAM["lr"], 4
    for it in range(1, iters + 1):
        before = {k: host(v).astype(np.float64) for k, v in st.items() if k != "step"}
        _, g_r, g_t, _ = nr.nicp_cost_grad(pb, st["rotations"], st["translations"])
        nr.nicp_adam(pb, num_iterations=1, state=st, resume=True)
        assert int(st["step"][0]) == it
        bc1, bc2 = 1.0 - R.ADAM["beta1"] ** it, 1.0 - R.ADAM["beta2"] ** it
        for tag, gd in (("rot", g_r), ("trn", g_t)):
            names = ("rotations", "exp_avg_rot", "exp_avg_sq_rot") if tag == "rot" else ("translations", "exp_avg_trn", "exp_avg_sq_trn")
            gd = host(gd).astype(np.float64)
            m = before[names[1]] + (gd - before[names[1]]) * (1.0 - R.ADAM["beta1"])
            v = before[names[2]] * R.ADAM["beta2"] + (1.0 - R.ADAM["beta2"]) * gd * gd
            pnew = before[names[0]] - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + R.ADAM["eps"])
            for name, want in zip(names, (pnew, m, v)):
                held("capacity iteration %d %s vs Adam on the unfused gradient" % (it, name), st[name], want)
        lr = lr * R.ADAM["gamma"]
    # the same four iterations in one launch (the two state copies alternate inside it), eagerly and replayed from a captured graph: bit-equal
    one = {k: v.clone() for k, v in start.items()}
    T4 = nr.nicp_adam(pb, num_iterations=iters, state=one, resume=True)[0].clone()
    for k in st:
        assert torch.equal(one[k], st[k]), k
    again = {k: v.clone() for k, v in start.items()}
    out = pb.last_out
    out[0].fill_(float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nr.nicp_adam(pb, num_iterations=iters, state=again, resume=True, out=out)
    for k in again:
        again[k].copy_(start[k])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], T4)
    for k in st:
        assert torch.equal(again[k], st[k]), k
    T = torch.full((cap, 4, 4), 7.0, device=DEV)
    assert raw_adam(nr, pb, 1, T, max_nodes=cap + 1) == -1
    with pytest.raises(ValueError, match="at most"):
        nr.Problem(dev(np.zeros((cap + 1, 3), np.float32)), pb.src, pb.tgt, ai, aw, pb.edges, pb.ew)
    torch.cuda.synchronize()
    assert (T == 7.0).all()


# ------------------------------------------------------------------------------------------------ the 4DMatch convenience
def test_nonrigid_registration(nr, gold):
    sc = R.make_scene("c")
    src, nodes, tgt = dev(sc["cloud"]), dev(sc["nodes"]), dev(sc["tgt"])
    matches = torch.stack([dev(sc["corr"]), torch.arange(tgt.shape[0], device=DEV)], 1)
    reg = nr.NonRigidRegistration(num_anchors=sc["K"], node_coverage=sc["coverage"], num_iterations=50)
    warped, T, graph = reg(src, tgt, matches, nodes=nodes)
    g = nr.ed_graph(src, nodes, sc["K"], sc["coverage"])
    pb = nr.Problem(nodes, src[matches[:, 0]], tgt, g["anchor_indices"][matches[:, 0]].contiguous(), g["anchor_weights"][matches[:, 0]].contiguous(),
                    g["edge_indices"], g["edge_weights"])
    T2 = nr.nicp_adam(pb, num_iterations=50)[0]
    assert torch.equal(T, T2) and torch.equal(graph["edge_indices"], g["edge_indices"])
    assert torch.equal(warped, nr.ed_warp(src, nodes, T2, g["anchor_indices"], g["anchor_weights"])[0])
    # a list of pairs in one call, nodes grid-subsampled from the source
    reg2 = nr.NonRigidRegistration(num_anchors=4, node_coverage=0.5, num_iterations=10)
    ws, Ts, graphs = reg2([src, src[:200].contiguous()], [tgt, tgt], [matches, matches[matches[:, 0] < 200].contiguous()])
    assert len(ws) == 2 and ws[0].shape == src.shape and ws[1].shape == (200, 3) and Ts[0].shape[0] == graphs[0]["nodes"].shape[0]
    one = reg2(src, tgt, matches)
    assert torch.equal(one[0], ws[0]) and torch.equal(one[1], Ts[0])
