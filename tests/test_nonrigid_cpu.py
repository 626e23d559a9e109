"""CPU checks of the non-rigid ICP path: the float64 numpy statement tests/nonrigid_ref.py reproduces the reference's recorded float64 outputs
(tests/golden/nonrigid.npz, minted by tools/golden/make_golden_nonrigid.py), and diffreg_hip.nonrigid imports and refuses without a device."""
import os

import numpy as np
import pytest
import torch

from tests import nonrigid_ref as R
from tests.conftest import GOLDEN

TOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "nonrigid.npz"))


scene_inputs = R.scene_inputs


@pytest.mark.parametrize("name", R.SCENES)
def test_inputs_are_the_scenes(gold, name):
    sc = R.make_scene(name)
    for k in ("cloud", "nodes", "corr", "tgt"):
        assert np.array_equal(gold["%s_in_%s" % (name, k)], sc[k])
    assert R.screen(sc["cloud"], sc["nodes"], sc["K"]) > 1e-5


@pytest.mark.parametrize("name", R.SCENES)
def test_graph_reproduces_reference(gold, name):
    sc = R.make_scene(name)
    g = R.build_graph(sc["cloud"], sc["nodes"], sc["K"], sc["coverage"])
    for k in ("anchor_indices", "edge_indices"):
        assert np.array_equal(g[k], gold["%s_graph_%s" % (name, k)])
    for k in ("anchor_weights", "anchor_distances", "edge_weights", "edge_distances"):
        assert np.abs(g[k] - gold["%s_graph_%s" % (name, k)]).max() <= TOL, k
    assert g["anchor_indices"].shape[1] == min(sc["K"], sc["nodes"].shape[0])
    if name == "e":
        held = R.holes(g["anchor_indices"][sc["corr"]])
        assert np.array_equal(held, gold["e_corr_anchor_indices"]) and (held[5] == -1).all()


@pytest.mark.parametrize("name", R.SCENES)
def test_cost_gradient_and_warp_reproduce_reference(gold, name):
    s = scene_inputs(gold, name)
    M = s["nodes"].shape[0]
    for n in R.STATES:
        rot = np.tile(np.eye(3), (M, 1, 1)) if n == 0 else gold["%s_adam%d_rot" % (name, n)]
        trn = np.zeros((M, 3)) if n == 0 else gold["%s_adam%d_trn" % (name, n)]
        terms, g_r, g_t = R.cost_grad(rot, trn, s["nodes"], s["src"], s["tgt"], s["ai"], s["aw"], s["edges"], s["ew"])
        assert np.abs(terms - gold["%s_state%d_cost" % (name, n)]).max() <= TOL
        assert np.abs(g_r - gold["%s_state%d_grad_rot" % (name, n)]).max() <= TOL
        assert np.abs(g_t - gold["%s_state%d_grad_trn" % (name, n)]).max() <= TOL
        T = R.to_transforms(rot, trn)
        assert np.abs(R.apply_deformation(s["cloud"], s["nodes"], T, s["all_ai"], s["all_aw"]) - gold["%s_state%d_warp" % (name, n)]).max() <= TOL
        w = R.apply_deformation(s["src"], s["nodes"], T, s["ai"], s["aw"])
        assert np.abs(w - gold["%s_state%d_warp_corr" % (name, n)]).max() <= TOL
        if name == "e":
            assert (w[5] == 0).all()                        # all anchors -1: scatter_add_ leaves the row at zero


@pytest.mark.parametrize("name", R.SCENES)
def test_solver_reproduces_reference(gold, name):
    s = scene_inputs(gold, name)
    states, trace = R.adam_run(s["nodes"], s["src"], s["tgt"], s["ai"], s["aw"], s["edges"], s["ew"], R.STEPS[-1])
    worst = 0.0
    for n in R.STEPS:
        for k, v in states[n].items():
            worst = max(worst, float(np.abs(v - gold["%s_adam%d_%s" % (name, n, k)]).max()))
    worst = max(worst, float(np.abs(trace - gold[name + "_trace"]).max()))
    print("scene %s: largest deviation of the numpy solver from the reference's float64 over 500 iterations %.2e" % (name, worst))
    assert worst <= TOL


def test_gradient_is_autograd(gold):
    s = scene_inputs(gold, "e")
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64 if a.dtype.kind == "f" else np.int64))
    rot = t(gold["e_adam10_rot"]).requires_grad_(True)
    trn = t(gold["e_adam10_trn"]).requires_grad_(True)
    R.torch_cost(rot, trn, t(s["nodes"]), t(s["src"]), t(s["tgt"]), t(s["ai"]), t(s["aw"]), t(s["edges"]), t(s["ew"])).backward()
    _, g_r, g_t = R.cost_grad(rot.detach().numpy(), trn.detach().numpy(), s["nodes"], s["src"], s["tgt"], s["ai"], s["aw"], s["edges"], s["ew"])
    assert np.abs(g_r - rot.grad.numpy()).max() <= TOL and np.abs(g_t - trn.grad.numpy()).max() <= TOL


def test_reference_float32_stays_within_the_fixture_condition(gold):
    for name in R.SCENES:
        for n in R.STEPS:
            for k in ("rot", "trn"):
                assert np.abs(gold["%s_adam%d_%s_dev32" % (name, n, k)]).max() <= 1e-4


# ------------------------------------------------------------------------------------------------ the module, without a device
def test_module_imports_and_states_capacity():
    from diffreg_hip import nonrigid
    assert nonrigid.node_capacity() >= 512
    for f in ("build_euclidean_deformation_graph", "apply_deformation", "non_rigid_icp_adam", "NonRigidRegistration"):
        assert hasattr(nonrigid, f)


def _cpu_problem(M=4, N=5, K=2, dtype=torch.float32):
    g = torch.Generator().manual_seed(1)
    nodes, src, tgt = (torch.rand(n, 3, generator=g).to(dtype) for n in (M, N, N))
    ai = torch.randint(0, M, (N, K), generator=g)
    aw = torch.rand(N, K, generator=g).to(dtype)
    edges = torch.stack([torch.arange(M), torch.arange(M)], 1)
    ew = torch.ones(M, dtype=dtype)
    return [nodes, src, tgt, ai, aw, edges, ew]


def test_refusals_raise_without_a_device():
    from diffreg_hip import nonrigid
    args = _cpu_problem()
    with pytest.raises(RuntimeError):                       # well-formed, but there is no CPU path
        nonrigid.non_rigid_icp_adam(*args, num_iterations=1)
    with pytest.raises(TypeError):
        nonrigid.non_rigid_icp_adam(*_cpu_problem(dtype=torch.float64), num_iterations=1)
    bad = list(args)
    bad[3] = torch.cat([args[3], args[3]], 1)[:, ::2]       # a strided view: not contiguous
    with pytest.raises(ValueError, match="contiguous"):
        nonrigid.non_rigid_icp_adam(*bad, num_iterations=1)
    bad = list(args)
    bad[3] = args[3].to(torch.int32)
    with pytest.raises(TypeError):
        nonrigid.non_rigid_icp_adam(*bad, num_iterations=1)
    with pytest.raises(ValueError, match="at most"):
        nonrigid.non_rigid_icp_adam(*_cpu_problem(M=nonrigid.node_capacity() + 1), num_iterations=1)
    with pytest.raises(NotImplementedError):
        nonrigid.build_euclidean_deformation_graph(args[1], args[0], 2, 0.5, return_adjacent_matrix=True)
    with pytest.raises(TypeError):
        nonrigid.build_euclidean_deformation_graph(args[1].double(), args[0], 2, 0.5)
    with pytest.raises(ValueError):
        nonrigid.build_euclidean_deformation_graph(args[1], args[0], 9, 0.5)
    with pytest.raises(ValueError, match="contiguous"):
        nonrigid.apply_deformation(args[1], args[0], torch.eye(4).repeat(4, 1, 1), bad[3].long()[:, :1].expand(5, 2), args[4])
    reg = nonrigid.NonRigidRegistration(num_anchors=2, node_coverage=0.5)
    with pytest.raises(ValueError, match="at most"):
        reg(args[1], args[2], torch.zeros(3, 2, dtype=torch.int64), nodes=torch.rand(nonrigid.node_capacity() + 1, 3))
