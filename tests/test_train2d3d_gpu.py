"""2D-3D training branch on the device (dr_fusion_layer_*, dr_l2_normalize_*, dr_circle_loss_*; diffreg_hip.autograd2d3d, overlay2d3d with
training=True) against the reference's own float32 / float64 backward (tests/golden/train2d3d_branch.npz, minted by
tools/golden/make_golden_train2d3d.py), and -- at sizes no fixture holds -- against float64 / float32 torch autograd through the restatement in
tests/train2d3d_ref.py (pinned to that fixture and to oracle/diffreg_oracle.py by tests/test_train2d3d_oracle.py).  Needs a GPU.

Bar per gradient tensor (tests/test_train_gpu.py): |dev - ref64| <= max(1e-3 max|ref64|, 2 max|ref32 - ref64|); conf_matrix_gt_hat 1e-4;
losses 1e-5 relative to float64 (or twice the float32 reference's own distance).  A gradient that vanishes in exact arithmetic -- the key
projection's bias: softmax is invariant to the shift q . b_k of a query's scores -- is rounding noise in every float32 computation; that tensor
alone is held absolutely, at 1e-6 of the largest gradient of the same backward (`floor_for`)."""
import numpy as np
import pytest
import torch

from oracle import diffreg_oracle as orc
from tests import train2d3d_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bar(dev, r32, r64, what, floor=0.0):
    dev, r32, r64 = (torch.as_tensor(a).detach().double().cpu() for a in (dev, r32, r64))
    assert dev.shape == r64.shape, (what, dev.shape, r64.shape)
    M = float(r64.abs().max())
    e, r = float((dev - r64).abs().max()), float((r32 - r64).abs().max())
    assert e <= max(1e-3 * M, 2 * r, floor, 1e-12), (what, "device %.3e from float64, float32 torch %.3e, tensor max %.3e" % (e, r, M))


def floor_for(name, grads64):
    """the absolute bar of the key projection's bias gradient (zero in exact arithmetic); every other tensor: none"""
    if not name.endswith("attention.attention.k_token_layer.bias"):
        return 0.0
    return 1e-6 * max(float(torch.as_tensor(g).abs().max()) for g in grads64.values())


# ---- the layer alone --------------------------------------------------------------------------------------------------------------------------
def _layer(C, H, seed):
    torch.manual_seed(seed)
    layer = R.TransformerLayer(C, H)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if "norm" in n:
                p.add_(0.1 * torch.randn_like(p))
            elif n.endswith("bias"):
                p.copy_(0.1 * torch.randn_like(p))
    return layer


def _layer_case(layer, L, S, self_call, masked, seed, dtype, dev_path):
    import copy
    g = torch.Generator().manual_seed(seed)
    C = layer.output.norm.weight.shape[0]
    x0 = torch.randn(1, L, C, generator=g)
    y0 = x0 if self_call else torch.randn(1, S, C, generator=g)
    valid = (torch.rand(1, y0.shape[1], generator=g) > 0.3) if masked else None
    if valid is not None:
        valid[0, 0] = True
    go = torch.randn(1, L, C, generator=g)
    m = copy.deepcopy(layer).to(device=DEV, dtype=dtype)
    x = x0.to(DEV, dtype).requires_grad_(True)
    y = x if self_call else y0.to(DEV, dtype).requires_grad_(True)
    vm = None if valid is None else valid.to(DEV)
    if dev_path:
        from diffreg_hip import autograd2d3d
        out = autograd2d3d.fusion_layer(m, x, y, vm)
    else:
        out = m(x, y, y, k_masks=None if vm is None else ~vm)
    out.backward(go.to(DEV, dtype))
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters()}
    grads["x"] = x.grad.detach().clone()
    if not self_call:
        grads["y"] = y.grad.detach().clone()
    return out.detach(), grads


@pytest.mark.parametrize("L,S,self_call,masked", [(5, 7, False, False), (7, 7, True, False), (5, 7, False, True), (257, 255, False, True),
                                                  (255, 255, True, True), (1530, 1024, False, False), (1024, 1530, False, False),
                                                  (1530, 1530, True, False)])
def test_layer_against_float64_autograd(L, S, self_call, masked):
    layer = _layer(256, 4, 3)
    d_out, d_g = _layer_case(layer, L, S, self_call, masked, 11, torch.float32, True)
    o32, g32 = _layer_case(layer, L, S, self_call, masked, 11, torch.float32, False)
    o64, g64 = _layer_case(layer, L, S, self_call, masked, 11, torch.float64, False)
    bar(d_out, o32, o64, "out")
    assert sorted(d_g) == sorted(g64)
    for n in g64:
        bar(d_g[n], g32[n], g64[n], n, floor_for(n, g64))


def test_layer_small_width():
    """C = 64, H = 4 (d = 16): the LayerNorm backward's narrowest lane layout"""
    layer = _layer(64, 4, 5)
    d_out, d_g = _layer_case(layer, 33, 17, False, True, 12, torch.float32, True)
    o32, g32 = _layer_case(layer, 33, 17, False, True, 12, torch.float32, False)
    o64, g64 = _layer_case(layer, 33, 17, False, True, 12, torch.float64, False)
    bar(d_out, o32, o64, "out")
    for n in g64:
        bar(d_g[n], g32[n], g64[n], n, floor_for(n, g64))


def test_layer_restatement_is_the_oracles():
    """the test-side TransformerLayer is oracle.transformer_layer_2d3d (float64, on the GPU)"""
    layer = _layer(256, 4, 3).double().to(DEV)
    W = {"l." + k: v for k, v in layer.state_dict().items()}
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(1, 40, 256, generator=g).double().to(DEV), torch.randn(1, 50, 256, generator=g).double().to(DEV)
    with torch.no_grad():
        assert (layer(x, y, y) - orc.transformer_layer_2d3d(W, "l.", x, y, 4)).abs().max().item() < 1e-12


def test_layer_backward_is_bit_reproducible():
    layer = _layer(256, 4, 3)
    a = _layer_case(layer, 1530, 1024, False, False, 13, torch.float32, True)[1]
    b = _layer_case(layer, 1530, 1024, False, False, 13, torch.float32, True)[1]
    for n in a:
        assert torch.equal(a[n], b[n]), n


# ---- circle loss and normalisation ------------------------------------------------------------------------------------------------------------
def _circle_case(M, N, C, K, seed, clamp_rows=0):
    g = torch.Generator().manual_seed(seed)
    img = torch.nn.functional.normalize(torch.randn(M, C, generator=g), dim=1)
    pcd = torch.nn.functional.normalize(torch.randn(N, C, generator=g), dim=1)
    flat = torch.randperm(M * N, generator=g)[:K]
    ii, jj = (flat // N).long(), (flat % N).long()
    # correlate the listed pairs so that the positives carry informative weights
    for k in range(min(K, 64)):
        pcd[jj[k]] = torch.nn.functional.normalize(img[ii[k]] + 0.3 * pcd[jj[k]], dim=0)
    for k in range(clamp_rows):
        # the same row on both sides, 1 % longer than a unit row: 2 - 2 x y = -0.0402 in any precision -- the clamp is active at (ii[k], jj[k])
        img[ii[k]] = img[ii[k]] * 1.01
        pcd[jj[k]] = img[ii[k]]
    ov = torch.rand(K, generator=g)
    ov[:clamp_rows] = 0.1                  # the clamped pairs are negatives (overlap < 0.2): their entries carry a nonzero logit
    return img, pcd, ii, jj, ov


def _circle_ref(img, pcd, ii, jj, ov, dtype):
    lm = R.CoarseMatchingLoss()
    a, b = img.to(DEV, dtype).requires_grad_(True), pcd.to(DEV, dtype).requires_grad_(True)
    loss = lm.circle(a, b, dict(gt_img_node_corr_indices=ii.to(DEV), gt_pcd_node_corr_indices=jj.to(DEV), gt_node_corr_min_overlaps=ov.to(DEV)))
    loss.backward()
    return loss.detach(), a.grad, b.grad


@pytest.mark.parametrize("M,N,K", [(160, 96, 300), (37, 29, 40), (1530, 1024, 4000)])
def test_circle_loss_against_float64(M, N, K):
    from diffreg_hip import lib
    img, pcd, ii, jj, ov = _circle_case(M, N, 256, K, 21)
    prm = lib.circle_params(0.1, 1.4, 0.1, 1.4, 40.0, 0.3, 0.2)
    l64, gi64, gp64 = _circle_ref(img, pcd, ii, jj, ov, torch.float64)
    l32, gi32, gp32 = _circle_ref(img, pcd, ii, jj, ov, torch.float32)
    d = lambda t_: t_.to(DEV)
    loss = lib.circle_loss(d(img), d(pcd), d(ii), d(jj), d(ov), d(ov), prm)
    l2, gi, gp = lib.circle_loss_backward(d(img), d(pcd), d(ii), d(jj), d(ov), d(ov), prm)
    assert torch.isfinite(l64)
    assert abs(loss.item() - l64.item()) <= max(1e-5 * abs(l64.item()), 2 * abs(l32.item() - l64.item())) and l2.item() == loss.item()
    bar(gi, gi32, gi64, "grad_img")
    bar(gp, gp32, gp64, "grad_pcd")
    # the scale by grad_loss, and bit-reproducibility
    _, gi_b, _ = lib.circle_loss_backward(d(img), d(pcd), d(ii), d(jj), d(ov), d(ov), prm, torch.tensor(2.0, device=DEV))
    assert torch.allclose(gi_b, 2 * gi, rtol=1e-6, atol=0)
    assert torch.equal(lib.circle_loss_backward(d(img), d(pcd), d(ii), d(jj), d(ov), d(ov), prm)[1], gi)


def test_circle_loss_clamp_entries_get_no_gradient():
    """listed pairs with x . y > 1: clamp(2 - 2 x y, 0) is active there, and torch passes no gradient through those entries"""
    from diffreg_hip import lib
    img, pcd, ii, jj, ov = _circle_case(37, 29, 256, 40, 22, 5)
    d = lambda t_: t_.to(DEV)
    prm = lib.circle_params(0.1, 1.4, 0.1, 1.4, 40.0, 0.3, 0.2)
    l64, gi64, gp64 = _circle_ref(img, pcd, ii, jj, ov, torch.float64)
    _, gi, gp = lib.circle_loss_backward(d(img), d(pcd), d(ii), d(jj), d(ov), d(ov), prm)
    l32, gi32, gp32 = _circle_ref(img, pcd, ii, jj, ov, torch.float32)
    assert (2 - 2 * (img[ii[:5]] * pcd[jj[:5]]).sum(1) < -0.03).all() and (ov[:5] < 0.2).all()
    assert torch.isfinite(gi).all() and torch.isfinite(gp).all()
    bar(gi, gi32, gi64, "grad_img")
    bar(gp, gp32, gp64, "grad_pcd")


@pytest.mark.parametrize("K", [0, 3])
def test_circle_loss_empty_anchor_set(K):
    """no positives (K = 0), or positives without a row / column holding also a negative? -> the reference's NaN loss and torch's gradient"""
    from diffreg_hip import lib
    img, pcd, ii, jj, ov = _circle_case(20, 16, 64, max(K, 1), 23)
    ii, jj, ov = ii[:K], jj[:K], (ov[:K] * 0.0 + 0.1)            # overlap 0.1: not a positive (<= 0.3) -- every entry is a negative
    d = lambda t_: t_.to(DEV)
    prm = lib.circle_params(0.1, 1.4, 0.1, 1.4, 40.0, 0.3, 0.2)
    l64, gi64, gp64 = _circle_ref(img, pcd, ii, jj, ov, torch.float64)
    loss, gi, gp = lib.circle_loss_backward(d(img), d(pcd), d(ii), d(jj), d(ov), d(ov), prm)
    assert torch.isnan(l64) and torch.isnan(loss)
    assert torch.equal(gi.double().cpu(), gi64.cpu()) and torch.equal(gp.double().cpu(), gp64.cpu())


def test_normalize_forward_backward():
    from diffreg_hip import autograd2d3d
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(1530, 256, generator=g)
    x0[3] *= 1e-3
    x0[7] *= 1e-14                         # |x| < eps = 1e-12: y = x / eps, grad_x = g / eps (the clamp_min branch)
    go = torch.randn(1530, 256, generator=g)
    x = x0.to(DEV).requires_grad_(True)
    y = autograd2d3d.normalize(x)
    y.backward(go.to(DEV))
    x64 = x0.double().to(DEV).requires_grad_(True)
    y64 = torch.nn.functional.normalize(x64, p=2, dim=1)
    y64.backward(go.double().to(DEV))
    assert (y.double() - y64).abs().max().item() < 1e-6
    assert x64.norm(dim=1)[7].item() < 1e-12
    rest = torch.arange(1530, device=DEV) != 7
    assert (x.grad.double() - x64.grad)[rest].abs().max().item() <= 1e-5 * x64.grad[rest].abs().max().item()
    assert (x.grad.double() - x64.grad)[7].abs().max().item() <= 1e-6 * x64.grad[7].abs().max().item()


# ---- the whole coarse + denoising branch with its loss ----------------------------------------------------------------------------------------
def _host_and_loss():
    return R.load_synth(R.HostTrain2D3D()), R.CoarseMatchingLoss()


def _device_run(host, b, training=True):
    from diffreg_hip.overlay2d3d import accelerate, accelerate_loss
    hd, lm = R.clone_as(host, torch.float32, DEV), R.CoarseMatchingLoss()
    ov = accelerate(hd, training=training)
    undo = accelerate_loss(lm)
    hd.train()
    out = R.run_step(hd, lm, R.batch_to(b, DEV, torch.float32))
    ov.remove()
    undo()
    return out


def _branch_check(N, M, seed, nv=None, mv=None):
    host, _ = _host_and_loss()
    b = R.make_batch(N, M, seed, nv=nv, mv=mv)
    r64 = R.run_step(R.clone_as(host, torch.float64, DEV).train(), R.CoarseMatchingLoss(), R.batch_to(b, DEV, torch.float64))
    r32 = R.run_step(R.clone_as(host, torch.float32, DEV).train(), R.CoarseMatchingLoss(), R.batch_to(b, DEV, torch.float32))
    before = dict(R.calls)
    od, losses, grads = _device_run(host, b)
    assert R.calls == before, "an original forward ran under the training overlay"
    for k in range(4):
        l64 = float(r64[1][k])
        assert abs(float(losses[k]) - l64) <= 1e-5 * abs(l64), (k, float(losses[k]), l64)
    assert (od["conf_matrix_gt_hat"].double() - r64[0]["conf_matrix_gt_hat"]).abs().max().item() < 1e-4
    assert (od["conf_matrix_pred"].double() - r64[0]["conf_matrix_pred"]).abs().max().item() < 1e-4
    assert sorted(grads) == sorted(r64[2])
    for n in r64[2]:
        bar(grads[n], r32[2][n], r64[2][n], n, floor_for(n, r64[2]))
    return host, b, grads


def test_branch_against_reference_fixture(golden):
    """the device step (overlay + accelerate_loss) against the REFERENCE's modules and loss, float32 and float64 backward"""
    g = golden("train2d3d_branch")
    host, _ = _host_and_loss()
    b = R.make_batch(96, 160, 31, nv=90, mv=150)
    assert np.allclose(R.input_checksum(b), g["input_checksum"], rtol=1e-6, atol=0)      # (float32 rounding of the warp differs by CPU)
    before = dict(R.calls)
    od, losses, grads = _device_run(host, b)
    assert R.calls == before, "an original forward ran under the training overlay"
    for k in range(4):
        l64 = float(g["losses64"][k])
        assert abs(float(losses[k]) - l64) <= 1e-5 * abs(l64), (k, float(losses[k]), l64)
    assert np.abs(od["conf_matrix_gt_hat"][0].detach().double().cpu().numpy() - g["conf_gt_hat64"]).max() < 1e-4
    assert np.abs(od["conf_matrix_pred"][0].detach().double().cpu().numpy() - g["conf_pred64"]).max() < 1e-4
    g64 = {k[4:]: g[k] for k in g.files if k.startswith("g64_")}
    assert sorted(grads) == sorted(g64)
    for n in g64:
        bar(R.fixture_sub(grads[n]), g["g32_" + n], g64[n], n, floor_for(n, g64))


def test_branch_small_masked():
    _branch_check(96, 160, 31, nv=90, mv=150)


def test_branch_real_size():
    """N = 1024 point nodes, M = 34 x 45 = 1530 image tokens (EXP/model.py:172-173)"""
    _branch_check(1024, 1530, 32)


def test_overlay_flag_and_reproducibility():
    host, _ = _host_and_loss()
    b = R.make_batch(96, 160, 33)
    g1 = _device_run(host, b)[2]
    g2 = _device_run(host, b)[2]
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    # without training=True, train mode stays on the original code
    from diffreg_hip.overlay2d3d import accelerate
    hd = R.clone_as(host, torch.float32, DEV)
    ov = accelerate(hd)
    before = dict(R.calls)
    R.run_step(hd.train(), R.CoarseMatchingLoss(), R.batch_to(b, DEV, torch.float32))
    assert R.calls["fusion"] == before["fusion"] + 2 and R.calls["matching"] == before["matching"] + 2 and R.calls["loss"] == before["loss"] + 1
    ov.remove()
