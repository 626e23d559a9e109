"""CPU checks behind tests/test_train2d3d_gpu.py: the test-side restatement of the 2D-3D training branch (tests/train2d3d_ref.py) reproduces the
REFERENCE's own forward and float32 / float64 backward (tests/golden/train2d3d_branch.npz, minted from Diff-Reg-2d3d's CrossModalFusionModule,
Matching and CoarseMatchingLoss by tools/golden/make_golden_train2d3d.py) -- so the GPU tests that use the restatement at sizes no fixture holds
hold the device to the reference -- and is the committed oracle's (oracle/diffreg_oracle.py: fusion_module, match_head_2d3d) in value and in
float64 gradient; the closed form of the circle loss's
gradient that csrc/circle_loss.hip evaluates (row / column softmax weights, softplus', -1 / D, the clamp) is torch autograd's on that restatement --
including the clamp and an empty anchor set (NaN loss, zero gradient)."""
import numpy as np
import torch

from oracle import diffreg_oracle as orc
from tests import train2d3d_ref as R

F64 = torch.float64
PRM = dict(pos_margin=0.1, neg_margin=1.4, pos_optimal=0.1, neg_optimal=1.4, log_scale=40.0, pos_overlap=0.3, neg_overlap=0.2)


def closed_form(img, pcd, ii, jj, ov, p=PRM):
    """numpy float64 statement of dr_circle_loss_backward_f32: -> (loss, d loss / d img, d loss / d pcd)"""
    img, pcd = img.numpy(), pcd.numpy()
    M, N = img.shape[0], pcd.shape[0]
    s = img @ pcd.T
    t = 2.0 - 2.0 * s
    D = np.sqrt(np.maximum(t, 0.0) + 1e-8)
    omin = np.zeros((M, N)); omin[ii.numpy(), jj.numpy()] = ov.numpy()
    pos, neg = omin > p["pos_overlap"], omin < p["neg_overlap"]
    pw = np.maximum(0.0, D - p["pos_optimal"]) * np.sqrt(omin * pos) * pos
    nw = np.maximum(0.0, p["neg_optimal"] - D) * neg
    ls = p["log_scale"]
    a, b = ls * (D - p["pos_margin"]) * pw, ls * (p["neg_margin"] - D) * nw

    def lse(x, ax):
        m = x.max(axis=ax, keepdims=True)
        return m + np.log(np.exp(x - m).sum(axis=ax, keepdims=True))

    sp = lambda x: np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20))))
    sig = lambda x: np.where(x > 20, 1.0, np.exp(np.minimum(x, 20)) / (1 + np.exp(np.minimum(x, 20))))
    gD = np.zeros((M, N))
    loss = 0.0
    for ax in (1, 0):
        la, lb = lse(a, ax), lse(b, ax)
        anchors = (pos.sum(axis=ax, keepdims=True) > 0) & (neg.sum(axis=ax, keepdims=True) > 0)
        n = anchors.sum()
        loss += (sp(la + lb)[anchors].sum() / ls / n if n else np.nan) / 2
        if n:
            gD += anchors * 0.5 / n * sig(la + lb) * (np.exp(a - la) * pw - np.exp(b - lb) * nw)
    gS = np.where(t >= 0, -gD / D, 0.0)
    return loss, gS @ pcd, gS.T @ img


def _case(M, N, C, K, seed, clamp_rows=0, ov_value=None):
    g = torch.Generator().manual_seed(seed)
    img = torch.nn.functional.normalize(torch.randn(M, C, generator=g, dtype=F64), dim=1)
    pcd = torch.nn.functional.normalize(torch.randn(N, C, generator=g, dtype=F64), dim=1)
    flat = torch.randperm(M * N, generator=g)[:K]
    ii, jj = flat // N, flat % N
    for k in range(min(K, 32)):
        pcd[jj[k]] = torch.nn.functional.normalize(img[ii[k]] + 0.3 * pcd[jj[k]], dim=0)
    for k in range(clamp_rows):
        img[ii[k]] = img[ii[k]] * 1.01
        pcd[jj[k]] = img[ii[k]]
    ov = torch.rand(K, generator=g, dtype=F64) if ov_value is None else torch.full((K,), ov_value, dtype=F64)
    return img, pcd, ii, jj, ov


def _autograd(img, pcd, ii, jj, ov):
    a, b = img.clone().requires_grad_(True), pcd.clone().requires_grad_(True)
    loss = R.CoarseMatchingLoss().circle(a, b, dict(gt_img_node_corr_indices=ii, gt_pcd_node_corr_indices=jj, gt_node_corr_min_overlaps=ov))
    loss.backward()
    return float(loss.detach()), a.grad.numpy(), b.grad.numpy()


def test_circle_closed_form_is_autograd():
    for M, N, K, clamp in ((40, 30, 60, 0), (64, 48, 200, 4), (120, 90, 500, 0)):
        img, pcd, ii, jj, ov = _case(M, N, 32, K, M, clamp)
        l_ag, gi_ag, gp_ag = _autograd(img, pcd, ii, jj, ov)
        l_cf, gi_cf, gp_cf = closed_form(img, pcd, ii, jj, ov)
        assert np.isfinite(l_ag) and abs(l_ag - l_cf) < 1e-12 * max(1.0, abs(l_ag))
        assert np.abs(gi_ag - gi_cf).max() < 1e-12 * max(1.0, np.abs(gi_ag).max())
        assert np.abs(gp_ag - gp_cf).max() < 1e-12 * max(1.0, np.abs(gp_ag).max())


def test_circle_empty_anchor_set():
    for K in (0, 5):                                 # no list / only entries between the thresholds: no positive anywhere
        img, pcd, ii, jj, ov = _case(20, 16, 16, max(K, 1), 3, ov_value=0.25)
        ii, jj, ov = ii[:K], jj[:K], ov[:K]
        l_ag, gi_ag, gp_ag = _autograd(img, pcd, ii, jj, ov)
        l_cf, gi_cf, gp_cf = closed_form(img, pcd, ii, jj, ov)
        assert np.isnan(l_ag) and np.isnan(l_cf)
        assert not gi_ag.any() and not gp_ag.any() and not gi_cf.any() and not gp_cf.any()


def test_restatement_is_the_oracle():
    """HostTrain2D3D's fusion module and matching head (float64) against oracle.fusion_module / match_head_2d3d on the same weights: values
    and float64 gradients"""
    host = R.load_synth(R.HostTrain2D3D()).double()
    b = R.batch_to(R.make_batch(24, 40, 7, nv=20, mv=33), "cpu", F64)
    W = dict(host.state_dict())
    cfg = dict(H=4, n_layers=6, skh_iters=3)
    feats = {k: b[k].clone().requires_grad_(True) for k in ("img_feats", "img_dino", "pcd_feats")}
    img_h, pcd_h = host.transformer(feats["img_feats"][None], feats["img_dino"][None], b["img_pixels"][None], feats["pcd_feats"][None],
                                    b["pcd_points"][None])
    conf_h = host.coarse_matching(pcd_h, img_h, b["src_mask"], b["tgt_mask"])[0]
    Wg = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    feats_o = {k: b[k].clone().requires_grad_(True) for k in ("img_feats", "img_dino", "pcd_feats")}
    img_o, pcd_o = orc.fusion_module(Wg, cfg, feats_o["img_feats"][None], feats_o["img_dino"][None], b["img_pixels"][None], feats_o["pcd_feats"][None],
                                     b["pcd_points"][None], prefix="transformer.")
    conf_o = orc.match_head_2d3d(Wg, cfg, pcd_o, img_o, b["src_mask"], b["tgt_mask"], prefix="coarse_matching.")
    assert (img_h - img_o).abs().max().item() < 1e-10 and (pcd_h - pcd_o).abs().max().item() < 1e-10
    assert (conf_h - conf_o).abs().max().item() < 1e-10
    g = torch.Generator().manual_seed(1)
    wts = torch.randn(conf_h.shape, generator=g, dtype=F64)
    ((conf_h * wts).sum() + img_h.square().mean()).backward()
    ((conf_o * wts).sum() + img_o.square().mean()).backward()
    for n, p in host.named_parameters():
        if n.startswith("transformer.") or n.startswith("coarse_matching."):
            ref = Wg[n].grad
            assert ref is not None and (p.grad - ref).abs().max().item() <= 1e-9 * max(1.0, ref.abs().max().item()), n
    for k in feats:
        assert (feats[k].grad - feats_o[k].grad).abs().max().item() <= 1e-9 * max(1.0, feats_o[k].grad.abs().max().item()), k


def test_restatement_reproduces_reference_fixture(golden):
    """losses, both conf matrices and every gradient of the branch step: the restatement in float64 IS the reference's float64 run (1e-9 of each
    tensor's maximum; 1e-7 absolute on the conf matrices, which the fixture stores as float32), and its float32 run is as close to the
    reference's float64 as the reference's own float32 backward (twice), or within 1e-3 of the tensor's maximum"""
    g = golden("train2d3d_branch")
    b = R.make_batch(96, 160, 31, nv=90, mv=150)
    assert np.allclose(R.input_checksum(b), g["input_checksum"], rtol=1e-6, atol=0)      # (float32 rounding of the warp differs by CPU)
    host = R.load_synth(R.HostTrain2D3D())
    g64 = {k[4:]: g[k] for k in g.files if k.startswith("g64_")}
    od, losses, grads = R.run_step(R.clone_as(host, F64, "cpu").train(), R.CoarseMatchingLoss(), R.batch_to(b, "cpu", F64))
    assert np.abs(np.array([float(l.detach()) for l in losses]) - g["losses64"]).max() <= 1e-9 * np.abs(g["losses64"]).max()
    assert np.abs(od["conf_matrix_pred"][0].detach().numpy() - g["conf_pred64"]).max() < 1e-7
    assert np.abs(od["conf_matrix_gt_hat"][0].detach().numpy() - g["conf_gt_hat64"]).max() < 1e-7
    assert sorted(grads) == sorted(g64)
    big = max(np.abs(a).max() for a in g64.values())
    for n, ref in g64.items():
        assert np.abs(R.fixture_sub(grads[n]) - ref).max() <= max(1e-9 * np.abs(ref).max(), 1e-12 * big), n
    od, losses, grads = R.run_step(R.clone_as(host, torch.float32, "cpu").train(), R.CoarseMatchingLoss(), R.batch_to(b, "cpu", torch.float32))
    assert np.abs(np.array([float(l.detach()) for l in losses]) - g["losses64"]).max() <= 1e-5 * np.abs(g["losses64"]).max()
    for n, ref in g64.items():
        e, r = np.abs(R.fixture_sub(grads[n]) - ref).max(), np.abs(g["g32_" + n].astype(np.float64) - ref).max()
        floor = 1e-6 * big if n.endswith("attention.attention.k_token_layer.bias") else 0.0
        assert e <= max(1e-3 * np.abs(ref).max(), 2 * r, floor), (n, e, r)
