"""Test-side restatement of the 2D-3D training branch in plain torch (float32 or float64, any device), with the reference's module and attribute
names so that diffreg_hip.autograd2d3d / overlay2d3d can be installed on it: vision3d TransformerLayer (vision3d/layers/transformer.py:58-301),
CrossModalFusionModule (EXP/fusion_module.py:61-107), Matching, sinkhorn branch (EXP/matching.py:91-147), CoarseMatchingLoss (EXP/loss.py:30-75,
vision3d/loss/circle_loss.py:11-52), and a host with the training branch of MATR2D3D.forward (EXP/model.py:386-392, 548-553, 615-631) minus the
GT search and the noising.  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1/.  `calls` counts entries into the original
forwards (the overlay tests assert that the device path never enters them)."""
import copy

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from diffreg_hip import synth

calls = {"fusion": 0, "matching": 0, "loss": 0}


class _MHA(nn.Module):
    def __init__(self, C, H):
        super().__init__()
        self.num_heads = H
        self.q_token_layer, self.k_token_layer, self.v_token_layer = nn.Linear(C, C), nn.Linear(C, C), nn.Linear(C, C)


class _AttentionLayer(nn.Module):
    def __init__(self, C, H):
        super().__init__()
        self.attention = _MHA(C, H)
        self.linear = nn.Linear(C, C)
        self.norm = nn.LayerNorm(C)


class _Output(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.expand, self.squeeze, self.norm = nn.Linear(C, 2 * C), nn.Linear(2 * C, C), nn.LayerNorm(C)


class TransformerLayer(nn.Module):
    def __init__(self, C, H):
        super().__init__()
        self.attention = _AttentionLayer(C, H)
        self.output = _Output(C)

    def forward(self, x, y, v=None, k_masks=None):
        """k_masks: True = the key is ignored (the reference's convention)"""
        mha = self.attention.attention
        B, L, C = x.shape
        S, H = y.shape[1], mha.num_heads
        d = C // H
        q = mha.q_token_layer(x).view(B, L, H, d).transpose(1, 2)
        k = mha.k_token_layer(y).view(B, S, H, d).transpose(1, 2)
        vv = mha.v_token_layer(y).view(B, S, H, d).transpose(1, 2)
        a = torch.einsum("bhnc,bhmc->bhnm", q, k) / d ** 0.5
        if k_masks is not None:
            a = a.masked_fill(k_masks[:, None, None, :], float("-inf"))
        h = torch.matmul(torch.softmax(a, dim=-1), vv).transpose(1, 2).reshape(B, L, C)
        z = self.attention.norm(self.attention.linear(h) + x)
        o = self.output
        return o.norm(z + o.squeeze(torch.relu(o.expand(z))))


class FourierEmbedding(nn.Module):
    """vision3d/layers/embedding.py:75-100 with use_pi=False, use_input=True"""
    def __init__(self, L=10):
        super().__init__()
        self.L = L

    def forward(self, p):
        shape, D = p.shape[:-1], p.shape[-1]
        x = p.reshape(-1, 1, D)
        fac = (2.0 ** torch.arange(0, self.L, device=p.device).to(p.dtype)).view(1, -1, 1)
        emb = torch.cat([torch.sin(fac * x), torch.cos(fac * x)], dim=-1).reshape(*shape, 2 * self.L * D)
        return torch.cat([p, emb], dim=-1)


class CrossModalFusionModule(nn.Module):
    def __init__(self, img_dim, dino_dim, pcd_dim, C, H, blocks):
        super().__init__()
        self.use_embedding = True
        self.embedding = FourierEmbedding(10)
        self.img_emb_proj, self.pcd_emb_proj = nn.Linear(42, C), nn.Linear(63, C)
        self.img_in_proj, self.img_in_proj_dino, self.img_in_proj_all = nn.Linear(img_dim, C), nn.Linear(dino_dim, C), nn.Linear(2 * C, C)
        self.pcd_in_proj, self.out_proj = nn.Linear(pcd_dim, C), nn.Linear(C, C)
        self.blocks = blocks
        self.transformer = nn.ModuleList([TransformerLayer(C, H) for _ in blocks])

    def forward(self, img_feats, img_feats_dino, img_pixels, pcd_feats, pcd_points):
        calls["fusion"] += 1
        img = self.img_in_proj_all(torch.relu(torch.cat([self.img_in_proj(img_feats), self.img_in_proj_dino(img_feats_dino)], dim=-1)))
        pcd = self.pcd_in_proj(pcd_feats)
        img = img + self.img_emb_proj(self.embedding(img_pixels))
        pcd = pcd + self.pcd_emb_proj(self.embedding(pcd_points - pcd_points.mean(dim=1)))
        for i, block in enumerate(self.blocks):
            if block == "self":
                img = self.transformer[i](img, img, img)
                pcd = self.transformer[i](pcd, pcd, pcd)
            else:
                img = self.transformer[i](img, pcd, pcd)
                pcd = self.transformer[i](pcd, img, img)
        return self.out_proj(img), self.out_proj(pcd)


def log_optimal_transport(scores, alpha, iters, src_mask, tgt_mask):
    """EXP/matching.py (SuperGlue form) with the reference's dtype quirks, any device (oracle.sinkhorn_log, device-aware)"""
    B, N, M = scores.shape
    rows = src_mask.sum(1, keepdim=True)
    cols = tgt_mask.sum(1, keepdim=True)
    a = alpha.to(scores.dtype)
    Z = torch.cat([torch.cat([scores, a.expand(B, N, 1)], 2), a.expand(B, 1, M + 1)], 1)
    nu0 = -(rows + cols).log()
    log_mu = torch.cat([nu0.expand(B, N), cols.log() + nu0], 1)
    log_nu = torch.cat([nu0.expand(B, M), rows.log() + nu0], 1)
    u, v = torch.zeros_like(log_mu).to(scores.dtype), torch.zeros_like(log_nu).to(scores.dtype)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v[:, None, :], dim=2)
        v = log_nu - torch.logsumexp(Z + u[:, :, None], dim=1)
    return Z + u[:, :, None] + v[:, None, :] - nu0[:, :, None]


class Matching(nn.Module):
    def __init__(self, C, iters=3):
        super().__init__()
        self.src_proj = nn.Linear(C, C, bias=False)
        self.bin_score = nn.Parameter(torch.tensor(1.0))
        self.skh_iters = iters
        self.match_type = "sinkhorn"

    def forward(self, src_feats, tgt_feats, src_mask, tgt_mask, mutual=True):
        calls["matching"] += 1
        s, t = self.src_proj(src_feats), self.src_proj(tgt_feats)
        s, t = s / s.shape[-1] ** 0.5, t / t.shape[-1] ** 0.5
        sim = torch.einsum("bsc,btc->bst", s, t).masked_fill(~(src_mask[..., None] * tgt_mask[:, None]).bool(), float("-inf"))
        conf = log_optimal_transport(sim, self.bin_score, self.skh_iters, src_mask, tgt_mask).exp()[:, :-1, :-1].contiguous()
        with torch.no_grad():                # the mutual top-1 read-out (a value): row arg-maxima whose column arg-maximum is the same row
            c = conf[0]
            ri, ci = c.argmax(1), c.argmax(0)
            rows = torch.arange(c.shape[0], device=c.device)
            keep = ci[ri] == rows if mutual else torch.ones_like(rows, dtype=torch.bool)
            si, ti = rows[keep], ri[keep]
        return conf, si, ti, c[si, ti]


def circle_loss(dist, pos, neg, pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale, pos_scales=None):
    """the weighted circle loss: detached weights (positives: relu(dist - pos_optimal) x scale; negatives: relu(neg_optimal - dist)), positive and
    negative log-sum-exps along rows and along columns over ALL entries, softplus / log_scale, mean over the anchors that hold both a positive and a
    negative (an empty anchor set: NaN), the row and column means averaged"""
    zero = torch.zeros_like(dist)
    big = 1e5 * (~pos).to(dist.dtype), 1e5 * (~neg).to(dist.dtype)
    wp = torch.maximum(zero, dist - big[0] - pos_optimal)
    wp = (wp * pos_scales if pos_scales is not None else wp).detach()
    wn = torch.maximum(zero, neg_optimal - (dist + big[1])).detach()
    lp, ln = log_scale * (dist - pos_margin) * wp, log_scale * (neg_margin - dist) * wn
    terms = []
    for dim in (-1, -2):
        anchors = (pos.sum(dim) > 0) & (neg.sum(dim) > 0)
        per = F.softplus(torch.logsumexp(lp, dim=dim) + torch.logsumexp(ln, dim=dim)) / log_scale
        terms.append(per[anchors].mean())
    return (terms[0] + terms[1]) / 2


class CircleLoss(nn.Module):
    def __init__(self, pos_margin=0.1, neg_margin=1.4, pos_optimal=0.1, neg_optimal=1.4, log_scale=40.0):
        super().__init__()
        self.pos_margin, self.neg_margin, self.pos_optimal, self.neg_optimal, self.log_scale = pos_margin, neg_margin, pos_optimal, neg_optimal, log_scale

    def forward(self, pos_masks, neg_masks, feat_dists, pos_scales=None):
        return circle_loss(feat_dists, pos_masks, neg_masks, self.pos_margin, self.neg_margin, self.pos_optimal, self.neg_optimal, self.log_scale,
                           pos_scales)


def feat_dists(x, y):
    return torch.sqrt((2.0 - 2.0 * (x @ y.T)).clamp(min=0.0) + 1e-8)


class CoarseMatchingLoss(nn.Module):
    """EXP/config.py:155-163 values"""
    def __init__(self):
        super().__init__()
        self.weighted_circle_loss = CircleLoss(0.1, 1.4, 0.1, 1.4, 40.0)
        self.positive_overlap, self.negative_overlap = 0.3, 0.2
        self.pos_w, self.neg_w, self.focal_alpha, self.focal_gamma = 1.0, 1.0, 0.25, 2.0

    def circle(self, img, pcd, od):
        ii, jj = od["gt_img_node_corr_indices"], od["gt_pcd_node_corr_indices"]
        d = feat_dists(img, pcd)
        mn = torch.zeros_like(d)
        mn[ii, jj] = od["gt_node_corr_min_overlaps"].to(d.dtype)
        pos = torch.gt(mn, self.positive_overlap)
        mx = torch.zeros_like(d)
        mx[ii, jj] = od["gt_node_corr_min_overlaps"].to(d.dtype)        # EXP/loss.py:36 (the max overlaps are read from the MIN list)
        neg = torch.lt(mx, self.negative_overlap)
        return self.weighted_circle_loss(pos, neg, d, torch.sqrt(mn * pos.to(d.dtype)))

    def focal(self, conf, conf_gt):
        pos, neg = conf_gt == 1, conf_gt == 0
        pos_w, neg_w = self.pos_w, self.neg_w
        if not pos.any():
            pos = pos.clone(); pos[0, 0, 0] = True; pos_w = 0.0
        if not neg.any():
            neg = neg.clone(); neg[0, 0, 0] = True; neg_w = 0.0
        conf = torch.clamp(conf, 1e-6, 1 - 1e-6)
        a, g = self.focal_alpha, self.focal_gamma
        lp = -a * torch.pow(1 - conf[pos], g) * conf[pos].log()
        ln = -a * torch.pow(conf[neg], g) * (1 - conf[neg]).log()
        return pos_w * lp.mean() + neg_w * ln.mean()

    def forward(self, od):
        calls["loss"] += 1
        return (self.circle(od["img_feats_c"], od["pcd_feats_c"], od), self.circle(od["img_feats_c_denoising"], od["pcd_feats_c_denoising"], od),
                self.focal(od["conf_matrix_pred"], od["matrix_gt"]), self.focal(od["conf_matrix_gt_hat"], od["matrix_gt"]))


class _Bag(nn.Module):
    def __init__(self, **kw):
        super().__init__()
        for k, v in kw.items():
            setattr(self, k, v)


class HostTrain2D3D(nn.Module):
    """the differentiable part of MATR2D3D.forward's training branch on given backbone features, GT lists and warped points"""
    def __init__(self, C=256, H=4, img_dim=512, dino_dim=1024, pcd_dim=512, blocks=("self", "cross", "self", "cross", "self", "cross")):
        super().__init__()
        self.transformer = CrossModalFusionModule(img_dim, dino_dim, pcd_dim, C, H, list(blocks))
        self.denoising_transformer = CrossModalFusionModule(img_dim, dino_dim, pcd_dim, C, H, list(blocks))
        self.coarse_matching = Matching(C)
        self.denoising_coarse_matching = Matching(C)
        self.denoising_soft_procrustes = _Bag(sample_rate=1.0, max_condition_num=200.0)
        self.sampling_timesteps = 2

    def get_warped_from_noising_matching3D3D(self, *a):
        raise AssertionError("the eval loop is not part of these tests")

    def forward(self, b):
        img_c, pcd_c = self.transformer(b["img_feats"][None], b["img_dino"][None], b["img_pixels"][None], b["pcd_feats"][None], b["pcd_points"][None])
        img_c, pcd_c = img_c[0], pcd_c[0]
        sm, tm = b["src_mask"], b["tgt_mask"]
        conf_pred, _, _, _ = self.coarse_matching(pcd_c[None], img_c[None], sm, tm, True)
        od = dict(conf_matrix_pred=conf_pred, img_feats_c=F.normalize(img_c, p=2, dim=1), pcd_feats_c=F.normalize(pcd_c, p=2, dim=1))
        img_d, pcd_d = self.denoising_transformer(b["img_feats"][None], b["img_dino"][None], b["img_pixels"][None], b["pcd_feats"][None],
                                                  b["warped"][None])
        conf_hat, _, _, _ = self.denoising_coarse_matching(pcd_d, img_d, sm, tm, True)
        od.update(conf_matrix_gt_hat=conf_hat, matrix_gt=b["matrix_gt"], src_mask=sm, tgt_mask=tm,
                  img_feats_c_denoising=F.normalize(img_d[0], p=2, dim=1), pcd_feats_c_denoising=F.normalize(pcd_d[0], p=2, dim=1),
                  gt_img_node_corr_indices=b["gt_img"], gt_pcd_node_corr_indices=b["gt_pcd"], gt_node_corr_min_overlaps=b["gt_ov"])
        return od


def load_synth(host, seeds=(9, 10), head_gain=4.0):
    """synthetic weights (synth.make_weights_2d3d, one seed per module pair, prefixes renamed) into a HostTrain2D3D"""
    sd = {}
    for seed, (tp, mp) in zip(seeds, (("transformer.", "coarse_matching."), ("denoising_transformer.", "denoising_coarse_matching."))):
        for k, a in synth.make_weights_2d3d(seed=seed, head_gain=head_gain).items():
            if k.startswith("denoising_transformer."):
                sd[tp + k[len("denoising_transformer."):]] = torch.from_numpy(np.ascontiguousarray(a))
            elif k.startswith("denoising_coarse_matching.") and "tgt_proj" not in k:
                sd[mp + k[len("denoising_coarse_matching."):]] = torch.from_numpy(np.ascontiguousarray(a))
    host.load_state_dict(sd)
    return host


def make_batch(N, M, seed, K=None, nv=None, mv=None):
    """backbone features, positions, masks, GT matrix and a duplicate-free GT node-correspondence list with overlaps (float32, CPU)"""
    Wn = synth.make_weights_2d3d(seed=9)
    p = synth.make_pair_2d3d(N, M, seed, weights=Wn)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    g = torch.Generator().manual_seed(seed)
    K = K if K is not None else max(8, (N * M) // 200)
    flat = torch.randperm(N * M, generator=g)[:K]
    ov = torch.rand(K, generator=g)
    ang = 0.3
    Rz = torch.tensor([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    s_pcd = T(p["s_pcd"])
    matrix_gt = torch.zeros(1, N, M)
    matrix_gt.view(-1)[torch.randperm(N * M, generator=g)[: max(6, N // 4)]] = 1.0
    nv = N if nv is None else nv
    mv = M if mv is None else mv
    return dict(img_feats=T(p["img_feats"]), img_dino=T(p["img_dino"]), img_pixels=T(p["img_pixels"]), pcd_feats=T(p["pcd_feats"]), pcd_points=s_pcd,
                warped=s_pcd @ Rz.T + torch.tensor([0.05, -0.02, 0.01]), src_mask=torch.arange(N)[None] < nv, tgt_mask=torch.arange(M)[None] < mv,
                matrix_gt=matrix_gt, gt_img=(flat % M).long(), gt_pcd=(flat // M).long(), gt_ov=ov)


def batch_to(b, device, dtype):
    return {k: (v.to(device=device, dtype=dtype) if v.is_floating_point() else v.to(device)) for k, v in b.items()}


def run_step(host, loss_module, b, want_feat_grads=True):
    """forward + (loss_circle + loss_matrix_gt_hat).backward() (OverallLoss, EXP/loss.py:226-238) -> (output dict, the four losses, gradients by
    name: every parameter and the three backbone-feature inputs)"""
    host.zero_grad(set_to_none=True)
    b = dict(b)
    if want_feat_grads:
        for k in ("img_feats", "img_dino", "pcd_feats"):
            b[k] = b[k].clone().requires_grad_(True)
    od = host(b)
    losses = loss_module(od)
    (losses[0] + losses[3]).backward()
    grads = {n: p.grad.detach().clone() for n, p in host.named_parameters() if p.grad is not None}
    if want_feat_grads:
        grads.update({"input." + k: b[k].grad.detach().clone() for k in ("img_feats", "img_dino", "pcd_feats")})
    return od, losses, grads


FIXTURE_STRIDE = 16      # tools/golden/make_golden_train2d3d.py: entries [::16, ::16] of a matrix gradient


def fixture_sub(g):
    g = g.detach().double().cpu()
    return (g[::FIXTURE_STRIDE, ::FIXTURE_STRIDE] if g.dim() == 2 else g).numpy()


def input_checksum(b):
    """the fixture's check that make_batch still yields the inputs it was minted from"""
    return np.array([float(b[k].double().sum()) for k in sorted(b) if b[k].is_floating_point()])


def clone_as(host, dtype, device):
    return copy.deepcopy(host).to(device=device, dtype=dtype)
