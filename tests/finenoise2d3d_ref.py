"""Test-side restatement, in plain torch (float32 or float64, any device), of the three pieces of a 2D-3D training step behind the image backbone
that diffreg_hip runs with `accelerate(noising=True)` / `accelerate_loss(fine=True)`: FineMatchingLoss.forward (EXP/loss.py:157-215 with
vision3d's pairwise_distance, apply_transform and CircleLoss), SoftProcrustesLayer.forward (EXP/procrustes.py:17-93), q_sample
(EXP/model.py:109-139) and get_warped_from_noising_matching3D3D (EXP/model.py:830-846); and deterministic scenes (integer hash: the same on
every platform).  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1/.  tests/test_finenoise2d3d_oracle.py pins this file to
the fixture minted from the reference itself (tools/golden/make_golden_finenoise2d3d.py)."""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.train2d3d_ref import CircleLoss, CoarseMatchingLoss, HostTrain2D3D, circle_loss, log_optimal_transport

calls = {"procrustes": 0, "warp": 0, "fine": 0}

FINE_CFG = dict(pos_radius_3d=0.0375, neg_radius_3d=0.1, pos_radius_2d=8.0, neg_radius_2d=12.0, pos_margin=0.1, neg_margin=1.4, pos_optimal=0.1,
                neg_optimal=1.4, log_scale=24.0, max_correspondences=256)          # EXP/config.py:166-177
GRAD_COL_STRIDE = 4        # the fixture stores channels [::4] of the selected rows' gradients
MARGIN_3D, MARGIN_2D, MARGIN_F = 1e-6, 1e-4, 1e-6                                   # the fixture rules (DESIGN 5g's margins; fdist off 0)


def _hash01(idx, seed):
    x = np.asarray(idx, dtype=np.uint64) + np.uint64((int(seed) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(30); x = (x * np.uint64(0xBF58476D1CE4E5B9)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(27); x = (x * np.uint64(0x94D049BB133111EB)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def _gauss(shape, seed):
    n = int(np.prod(shape))
    u = sum(_hash01(np.arange(n) + k * n, seed) for k in range(4))
    return ((u - 2.0) * math.sqrt(3.0)).reshape(shape)


def _normalize(x):
    return x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)


def make_fine_scene(H=120, W=160, N=600, C=128, K=400, seed=3, pitch=0.004, spread=1.0, dup=0):
    """an H x W depth image (img_points, normalised img_feats), N points with their pixels and features, and K correspondences (pixel (v, u),
    point index): point j lies `pitch`-scale noise off the image point of its pixel, in a frame `transform` maps back; `dup` > 0 repeats the
    first `dup` correspondences (equal pixels AND equal points) at the end of the list; spread > 1 moves the points off the image (no positives)"""
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    z = 1.0 + 0.1 * np.sin(vv / 7.0) * np.cos(uu / 9.0)
    img_points = np.stack([uu * pitch, vv * pitch, z], -1).reshape(H * W, 3)
    img_feats = _normalize(_gauss((H * W, C), seed))
    pix_v = np.floor(_hash01(np.arange(N), seed + 1) * H).astype(np.int64)
    pix_u = np.floor(_hash01(np.arange(N), seed + 2) * W).astype(np.int64)
    at = pix_v * W + pix_u
    ang = 0.4
    R = np.array([[math.cos(ang), -math.sin(ang), 0.0], [math.sin(ang), math.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    t = np.array([0.3, -0.2, 0.1])
    world = img_points[at] * spread + 0.5 * pitch * _gauss((N, 3), seed + 3)
    pcd_points = (world - t) @ R                                               # transform: p R^T + t = world
    pcd_pixels = np.stack([pix_v, pix_u], -1) + 0.4 * (_hash01(np.arange(2 * N), seed + 4).reshape(N, 2) - 0.5)
    pcd_feats = _normalize(img_feats[at] + 0.08 * _gauss((N, C), seed + 5))
    transform = np.eye(4); transform[:3, :3] = R; transform[:3, 3] = t
    order = np.argsort(_hash01(np.arange(N), seed + 6), kind="stable")[:K]
    if dup:
        order = np.concatenate([order, order[:dup]])
    T = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    return dict(img_points=T(img_points), img_feats=T(img_feats), pcd_points=T(pcd_points), pcd_pixels=T(pcd_pixels), pcd_feats=T(pcd_feats),
                transform=T(transform), img_corr_pixels=T(np.stack([pix_v[order], pix_u[order]], -1), torch.int64),
                pcd_corr_indices=T(order, torch.int64), image_w=W, image_h=H)


FINE_CASES = {            # name -> make_fine_scene arguments; "sub" holds more correspondences than max_correspondences (sub-sampled, seeded numpy RNG)
    "sub": dict(K=400, seed=3),
    "dup": dict(K=150, seed=3, dup=30),
    "empty": dict(K=90, seed=3, spread=3.0),
}


def select(sc, cfg=FINE_CFG, rng_seed=0):
    """FineMatchingLoss.forward's sub-sampling (EXP/loss.py:177-183) with numpy's global RNG seeded"""
    px, idx = sc["img_corr_pixels"], sc["pcd_corr_indices"]
    if idx.shape[0] > cfg["max_correspondences"]:
        np.random.seed(rng_seed)
        sel = torch.from_numpy(np.random.choice(idx.shape[0], size=cfg["max_correspondences"], replace=False))
        px, idx = px[sel], idx[sel]
    return px, idx


def strict_distance(x, y):
    return torch.linalg.norm(x.unsqueeze(-2) - y.unsqueeze(-3), dim=-1)


def fine_terms(sc, sel_pixels, sel_indices, dtype, img_feats=None, pcd_feats=None):
    """EXP/loss.py:174-206 -> (dist3d, dist2d, fdist) of the selected correspondences, in `dtype`"""
    f = lambda k: sc[k].to(dtype)
    img_feats = f("img_feats") if img_feats is None else img_feats
    pcd_feats = f("pcd_feats") if pcd_feats is None else pcd_feats
    T = f("transform")
    pcd_points = torch.matmul(f("pcd_points"), T[:3, :3].transpose(-1, -2)) + T[None, :3, 3]
    ii = sel_pixels[:, 0] * sc["image_w"] + sel_pixels[:, 1]
    d3 = strict_distance(f("img_points")[ii], pcd_points[sel_indices])
    d2 = strict_distance(sel_pixels.to(dtype), f("pcd_pixels")[sel_indices])
    x, y = img_feats[ii], pcd_feats[sel_indices]
    fd = ((x ** 2).sum(-1)[:, None] - 2 * torch.matmul(x, y.transpose(-1, -2)) + (y ** 2).sum(-1)[None, :]).clamp(min=0.0)
    return d3, d2, fd


def fine_loss(sc, sel_pixels, sel_indices, dtype, cfg=FINE_CFG, img_feats=None, pcd_feats=None, mutant=None):
    """EXP/loss.py:186-213 -> (loss, recall); `mutant` (a test's own wrong variants): 'sqrt' takes the root of fdist"""
    d3, d2, fd = fine_terms(sc, sel_pixels, sel_indices, dtype, img_feats, pcd_feats)
    if mutant == "sqrt":
        fd = torch.sqrt(fd + 1e-8)
    pos = (d3 < cfg["pos_radius_3d"]) & (d2 < cfg["pos_radius_2d"])
    neg = (d3 > cfg["neg_radius_3d"]) | (d2 > cfg["neg_radius_2d"])
    loss = circle_loss(fd, pos, neg, cfg["pos_margin"], cfg["neg_margin"], cfg["pos_optimal"], cfg["neg_optimal"], cfg["log_scale"])
    with torch.no_grad():
        gt = pos.to(fd.dtype)
        pred = torch.zeros_like(fd)
        pred[torch.arange(fd.shape[0], device=fd.device), fd.min(-1)[1]] = 1.0
        recall = (pred * gt).sum() / (torch.gt(gt.sum(-1), 0).to(fd.dtype).sum() + 1e-12)
    return loss, recall


def fine_loss_and_grads(sc, sel_pixels, sel_indices, dtype, device="cpu", cfg=FINE_CFG, mutant=None):
    sc = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in sc.items()}
    fi = sc["img_feats"].to(dtype).clone().requires_grad_(True)
    fp = sc["pcd_feats"].to(dtype).clone().requires_grad_(True)
    loss, recall = fine_loss(sc, sel_pixels.to(device), sel_indices.to(device), dtype, cfg, fi, fp, mutant)
    if torch.isfinite(loss):
        loss.backward()
    gi = fi.grad if fi.grad is not None else torch.zeros_like(fi)
    gp = fp.grad if fp.grad is not None else torch.zeros_like(fp)
    return loss.detach(), recall, gi.detach(), gp.detach()


def fixture_rules(sc, sel_pixels, sel_indices, cfg=FINE_CFG):
    """the rules a fine-loss fixture scene must obey (cap on undecided cases: 0); returns a list of violations"""
    bad = []
    d3, d2, fd = fine_terms(sc, sel_pixels, sel_indices, torch.float64)
    _, _, fd32 = fine_terms(sc, sel_pixels, sel_indices, torch.float32)
    for r in (cfg["pos_radius_3d"], cfg["neg_radius_3d"]):
        if bool(((d3 - r).abs() <= MARGIN_3D).any()):
            bad.append("a 3-D distance within %g of the radius %g" % (MARGIN_3D, r))
    for r in (cfg["pos_radius_2d"], cfg["neg_radius_2d"]):
        if bool(((d2 - r).abs() <= MARGIN_2D).any()):
            bad.append("a 2-D distance within %g of the radius %g" % (MARGIN_2D, r))
    if bool((fd <= MARGIN_F).any()):
        bad.append("an fdist within %g of 0" % MARGIN_F)
    if not torch.equal(fd.min(-1)[1], fd32.min(-1)[1]):
        bad.append("float32 and float64 row arg-mins of fdist differ")
    return bad


# ---- the noising front end ----------------------------------------------------------------------------------------------------------------------
def soft_procrustes(conf, src_pcd, tgt_pcd, src_mask, tgt_mask, sample_rate, max_cond, want_sel=False, k_padded=False):
    """SoftProcrustesLayer.forward in conf's dtype and on its device (the reference's `.cpu().double()` SVD: double, where the tensors are) ->
    (R, t, R_forwd, t_forwd, condition, solution_mask[, the K selected flat indices, the sorted confidences]).  k_padded: the test's own wrong
    variant that takes K from the padded sizes"""
    B, N, M = conf.shape
    entry_max = (torch.stack([src_mask.sum(1), tgt_mask.sum(1)], 0).max(0)[0] * sample_rate).int()
    if k_padded:
        entry_max = torch.full_like(entry_max, int(max(N, M) * sample_rate))
    K = int(entry_max.float().mean().int())
    srt, idx = conf.view(B, -1).sort(descending=True, dim=1)
    w, idx = srt[:, :K].clone(), idx[:, :K]
    b = torch.arange(B, device=conf.device).view(-1, 1).repeat(1, K).view(-1)
    X = src_pcd[b, (idx // M).view(-1)].view(B, K, -1)
    Y = tgt_pcd[b, (idx % M).view(-1)].view(B, K, -1)
    w = (w * (torch.arange(K, device=conf.device).view(1, -1) < entry_max[:, None]).to(w.dtype))[..., None]
    wn = w / (w.abs().sum(1, keepdim=True) + 0.0001)
    mx, my = (wn * X).sum(1, keepdim=True), (wn * Y).sum(1, keepdim=True)
    Sxy = torch.matmul((Y - my).transpose(1, 2), wn * (X - mx)).double()
    U, D, V = Sxy.svd()
    cond = D.max(1)[0] / D.min(1)[0]
    S = torch.eye(3, dtype=torch.float64, device=conf.device)[None].repeat(B, 1, 1)
    S[:, 2:3, 2:3] = (U.det() * V.det()).view(-1, 1, 1)
    R = torch.matmul(U, torch.matmul(S, V.transpose(1, 2))).to(conf.dtype)
    t = my.transpose(1, 2) - torch.matmul(R, mx.transpose(1, 2))
    ok = cond < max_cond
    Rf, tf = R.clone(), t.clone()
    Rf[~ok] = torch.eye(3, dtype=R.dtype, device=R.device)
    tf[~ok] = torch.zeros(3, 1, dtype=R.dtype, device=R.device)
    out = (R, t, Rf, tf, cond, ok)
    return out + (idx, srt) if want_sel else out


def warp(s_pcd, t_pcd, src_mask, tgt_mask, matrix, bin_score, iters, sample_rate, max_cond, k_padded=False):
    """get_warped_from_noising_matching3D3D (EXP/model.py:830-846; the fill is out of place here) -> (warped, R, t, R_forwd, t_forwd, condition,
    solution_mask, conf); float64 inputs give the float64 run with the reference's own cast of conf to float32 REMOVED (its only effect there)"""
    x = matrix.masked_fill(~(src_mask[..., None] * tgt_mask[:, None]).bool(), float("-inf"))
    conf = log_optimal_transport(x, bin_score, iters, src_mask, tgt_mask).exp()[:, :-1, :-1].contiguous()
    if s_pcd.dtype == torch.float32:
        conf = conf.type(torch.float32)
    R, t, Rf, tf, cond, ok = soft_procrustes(conf, s_pcd, t_pcd, src_mask, tgt_mask, sample_rate, max_cond, k_padded=k_padded)
    warped = (torch.matmul(Rf, s_pcd.transpose(1, 2)) + tf).transpose(1, 2)
    return warped, R, t, Rf, tf, cond, ok, conf


def q_sample(x_start, t, noise, timesteps=1000):
    """EXP/model.py:109-139, verbatim arithmetic (the schedule rebuilt on every call)"""
    x = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64)
    ac = torch.cos(((x / timesteps) + 0.008) / (1 + 0.008) * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    betas = torch.clip(1 - (ac[1:] / ac[:-1]), 0, 0.999).to(x_start.device)
    alphas_cumprod = torch.cumprod(1. - betas, dim=0)
    shape = (t.shape[0],) + (1,) * (len(x_start.shape) - 1)
    a = torch.sqrt(alphas_cumprod).gather(-1, t).reshape(shape)
    b = torch.sqrt(1. - alphas_cumprod).gather(-1, t).reshape(shape)
    return a * x_start + b * noise


def make_warp_case(N=96, M=160, nv=90, mv=150, seed=7, noise=0.6, degenerate=False):
    """source points, target points = a rigid motion of matched sources + noise, masks with padding, a GT matrix and its noised scores (float32;
    the reference's q_sample makes them float64 -- the tests cast); degenerate: the sources lie within centimetres of a line, so the fit's condition number is
    above max_condition_num and the warp is the identity"""
    s = _gauss((N, 3), seed) * 0.5
    if degenerate:
        s = np.outer(_gauss((N,), seed), np.array([1.0, 0.5, -0.25])) + 0.03 * _gauss((N, 3), seed + 9)
    ang = 0.5
    R = np.array([[math.cos(ang), 0.0, math.sin(ang)], [0.0, 1.0, 0.0], [-math.sin(ang), 0.0, math.cos(ang)]])
    match = np.floor(_hash01(np.arange(M), seed + 1) * nv).astype(np.int64)
    t = s[match] @ R.T + np.array([0.2, -0.1, 0.3]) + 0.01 * _gauss((M, 3), seed + 2)
    gt = np.zeros((1, N, M))
    cols = np.arange(0, mv, 3)
    gt[0, match[cols], cols] = 1.0
    x = gt * 0.8 + noise * _gauss((1, N, M), seed + 3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    return dict(s_pcd=T(s)[None], t_pcd=T(t)[None], src_mask=torch.arange(N)[None] < nv, tgt_mask=torch.arange(M)[None] < mv, matrix_gt=T(gt),
                scores=T(x), w=T(_gauss((1, N, 3), seed + 4)))


WARP_CASES = {"fit": dict(seed=7), "gated": dict(seed=8, degenerate=True)}
WARP_HP = dict(iters=3, sample_rate=1.0, max_cond=200.0, bin_score=1.0)


def warp_and_grads(c, dtype, device="cpu", k_padded=False):
    """the warp of case `c` in `dtype` -> dict(warped, R, t, R_forwd, t_forwd, condition, mask, conf, g_bin = d(sum <warped, w>) / d bin_score,
    g_scores = d / d scores)"""
    f = lambda k: c[k].to(device=device, dtype=dtype)
    sm, tm = c["src_mask"].to(device), c["tgt_mask"].to(device)
    x = f("scores").clone().requires_grad_(True)
    bs = torch.tensor(WARP_HP["bin_score"], dtype=dtype, device=device, requires_grad=True)
    out = warp(f("s_pcd"), f("t_pcd"), sm, tm, x, bs, WARP_HP["iters"], WARP_HP["sample_rate"], WARP_HP["max_cond"], k_padded=k_padded)
    (out[0] * f("w")).sum().backward()
    z = lambda g, like: torch.zeros_like(like) if g is None else g
    names = ("warped", "R", "t", "R_forwd", "t_forwd", "condition", "mask", "conf")
    res = {k: v.detach() for k, v in zip(names, out)}
    res["g_bin"], res["g_scores"] = z(bs.grad, bs).detach(), z(x.grad, x).detach()
    return res


def topk_rule(conf, src_mask, tgt_mask, sample_rate):
    """the warp fixture's rule: the K-th and (K+1)-th sorted entries of conf differ by more than 1e-6 of the K-th -> (ok, the selected set)"""
    K = int(max(int(src_mask.sum()), int(tgt_mask.sum())) * sample_rate)
    srt, idx = conf.reshape(-1).sort(descending=True)
    return bool((srt[K - 1] - srt[K]) > 1e-6 * srt[K - 1]), set(idx[:K].tolist())


# ---- a MATR2D3D-shaped stand-in with the noising front end, and an OverallLoss ---------------------------------------------------------------
def random_choice(a, size=None, replace=True):
    """vision3d.ops.random_choice for an int `a` (numpy's global RNG), minus its .cuda()"""
    return torch.from_numpy(np.random.choice(a, size=size, replace=replace))


class SoftProcrustesLayer(nn.Module):
    def __init__(self, sample_rate=1.0, max_condition_num=200.0):
        super().__init__()
        self.sample_rate, self.max_condition_num = sample_rate, max_condition_num

    def forward(self, conf_matrix, src_pcd, tgt_pcd, src_mask, tgt_mask):
        calls["procrustes"] += 1
        return soft_procrustes(conf_matrix, src_pcd, tgt_pcd, src_mask, tgt_mask, self.sample_rate, self.max_condition_num)


class FineMatchingLoss(nn.Module):
    def __init__(self, cfg=FINE_CFG):
        super().__init__()
        self.max_correspondences = cfg["max_correspondences"]
        self.pos_radius_3d, self.neg_radius_3d = cfg["pos_radius_3d"], cfg["neg_radius_3d"]
        self.pos_radius_2d, self.neg_radius_2d = cfg["pos_radius_2d"], cfg["neg_radius_2d"]
        self.circle_loss = CircleLoss(cfg["pos_margin"], cfg["neg_margin"], cfg["pos_optimal"], cfg["neg_optimal"], cfg["log_scale"])

    def forward(self, data_dict, output_dict):
        calls["fine"] += 1
        px, idx = data_dict["img_corr_pixels"], data_dict["pcd_corr_indices"]
        if idx.shape[0] > self.max_correspondences:
            sel = random_choice(idx.shape[0], size=self.max_correspondences, replace=False).to(idx.device)
            px, idx = px[sel], idx[sel]
        sc = dict(img_points=output_dict["img_points_f"], pcd_points=output_dict["pcd_points_f"], pcd_pixels=output_dict["pcd_pixels_f"],
                  transform=data_dict["transform"], image_w=data_dict["image_w"])
        fi, fp = output_dict["img_feats_f"], output_dict["pcd_feats_f"]
        return fine_loss(sc, px, idx, fi.dtype, FINE_CFG, fi, fp)


class OverallLoss(nn.Module):
    def __init__(self):
        super().__init__()
        self.c_loss, self.f_loss = CoarseMatchingLoss(), FineMatchingLoss()


class HostNoising2D3D(HostTrain2D3D):
    """HostTrain2D3D plus the noising front end of MATR2D3D.forward's training branch (EXP/model.py:583, 600-611): one ladder rung's fit on the GT
    matrix, q_sample (this module's global, as the reference's), the warp, and the fine features handed through to the fine loss"""
    def __init__(self, **kw):
        super().__init__(**kw)
        self.denoising_soft_procrustes = SoftProcrustesLayer()
        self.pcd_backbone = nn.Identity()
        self.num_timesteps = 1000

    def get_warped_from_noising_matching3D3D(self, s_pcd, t_pcd, src_mask, tgt_mask, matrix_gt_disturbed):
        calls["warp"] += 1
        head = self.denoising_coarse_matching
        matrix_gt_disturbed.masked_fill_(~(src_mask[..., None] * tgt_mask[:, None]).bool(), float("-inf"))
        conf = log_optimal_transport(matrix_gt_disturbed, head.bin_score, head.skh_iters, src_mask, tgt_mask).exp()[:, :-1, :-1].contiguous()
        if s_pcd.dtype == torch.float32:
            conf = conf.type(torch.float32)
        R, t, Rf, tf, cond, ok = self.denoising_soft_procrustes(conf, s_pcd, t_pcd, src_mask, tgt_mask)
        return (torch.matmul(Rf, s_pcd.transpose(1, 2)) + tf).transpose(1, 2), t_pcd, Rf, tf

    def forward(self, b):
        img_c, pcd_c = self.transformer(b["img_feats"][None], b["img_dino"][None], b["img_pixels"][None], b["pcd_feats"][None], b["pcd_points"][None])
        img_c, pcd_c = img_c[0], pcd_c[0]
        sm, tm = b["src_mask"], b["tgt_mask"]
        conf_pred, _, _, _ = self.coarse_matching(pcd_c[None], img_c[None], sm, tm, True)
        od = dict(conf_matrix_pred=conf_pred, img_feats_c=F.normalize(img_c, p=2, dim=1), pcd_feats_c=F.normalize(pcd_c, p=2, dim=1))
        ladder = self.denoising_soft_procrustes(b["matrix_gt"], b["pcd_points"][None], b["t_pcd"][None], sm, tm)
        x = q_sample(x_start=b["matrix_gt"], t=b["ts"], noise=b["noise"], timesteps=self.num_timesteps)
        warped, _, Rf, tf = self.get_warped_from_noising_matching3D3D(b["pcd_points"][None], b["t_pcd"][None], sm, tm, x)
        img_d, pcd_d = self.denoising_transformer(b["img_feats"][None], b["img_dino"][None], b["img_pixels"][None], b["pcd_feats"][None], warped)
        conf_hat, _, _, _ = self.denoising_coarse_matching(pcd_d, img_d, sm, tm, True)
        od.update(conf_matrix_gt_hat=conf_hat, matrix_gt=b["matrix_gt"], src_mask=sm, tgt_mask=tm, ladder=ladder, R_forwd=Rf, t_forwd=tf,
                  img_feats_c_denoising=F.normalize(img_d[0], p=2, dim=1), pcd_feats_c_denoising=F.normalize(pcd_d[0], p=2, dim=1),
                  gt_img_node_corr_indices=b["gt_img"], gt_pcd_node_corr_indices=b["gt_pcd"], gt_node_corr_min_overlaps=b["gt_ov"])
        return od
