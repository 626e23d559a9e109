"""torch.autograd wrappers of the 2D-3D training branch (Diff-Reg-2d3d, EXP = experiments/2d3dmatr.rgbdv2.stage4.level3.stage1/): the
CrossModalFusionModule with its vision3d TransformerLayers (forward and backward one library call each: dr_fusion_layer_train_forward_f32 /
dr_fusion_layer_backward_f32), the position-free Sinkhorn matching head, and the circle + focal terms of CoarseMatchingLoss (dr_circle_loss_*,
dr_focal_loss_*).  Every function reads the reference module's own parameters, so gradients land in `.grad` of that module.

    img, pcd = fusion_module(model.transformer, img_feats, img_dino, img_pixels, pcd_feats, pcd_points)     # EXP/model.py:386-392
    conf, src_idx, tgt_idx, w = matching_head_2d3d(model.coarse_matching, pcd, img, src_mask, tgt_mask)    # EXP/model.py:548
    losses = coarse_matching_loss(loss_fn.c_loss, output_dict)                                              # EXP/loss.py:30-75

    loss, recall = fine_matching_loss(loss_fn.f_loss, data_dict, output_dict)                                # EXP/loss.py:157-215
    warped, tgt, R_forwd, t_forwd = noising_warp(model, s_pcd, t_pcd_da, src_mask, tgt_mask_da, x)          # EXP/model.py:830-846

The Fourier embeddings of the pixel / point positions are constants of the graph by default (the reference's own FourierEmbedding module
computes them); `fusion_module(..., embed_grad=True)` computes the point embedding with gradients enabled, so that the gradient of the warped
points (noising_warp: Sinkhorn -> top-K Procrustes -> R, t) reaches denoising_coarse_matching.bin_score as in the reference.  The image
backbone (with DINOv2 / Depth-Anything) and the inline GT retry ladder stay the reference's code: gradients reach the backbones through the
returned input gradients.
"""
import sys

import torch

from . import lib
from .autograd import _MatchingHeadG, _Procrustes, _SinkhornConf, focal_loss, _mm


def _det(t):
    return t.detach().float().contiguous()


def _tr(x):
    return x.transpose(-1, -2).contiguous()


def _pad4(x):
    pad = (-x.shape[-1]) % 4
    return torch.nn.functional.pad(x, (0, pad)) if pad else x


class _Linear(torch.autograd.Function):
    """nn.Linear (+ ReLU) on the library's GEMM: y = [relu](x W^T + b); backward: g W, g^T x and the bias gradient as g^T 1 (both on the GEMM:
    one fixed summation order)"""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        lead, K = x.shape[:-1], x.shape[-1]
        x2 = _pad4(_det(x).reshape(-1, K))
        W = _pad4(_det(weight))
        y = lib.linear_ex(x2, W, _det(bias) if bias is not None else None, epilogue=1 if relu else 0)
        ctx.save_for_backward(x2, W, y if relu else None)
        ctx.meta = (lead, K, relu, bias is not None)
        return y.view(*lead, W.shape[0])

    @staticmethod
    def backward(ctx, g):
        x2, W, y = ctx.saved_tensors
        lead, K, relu, has_b = ctx.meta
        g = g.reshape(-1, W.shape[0]).contiguous().float()
        if relu:
            g = lib.relu_backward(y, g)
        gx = lib.linear(g, _tr(W))[:, :K].reshape(*lead, K) if ctx.needs_input_grad[0] else None
        gW = _mm(_tr(g), _tr(x2))[:, :K]
        gb = _mm(_tr(g), torch.ones(1, g.shape[0], device=g.device)).reshape(-1) if has_b else None
        return gx, gW, gb, None


def linear(x, layer, relu=False):
    """differentiable nn.Linear `layer` (+ ReLU) on the device"""
    return _Linear.apply(x, layer.weight, layer.bias, relu)


def _fusion_layer_params(layer):
    """the 16 parameters of a vision3d TransformerLayer in lib.FUSION_LAYER_KEYS order"""
    a, o = layer.attention, layer.output
    mha = a.attention
    return (mha.q_token_layer.weight, mha.q_token_layer.bias, mha.k_token_layer.weight, mha.k_token_layer.bias, mha.v_token_layer.weight,
            mha.v_token_layer.bias, a.linear.weight, a.linear.bias, a.norm.weight, a.norm.bias, o.expand.weight, o.expand.bias,
            o.squeeze.weight, o.squeeze.bias, o.norm.weight, o.norm.bias)


class _FusionLayer(torch.autograd.Function):
    """TransformerLayer.forward(x, y, y, k_masks) (vision3d/layers/transformer.py:241-301): one library call forward, one backward.  A
    self-attention call passes the same tensor as x and y: autograd adds the two input gradients."""

    @staticmethod
    def forward(ctx, x, y, y_mask, H, *params):
        C = x.shape[-1]
        xd = _det(x)
        yd = xd if y is x else _det(y)
        ps = [_det(p) for p in params]
        out, saved = lib.fusion_layer_train_forward(ps, C, H, xd, yd, y_mask)
        ctx.save_for_backward(xd, yd, saved, *ps)
        ctx.H, ctx.y_mask, ctx.self_call = H, y_mask, y is x
        return out

    @staticmethod
    def backward(ctx, g):
        xd, yd, saved, *ps = ctx.saved_tensors
        if ctx.self_call:
            yd = xd
        gx, gy, grads = lib.fusion_layer_backward(ps, xd.shape[-1], ctx.H, xd, yd, ctx.y_mask, saved, g.contiguous().float())
        return (gx, gy, None, None) + tuple(grads)


def fusion_layer(layer, x, y, y_mask=None, n_head=None):
    """differentiable vision3d TransformerLayer: x [B,L,C] attends y [B,S,C]; y_mask [B,S] True = a valid key (None: every key)"""
    H = n_head or int(layer.attention.attention.num_heads)
    return _FusionLayer.apply(x, y, y_mask, H, *_fusion_layer_params(layer))


def fusion_module(module, img_feats, img_dino, img_pixels, pcd_feats, pcd_points, embed_grad=False):
    """CrossModalFusionModule.forward (EXP/fusion_module.py:61-107) from the module's own parameters, no masks (the path passes none,
    EXP/model.py:386-392, 615-621) -> (img [B,M,C], pcd [B,N,C]).  Gradients: every parameter, and whichever of img_feats / img_dino / pcd_feats
    requires grad; the positions are constants -- unless embed_grad: then the point embedding (vision3d's FourierEmbedding is differentiable in
    its input) is computed with gradients enabled and pcd_points receives its gradient through pcd_emb_proj."""
    img = torch.cat([linear(img_feats, module.img_in_proj, relu=True), linear(img_dino, module.img_in_proj_dino, relu=True)], dim=-1)  # relu(cat)
    img = linear(img, module.img_in_proj_all)
    pcd = linear(pcd_feats, module.pcd_in_proj)
    if module.use_embedding:
        with torch.no_grad():
            e_img = module.embedding(img_pixels.float())
            if not embed_grad:
                e_pcd = module.embedding((pcd_points - pcd_points.mean(dim=1)).float())    # fusion_module.py:55-59
        if embed_grad:
            e_pcd = module.embedding((pcd_points - pcd_points.mean(dim=1)).float())
        img = img + linear(e_img, module.img_emb_proj)
        pcd = pcd + linear(e_pcd, module.pcd_emb_proj)
    for i, block in enumerate(module.blocks):
        layer = module.transformer[i]
        if block == "self":
            img = fusion_layer(layer, img, img)
            pcd = fusion_layer(layer, pcd, pcd)
        else:
            img = fusion_layer(layer, img, pcd)
            pcd = fusion_layer(layer, pcd, img)
    return linear(img, module.out_proj), linear(pcd, module.out_proj)


def matching_head_2d3d(module, src_feats, tgt_feats, src_mask, tgt_mask, mutual=True):
    """Matching.forward, sinkhorn branch (EXP/matching.py:91-147): src_proj on both sides, / sqrt(C), mask, Sinkhorn (module.skh_iters) ->
    (conf [B,N,M], src_indices, tgt_indices, weights); conf is differentiable (dr_sinkhorn_backward_f32), the mutual top-1 read-out is a value
    (dr_mutual_topk_select_f32; above its tile size see _mutual_top1_large)."""
    conf = _MatchingHeadG.apply(src_feats, tgt_feats, module.src_proj.weight, module.bin_score, "none", None, None, None, None, src_mask, tgt_mask,
                                "sinkhorn", int(module.skh_iters), 1.0)
    with torch.no_grad():
        c = conf.detach().squeeze(0)
        if c.dim() == 2 and c.numel() <= _TOPK_MAX_ELEMS:
            si, ti, w = lib.batch_mutual_topk_select(c, 1, largest=True, threshold=None, mutual=mutual)
        else:
            si, ti, w = _mutual_top1_large(conf.detach().float(), mutual)
    return conf, si, ti, w


def _mutual_top1_large(conf, mutual):
    """the mutual read-out beyond the tile dr_mutual_topk_select_f32 holds in LDS, on dr_mutual_match_f32: entries > 0 that are their row's and
    their column's maximum (mutual = False -- the union of row and column top-1 -- has no kernel at this size and raises).  Inside the masks every Sinkhorn entry is > 0, so a valid row's arg-maximum is the reference's; the rows / columns
    outside the masks are all zeros, where torch.topk picks one of the tied entries in an unspecified order -- those are not listed.  The list
    length is read back (as the reference's boolean indexing does); a list longer than its bound raises."""
    B, N, M = conf.shape
    if not mutual:
        raise RuntimeError("matching read-out with mutual=False above %d entries is not supported" % _TOPK_MAX_ELEMS)
    cap = min(N, M)
    m, mc, cnt, _ = lib.mutual_match(conf, thr=0.0, mutual=True, cap=cap)
    n = int(cnt[0])
    if n > cap:
        raise RuntimeError("mutual top-1 read-out: %d entries exceed the bound %d (tied maxima)" % (n, cap))
    return m[0, :n, 1], m[0, :n, 2], mc[0, :n]


_TOPK_MAX_ELEMS = 64 * 1024 * 4   # dr_mutual_topk_select_f32: two bit planes of N M bits in 64 KiB of LDS


class _L2Normalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eps):
        y, n = lib.l2_normalize(_det(x), eps)
        ctx.save_for_backward(y, n)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, g):
        y, n = ctx.saved_tensors
        return lib.l2_normalize_backward(y, n, g, ctx.eps), None


def normalize(x, eps=1e-12):
    """F.normalize(x, p=2, dim=1) of rows x [R,C] (EXP/model.py:552-553)"""
    return _L2Normalize.apply(x, float(eps))


class _CircleLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, pcd, ii, jj, mn, mx, params):
        ctx.save_for_backward(_det(img), _det(pcd), ii, jj, mn, mx)
        ctx.params = params
        return lib.circle_loss(img, pcd, ii, jj, mn, mx, params)

    @staticmethod
    def backward(ctx, g):
        img, pcd, ii, jj, mn, mx = ctx.saved_tensors
        _, gi, gp = lib.circle_loss_backward(img, pcd, ii, jj, mn, mx, ctx.params, g)
        return gi, gp, None, None, None, None, None


def circle_loss(img_feats, pcd_feats, img_idx, pcd_idx, min_overlaps, max_overlaps, params):
    """the weighted circle loss of CoarseMatchingLoss on normalised features img [M,C] / pcd [N,C] (lib.circle_params)"""
    return _CircleLoss.apply(img_feats, pcd_feats, img_idx, pcd_idx, min_overlaps, max_overlaps, params)


def _circle_params(loss_module):
    c = loss_module.weighted_circle_loss
    return lib.circle_params(c.pos_margin, c.neg_margin, c.pos_optimal, c.neg_optimal, c.log_scale, loss_module.positive_overlap,
                             loss_module.negative_overlap)


def coarse_matching_loss(loss_module, output_dict):
    """CoarseMatchingLoss.forward (EXP/loss.py:30-75) -> (loss_circle, loss_circle_denoising, loss_focal, loss_matrix_gt_hat), differentiable
    where the reference's are.  The max overlaps are read from the MIN list, as the reference does (EXP/loss.py:36)."""
    params = _circle_params(loss_module)
    ii, jj = output_dict["gt_img_node_corr_indices"], output_dict["gt_pcd_node_corr_indices"]
    mn = output_dict["gt_node_corr_min_overlaps"]
    mx = output_dict["gt_node_corr_min_overlaps"]
    loss_circle = circle_loss(output_dict["img_feats_c"], output_dict["pcd_feats_c"], ii, jj, mn, mx, params)
    loss_circle_dn = circle_loss(output_dict["img_feats_c_denoising"], output_dict["pcd_feats_c_denoising"], ii, jj, mn, mx, params)
    conf_gt = output_dict["matrix_gt"]
    hp = (loss_module.focal_alpha, loss_module.focal_gamma, loss_module.pos_w, loss_module.neg_w)
    loss_focal = focal_loss(output_dict["conf_matrix_pred"], conf_gt, *hp)
    loss_gt_hat = focal_loss(output_dict["conf_matrix_gt_hat"], conf_gt, *hp)
    return loss_circle, loss_circle_dn, loss_focal, loss_gt_hat


class _FineLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img_feats, pcd_feats, img_points, pcd_points, pcd_pixels, transform, sel_pixels, sel_indices, image_w, params):
        loss, recall, saved = lib.fine_loss(img_points, img_feats, pcd_points, pcd_pixels, pcd_feats, transform, sel_pixels, sel_indices, image_w, params)
        ctx.save_for_backward(_det(img_feats), _det(pcd_feats), img_points, pcd_points, pcd_pixels, transform, sel_pixels, sel_indices, saved)
        ctx.image_w, ctx.params, ctx.dtypes = image_w, params, (img_feats.dtype, pcd_feats.dtype)
        ctx.mark_non_differentiable(recall)
        return loss, recall

    @staticmethod
    def backward(ctx, g, _g_recall):
        fi, fp, ip, pp, px, T, sp, si, saved = ctx.saved_tensors
        gi, gp = lib.fine_loss_backward(ip, fi, pp, px, fp, T, sp, si, ctx.image_w, ctx.params, saved, g)
        return gi.to(ctx.dtypes[0]), gp.to(ctx.dtypes[1]), None, None, None, None, None, None, None, None     # (the kernels are float32)


def _fine_params(loss_module):
    c = loss_module.circle_loss
    return lib.fine_params(loss_module.pos_radius_3d, loss_module.neg_radius_3d, loss_module.pos_radius_2d, loss_module.neg_radius_2d,
                           c.pos_margin, c.neg_margin, c.pos_optimal, c.neg_optimal, c.log_scale)


def fine_loss(img_feats, pcd_feats, img_points, pcd_points, pcd_pixels, transform, img_sel_pixels, pcd_sel_indices, image_w, params):
    """the fine loss on given selections (lib.fine_params) -> (loss, recall); differentiable in img_feats [HW,C] and pcd_feats [N,C]"""
    return _FineLoss.apply(img_feats, pcd_feats, img_points, pcd_points, pcd_pixels, transform, img_sel_pixels, pcd_sel_indices, int(image_w), params)


def fine_matching_loss(loss_module, data_dict, output_dict):
    """FineMatchingLoss.forward (EXP/loss.py:157-215) -> (loss, recall).  The sub-sampling above max_correspondences is the reference's own
    random_choice (vision3d.ops, numpy's global RNG), looked up in the module that defines the loss class: the random stream is the reference's."""
    assert data_dict["batch_size"] == 1, "Only support the batch_size of 1."
    sel_pixels, sel_indices = data_dict["img_corr_pixels"], data_dict["pcd_corr_indices"]
    if sel_indices.shape[0] > loss_module.max_correspondences:
        random_choice = vars(sys.modules[type(loss_module).__module__])["random_choice"]
        sel = random_choice(sel_indices.shape[0], size=loss_module.max_correspondences, replace=False)
        sel_pixels, sel_indices = sel_pixels[sel], sel_indices[sel]
    return fine_loss(output_dict["img_feats_f"], output_dict["pcd_feats_f"], output_dict["img_points_f"], output_dict["pcd_points_f"],
                     output_dict["pcd_pixels_f"], data_dict["transform"], sel_pixels, sel_indices, data_dict["image_w"], _fine_params(loss_module))


def soft_procrustes(layer, conf, src_pcd, tgt_pcd, src_mask, tgt_mask):
    """SoftProcrustesLayer.forward of the 2D-3D model (EXP/procrustes.py:48-93: K from the mask sums) on dr_procrustes_f32 ->
    (R, t, R_forwd, t_forwd, condition, solution_mask); differentiable in conf (dr_procrustes_backward_f32) where it requires grad.  On a 0 / 1
    matrix with more than K ones the reference's torch.sort leaves the choice among the equal entries unspecified; the device takes the lowest
    flat indices (parity-unpinned)."""
    return _Procrustes.apply(conf.float(), src_pcd.float().contiguous(), tgt_pcd.float().contiguous(), src_mask, tgt_mask, float(layer.sample_rate),
                             float(layer.max_condition_num), True)


def noising_warp(model, s_pcd, t_pcd, src_mask, tgt_mask, matrix):
    """MATR2D3D.get_warped_from_noising_matching3D3D (EXP/model.py:830-846): masked fill (IN PLACE, as the reference) -> Sinkhorn with
    denoising_coarse_matching.bin_score -> top-K Procrustes -> R_forwd s + t_forwd, as one autograd chain (dr_sinkhorn_f32, dr_procrustes_f32;
    backward dr_procrustes_backward_f32 -> dr_sinkhorn_backward_f32) -> (warped [B,N,3], t_pcd float32, R_forwd, t_forwd).  Where the condition
    gate fails R_forwd, t_forwd are the identity and no gradient flows."""
    head = model.denoising_coarse_matching
    if src_mask is not None:
        matrix.masked_fill_(~(src_mask[..., None] * tgt_mask[:, None]).bool(), float("-inf"))
    conf = _SinkhornConf.apply(matrix.float(), head.bin_score, int(head.skh_iters), src_mask, tgt_mask)
    _, _, Rf, tf, _, _ = soft_procrustes(model.denoising_soft_procrustes, conf, s_pcd, t_pcd, src_mask, tgt_mask)
    warped = (torch.matmul(Rf, s_pcd.float().transpose(1, 2)) + tf).transpose(1, 2)
    return warped, t_pcd.type(torch.float32), Rf, tf


_SCHEDULES = {}     # (timesteps, device) -> (sqrt(alphas_cumprod), sqrt(1 - alphas_cumprod)), float64, on the device


def _schedule(timesteps, device):
    key = (int(timesteps), str(device))
    hit = _SCHEDULES.get(key)
    if hit is None:
        import math
        with torch.no_grad():                                                # cosine_beta_schedule (EXP/model.py:109-121) and q_sample's tables (:128-134)
            x = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64)
            ac = torch.cos(((x / timesteps) + 0.008) / (1 + 0.008) * math.pi * 0.5) ** 2
            ac = ac / ac[0]
            betas = torch.clip(1 - (ac[1:] / ac[:-1]), 0, 0.999).to(device)
            alphas_cumprod = torch.cumprod(1. - betas, dim=0)
            hit = _SCHEDULES[key] = (torch.sqrt(alphas_cumprod), torch.sqrt(1. - alphas_cumprod))
    return hit


@torch.no_grad()
def q_sample(x_start, t, noise=None, timesteps=1000):
    """q_sample (EXP/model.py:123-139) with the 1 000-step schedule tables built once per (timesteps, device): the same float64 torch ops in the
    same order, so the result is bit-equal; the two coefficients are gathered by `t` on the device (no host read)."""
    if noise is None:
        noise = torch.randn_like(x_start)
    sa, so = _schedule(timesteps, x_start.device)
    shape = (t.shape[0],) + (1,) * (len(x_start.shape) - 1)
    return sa.gather(-1, t).reshape(shape) * x_start + so.gather(-1, t).reshape(shape) * noise
