"""The 2D-3D model's point backbone on the device: PointBackbone.forward (EXP/point_backbone.py:39-95; vision3d's KPConvBlock / KPResidualBlock /
UnaryBlockPackMode / GroupNormPackMode, local_maxpool_pack_mode and knn_interpolate_pack_mode) as a chain of torch.autograd.Functions whose
forward AND backward run in libdiffreg_hip.  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.

    feats_list = point_backbone(model.pcd_backbone, feats, data_dict)      # [out_proj(latent_s1) [N0,128], latent_s2 [N1,256], feats_s3 [N2,512]]

Per KPConv: dr_kpconv_gather_f32 (its backward for the input gradient) and ONE product on dr_linear_ex_f32 with W2[co][k Cin + c] = weights[k][c][co]
and the bias in the epilogue (K Cin = 15 at Cin = 1: the gather's row and W2 padded to 16 with zeros).  Every nn.Linear is a product on the same GEMM.
GroupNorm + residual sum + LeakyReLU of a block's tail is ONE dr_group_norm_apply_f32 after the statistics; the strided shortcut is dr_gather_pool_f32;
the decoder's kNN interpolation writes straight into the left columns of the concatenation buffer (dr_knn_interpolate_f32).  The module's own
buffers and parameters are read on every call (kernel points are never regenerated); gradients land in their `.grad`.  Under torch.no_grad() no
graph is recorded and nothing is read back to the host (the whole forward can be captured into a graph).  Neighbour lists wider than 64 are refused
(RuntimeError), never truncated.
"""
import torch

from . import lib
from .backbone_autograd import _KPGather, _Linear, _Pool, _w2


class _GroupNorm(torch.autograd.Function):
    """act( GN_a(a) + [GN_b(b) | b | 0] ): GroupNormPackMode (+ the residual sum of KPResidualBlock) + LeakyReLU(slope) or no activation"""

    @staticmethod
    def forward(ctx, a, gamma_a, beta_a, b, gamma_b, beta_b, G, eps, slope):
        ad = a.detach().float().contiguous()
        bd = b.detach().float().contiguous() if b is not None else None
        ga_, ba_ = gamma_a.detach().contiguous(), beta_a.detach().contiguous()
        norm_b = gamma_b is not None
        gb_, bb_ = (gamma_b.detach().contiguous(), beta_b.detach().contiguous()) if norm_b else (None, None)
        sa = lib.group_norm_stats(ad, G, eps)
        sb = lib.group_norm_stats(bd, G, eps) if norm_b else None
        out = lib.group_norm_apply(ad, sa, ga_, ba_, bd, sb, gb_, bb_, slope)
        e = ad.new_empty(0)
        ctx.save_for_backward(ad, sa[0], sa[1], ga_, bd if bd is not None else e, *(sb if norm_b else (e, e)), gb_ if norm_b else e, out)
        ctx.cfg = (b is not None, norm_b, slope)
        return out

    @staticmethod
    def backward(ctx, g):
        a, ma, ra, ga_, b, mb, rb, gb_, out = ctx.saved_tensors
        has_b, norm_b, slope = ctx.cfg
        da, db, dga, dba, dgb, dbb = lib.group_norm_backward(g.float(), out, a, (ma, ra), ga_, b if has_b else None, (mb, rb) if norm_b else None,
                                                             gb_ if norm_b else None, slope)
        return da, dga, dba, db, dgb, dbb, None, None, None


class _KnnCat(torch.autograd.Function):
    """cat([knn_interpolate_pack_mode(q, s, x, inds), skip], 1): the interpolation is written into the left columns of the buffer"""

    @staticmethod
    def forward(ctx, x, skip, q, s, inds):
        xd = x.detach().float().contiguous()
        C = xd.shape[1]
        buf = torch.empty(q.shape[0], C + skip.shape[1], device=xd.device)
        lib.knn_interpolate(q, s, inds, xd, out=buf, col=0)
        buf[:, C:].copy_(skip.detach())
        ctx.save_for_backward(q, s, inds)
        ctx.C = C
        return buf

    @staticmethod
    def backward(ctx, g):
        q, s, inds = ctx.saved_tensors
        g = g.float().contiguous()
        C = ctx.C
        gx = lib.knn_interpolate_backward(q, s, inds, g, C, col=0) if ctx.needs_input_grad[0] else None
        return gx, g[:, C:], None, None, None


def _slope(act):
    """LeakyReLU -> its slope; nn.Identity (act_cfg 'None') -> None"""
    if isinstance(act, torch.nn.LeakyReLU):
        return float(act.negative_slope)
    if isinstance(act, torch.nn.Identity):
        return None
    raise NotImplementedError("point backbone on the device: activation %s has no device form" % type(act).__name__)


def _gn(norm):
    """GroupNormPackMode -> its nn.GroupNorm"""
    gn = norm.norm
    if not isinstance(gn, torch.nn.GroupNorm) or not gn.affine:
        raise NotImplementedError("point backbone on the device: normalisation %s has no device form" % type(gn).__name__)
    return gn


def _norm_act(a, norm, act, b=None, norm_b=None):
    """act( GN(a) + [GN_b(b) | b | 0] )"""
    gn = _gn(norm)
    gnb = _gn(norm_b) if norm_b is not None else None
    if gnb is not None and (gnb.num_groups != gn.num_groups or gnb.eps != gn.eps):
        raise NotImplementedError("point backbone on the device: the two GroupNorms of a block tail must agree")
    return _GroupNorm.apply(a, gn.weight, gn.bias, b, gnb.weight if gnb is not None else None, gnb.bias if gnb is not None else None,
                            gn.num_groups, gn.eps, _slope(act))


def _linear(x, lin):
    return _Linear.apply(x, lin.weight, lin.bias)


def _kpconv(conv, q, s, x, inds, counts):
    """KPConv.forward (vision3d/layers/kpconv.py:96-151): gather + one GEMM, bias in the epilogue"""
    if getattr(conv, "groups", 1) != 1:
        raise NotImplementedError("point backbone on the device: grouped KPConv has no device form")
    if counts is not None:
        counts.append(lib.kpconv_neighbor_count(inds, x.detach().float().contiguous(), s.shape[0]))
    wf = _KPGather.apply(x, q, s, inds, conv.kernel_points.detach().float().contiguous(), float(conv.sigma), "linear", "sum")
    return _Linear.apply(wf, _w2(conv.weights), conv.bias)


def _kpconv_block(blk, q, s, x, inds, counts):
    """KPConvBlock (kpconv.py:203-207): act(GN(KPConv(x)))"""
    return _norm_act(_kpconv(blk.conv, q, s, x, inds, counts), blk.norm, blk.act)


def _unary(blk, x):
    """UnaryBlockPackMode (unary_block.py:26-30): act(GN(Linear(x)))"""
    return _norm_act(_linear(x, blk.mlp), blk.norm, blk.act)


def _residual(blk, q, s, x, inds, counts):
    """KPResidualBlock (kpconv.py:266-280): act(GN(unary2(conv(unary1(x)))) + shortcut), the tail in one apply pass"""
    y = _unary(blk.unary1, x)
    y = _kpconv_block(blk.conv, q, s, y, inds, counts)
    y = _linear(y, blk.unary2.mlp)                                              # unary2: Linear + GN, no activation
    sc = _Pool.apply(x, inds, False) if blk.strided else x                     # local_maxpool_pack_mode (zero shadow row)
    if isinstance(blk.unary_shortcut, torch.nn.Identity):
        return _norm_act(y, blk.unary2.norm, blk.act, sc)
    return _norm_act(y, blk.unary2.norm, blk.act, _linear(sc, blk.unary_shortcut.mlp), blk.unary_shortcut.norm)


def point_backbone(module, feats, data_dict, counts=None):
    """PointBackbone.forward(feats, data_dict) of `module` (the reference's module, or any module with its attribute names) on the device ->
    [out_proj(latent_s1), latent_s2, feats_s3].  `counts`: a list that receives each KPConv call's neighbour counts (int32, device), in call order."""
    dev = feats.device
    pts = [p.to(dev, torch.float32).contiguous() for p in data_dict["points"][:3]]
    nb = [i.to(dev, torch.int64).contiguous() for i in data_dict["neighbors"][:3]]
    sub = [i.to(dev, torch.int64).contiguous() for i in data_dict["subsampling"][:2]]
    up = [i.to(dev, torch.int64).contiguous() for i in data_dict["upsampling"][:2]]
    m = module
    s1 = _kpconv_block(m.encoder1_1, pts[0], pts[0], feats.float().contiguous(), nb[0], counts)
    s1 = _residual(m.encoder1_2, pts[0], pts[0], s1, nb[0], counts)
    s2 = _residual(m.encoder2_1, pts[1], pts[0], s1, sub[0], counts)
    s2 = _residual(m.encoder2_2, pts[1], pts[1], s2, nb[1], counts)
    s2 = _residual(m.encoder2_3, pts[1], pts[1], s2, nb[1], counts)
    s3 = _residual(m.encoder3_1, pts[2], pts[1], s2, sub[1], counts)
    s3 = _residual(m.encoder3_2, pts[2], pts[2], s3, nb[2], counts)
    s3 = _residual(m.encoder3_3, pts[2], pts[2], s3, nb[2], counts)
    l2 = _unary(m.decoder2, _KnnCat.apply(s3, s2, pts[1], pts[2], up[1]))
    l1 = _unary(m.decoder1, _KnnCat.apply(l2, s1, pts[0], pts[1], up[0]))
    return [_linear(l1, m.out_proj), l2, s3]
