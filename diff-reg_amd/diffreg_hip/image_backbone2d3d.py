"""The 2D-3D model's image backbone on the device, forward and backward: ImageBackbone.forward (EXP/image_backbone.py:254-289; BasicBlock :9-66,
vision3d's ConvBlock, vision3d/layers/conv_block.py:118-125) composed from dr_conv2d_rows_f32, dr_resize_rows_f32 and the GroupNorm entries of
the point backbone.  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.

    ib = DeviceImageBackbone(model.img_backbone)           # reads the module: kernel sizes, strides, paddings, channel counts, norm / act kinds
    rows, sizes = ib.forward_rows(x, dino_feat)            # 4 x [H W, C] token rows (finest first) and their (H, W)
    feats_list = ib.forward(x, dino_feat)                  # the reference's list of contiguous [1, C, H, W] tensors

Inside, every activation is token rows [H W, C] float32 (NHWC): nn.GroupNorm(G, C) over [1, C, H, W] is dr_group_norm_stats_f32(N = H W, C, G)
over them, a ConvBlock with GroupNorm is conv -> stats -> apply, the tail act(identity + GN(conv2)) of a BasicBlock is ONE apply pass (the
identity raw at stride 1, through its own statistics / gamma / beta when it is a strided ConvBlock), and the four sums of the decoder ride on
the `addend` of the conv or the resample.  DINO's [1, h, w, C] grid already is rows.  Weights are packed [Cout, k, k, Cin] once per conv and
re-packed when the parameter's `_version` or storage changes.  Workspaces come from torch's allocator; nothing is read back to the host, so the
call can be captured into a graph.  Anything without a device form -- another norm or activation, groups != 1, a padding mode other than zeros,
a non-affine GroupNorm, dropout, act-before-norm -- raises NotImplementedError when the module is bound, never at call time.

With gradients enabled, forward_rows / forward record an autograd graph of three Functions -- _Conv2dRows (dr_conv2d_rows_f32 and its two
gradients), _ResizeRows (dr_resize_rows_f32 and its gather backward), pcd_backbone2d3d._GroupNorm -- in the same structure as the inference arm
(the BasicBlock tail one apply pass, the decoder sums on the addends), so its outputs are bit-equal to the inference arm's; gradients land in
the .grad of the module's own parameters and reach x and dino_feat when those require them.  The data gradient of a convolution is skipped when
its input needs none (the stem).

bind(module) / overlay2d3d.accelerate(image_backbone=True): in training mode or with gradients enabled the bound forward calls the module's own
forward unchanged.  bind(module, grad=True) / accelerate(image_backbone_grad=True): the device path runs there as well (GroupNorm has no running
statistics and dropout is refused at bind time, so training and eval mode compute the same function).
"""
import torch
import torch.nn as nn

from . import lib
from .pcd_backbone2d3d import _GroupNorm

_WHO = "image backbone on the device: "


def _pair(v, what):
    if isinstance(v, (tuple, list)):
        if len(set(int(a) for a in v)) != 1:
            raise NotImplementedError(_WHO + "%s %s is not square" % (what, tuple(v)))
        return int(v[0])
    return int(v)


class _Conv:
    """one ConvBlock read from the module: its nn.Conv2d, its GroupNorm (or None) and its LeakyReLU slope (or None)"""

    def __init__(self, blk):
        conv = getattr(blk, "conv", None)
        if not isinstance(conv, nn.Conv2d):
            raise NotImplementedError(_WHO + "%s is not a Conv2d" % type(conv).__name__)
        if conv.groups != 1:
            raise NotImplementedError(_WHO + "groups = %d has no device form" % conv.groups)
        if conv.padding_mode != "zeros" or isinstance(conv.padding, str):
            raise NotImplementedError(_WHO + "padding %r / %r has no device form" % (conv.padding_mode, conv.padding))
        if getattr(blk, "act_before_norm", False):
            raise NotImplementedError(_WHO + "act-before-norm has no device form")
        if not isinstance(getattr(blk, "dropout", nn.Identity()), nn.Identity):
            raise NotImplementedError(_WHO + "dropout has no device form")
        self.conv = conv
        self.k = _pair(conv.kernel_size, "kernel")
        self.stride, self.padding, self.dilation = _pair(conv.stride, "stride"), _pair(conv.padding, "padding"), _pair(conv.dilation, "dilation")
        norm = blk.norm
        if isinstance(norm, nn.Identity):
            self.norm = None
        elif isinstance(norm, nn.GroupNorm) and norm.affine:
            self.norm = norm
        else:
            raise NotImplementedError(_WHO + "normalisation %s has no device form" % type(norm).__name__)
        self.slope = _slope(blk.act)
        if self.norm is None and self.slope is not None:
            raise NotImplementedError(_WHO + "an activation without a GroupNorm in front has no device form")
        self._key, self._packed = None, None
        self._key_t, self._packed_t = None, None

    def weight(self):
        w = self.conv.weight
        key = (w._version, w.data_ptr(), w.device, tuple(w.shape))
        if key != self._key:
            self._packed, self._key = lib.pack_conv_weight(w), key
        return self._packed

    def weight_t(self):
        """the [Cin, k k Cout] pack of the data gradient, re-packed like weight()"""
        w = self.conv.weight
        key = (w._version, w.data_ptr(), w.device, tuple(w.shape))
        if key != self._key_t:
            self._packed_t, self._key_t = lib.pack_conv_weight_t(w), key
        return self._packed_t

    def raw_grad(self, x, size, addend=None):
        """raw() recorded for autograd"""
        return _Conv2dRows.apply(x, self.conv.weight, self.conv.bias, addend, self, size), tuple(lib.conv_out_size(n, self.k, self.stride, self.padding, self.dilation) for n in size)

    def grad(self, x, size, addend=None):
        """__call__ recorded for autograd"""
        y, osz = self.raw_grad(x, size, addend)
        if self.norm is None:
            return y, osz
        gn = self.norm
        return _GroupNorm.apply(y, gn.weight, gn.bias, None, None, None, gn.num_groups, gn.eps, self.slope), osz

    def raw(self, x, size, addend=None):
        """the convolution alone (+ bias, + addend)"""
        b = self.conv.bias
        return lib.conv2d_rows(x, size, self.weight(), self.k, None if b is None else b.detach(), self.stride, self.padding, self.dilation, addend)

    def __call__(self, x, size, addend=None):
        """ConvBlock.forward: act(GN(conv(x)))"""
        y, osz = self.raw(x, size, addend)
        if self.norm is None:
            return y, osz
        gn = self.norm
        st = lib.group_norm_stats(y, gn.num_groups, gn.eps)
        return lib.group_norm_apply(y, st, gn.weight.detach(), gn.bias.detach(), slope=self.slope), osz


class _Conv2dRows(torch.autograd.Function):
    """conv(x) + bias + addend on token rows; backward: dr_conv2d_rows_backward_data_f32 (skipped when x needs no gradient),
    dr_conv2d_rows_backward_weight_f32, and the gradient itself for the addend"""

    @staticmethod
    def forward(ctx, x, weight, bias, addend, cv, size):
        xd = x.detach()
        out, _ = lib.conv2d_rows(xd, size, cv.weight(), cv.k, None if bias is None else bias.detach(), cv.stride, cv.padding, cv.dilation,
                                 None if addend is None else addend.detach())
        ctx.save_for_backward(xd)
        ctx.cv, ctx.size = cv, size
        return out

    @staticmethod
    def backward(ctx, g):
        (xd,) = ctx.saved_tensors
        cv, size = ctx.cv, ctx.size
        g = g.float().contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = lib.conv2d_rows_backward_data(g, size, cv.weight_t(), cv.k, cv.stride, cv.padding, cv.dilation)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            gw, gb = lib.conv2d_rows_backward_weight(xd, size, g, cv.k, cv.stride, cv.padding, cv.dilation, need_weight=ctx.needs_input_grad[1],
                                                     need_bias=ctx.needs_input_grad[2])
        return gx, gw, gb, (g if ctx.needs_input_grad[3] else None), None, None


class _ResizeRows(torch.autograd.Function):
    """addend + bilinear(x) on token rows; backward: the gather dr_resize_rows_backward_f32, and the gradient itself for the addend"""

    @staticmethod
    def forward(ctx, x, addend, src, dst):
        ctx.src, ctx.dst = src, dst
        return lib.resize_rows(x.detach(), src, dst, addend=None if addend is None else addend.detach())

    @staticmethod
    def backward(ctx, g):
        g = g.float().contiguous()
        gx = lib.resize_rows_backward(g, ctx.src, ctx.dst) if ctx.needs_input_grad[0] else None
        return gx, (g if ctx.needs_input_grad[1] else None), None, None


def _slope(act):
    if isinstance(act, nn.LeakyReLU):
        return float(act.negative_slope)
    if isinstance(act, nn.Identity):
        return None
    raise NotImplementedError(_WHO + "activation %s has no device form" % type(act).__name__)


class _Block:
    """BasicBlock (EXP/image_backbone.py:9-66): act(identity(x) + conv2(conv1(x))), the tail in one apply pass"""

    def __init__(self, blk):
        self.conv1, self.conv2 = _Conv(blk.conv1), _Conv(blk.conv2)
        if self.conv2.norm is None or self.conv2.slope is not None:
            raise NotImplementedError(_WHO + "a BasicBlock whose conv2 is not Conv + GroupNorm without activation has no device form")
        self.slope = _slope(blk.act)
        if isinstance(blk.identity, nn.Identity):
            self.identity = None
        else:
            self.identity = _Conv(blk.identity)
            a, b = self.conv2.norm, self.identity.norm
            if b is None or self.identity.slope is not None or a.num_groups != b.num_groups:
                raise NotImplementedError(_WHO + "the strided identity must be Conv + GroupNorm (same groups as conv2) without activation")

    def __call__(self, x, size):
        r, osz = self.conv1(x, size)
        r, _ = self.conv2.raw(r, osz)
        gn = self.conv2.norm
        st = lib.group_norm_stats(r, gn.num_groups, gn.eps)
        if self.identity is None:
            return lib.group_norm_apply(r, st, gn.weight.detach(), gn.bias.detach(), x, slope=self.slope), osz
        i, _ = self.identity.raw(x, size)
        gi = self.identity.norm
        sti = lib.group_norm_stats(i, gi.num_groups, gi.eps)
        return lib.group_norm_apply(r, st, gn.weight.detach(), gn.bias.detach(), i, sti, gi.weight.detach(), gi.bias.detach(), slope=self.slope), osz

    def grad(self, x, size):
        """__call__ recorded for autograd: the tail is one _GroupNorm node"""
        r, osz = self.conv1.grad(x, size)
        r, _ = self.conv2.raw_grad(r, osz)
        gn = self.conv2.norm
        if self.identity is None:
            return _GroupNorm.apply(r, gn.weight, gn.bias, x, None, None, gn.num_groups, gn.eps, self.slope), osz
        i, _ = self.identity.raw_grad(x, size)
        gi = self.identity.norm
        return _GroupNorm.apply(r, gn.weight, gn.bias, i, gi.weight, gi.bias, gn.num_groups, gn.eps, self.slope), osz


class DeviceImageBackbone:
    def __init__(self, module):
        """binds every layer of `module` (the reference's ImageBackbone, or any module with its attribute names); NotImplementedError for anything
        the device path does not cover"""
        m = self.module = module
        self.encoder1 = _Conv(m.encoder1)
        self.encoder2, self.encoder3, self.encoder4 = ([_Block(b) for b in seq] for seq in (m.encoder2, m.encoder3, m.encoder4))
        self.decoder4_1, self.decoder3_1, self.decoder2_1, self.decoder1_1 = (_Conv(b) for b in (m.decoder4_1, m.decoder3_1, m.decoder2_1, m.decoder1_1))
        self.decoder3_2, self.decoder2_2, self.decoder1_2 = ([_Conv(b) for b in seq] for seq in (m.decoder3_2, m.decoder2_2, m.decoder1_2))
        self.out_proj = _Conv(m.out_proj)
        for c in (self.decoder4_1, self.decoder3_1, self.decoder2_1, self.decoder1_1, self.out_proj):
            if c.norm is not None:
                raise NotImplementedError(_WHO + "a normalised lateral / output projection has no device form")

    @staticmethod
    def _seq(layers, x, size):
        for layer in layers:
            x, size = layer(x, size)
        return x, size

    @staticmethod
    def _seq_grad(layers, x, size):
        for layer in layers:
            x, size = layer.grad(x, size)
        return x, size

    def _forward_rows_grad(self, x, dino_feat):
        """forward_rows with the autograd graph recorded: the same kernels in the same order, so the same numbers"""
        _, Cin, H, W = x.shape
        xr = x.float()
        xr = xr.reshape(H * W, 1) if Cin == 1 else xr[0].permute(1, 2, 0).reshape(H * W, Cin).contiguous()
        dino = dino_feat.float().reshape(-1, dino_feat.shape[3]).contiguous()
        dsz = tuple(dino_feat.shape[1:3])
        s1, z1 = self.encoder1.grad(xr.contiguous(), (H, W))
        s2, z2 = self._seq_grad(self.encoder2, s1, z1)
        s3, z3 = self._seq_grad(self.encoder3, s2, z2)
        s4, z4 = self._seq_grad(self.encoder4, s3, z3)
        if dino.shape[1] != s4.shape[1]:
            raise ValueError(_WHO + "dino_feat has %d channels, the stage-4 map %d" % (dino.shape[1], s4.shape[1]))
        l4, _ = self.decoder4_1.grad(_ResizeRows.apply(dino, s4, dsz, z4), z4)
        l3, _ = self.decoder3_1.grad(s3, z3)
        l3, _ = self._seq_grad(self.decoder3_2, _ResizeRows.apply(l4, l3, z4, z3), z3)
        l2, _ = self.decoder2_1.grad(s2, z2)
        l2, _ = self._seq_grad(self.decoder2_2, _ResizeRows.apply(l3, l2, z3, z2), z2)
        l1, _ = self.decoder1_1.grad(s1, z1, addend=l2)
        l1, _ = self._seq_grad(self.decoder1_2, _ResizeRows.apply(l1, None, z1, (H, W)), (H, W))
        l1, _ = self.out_proj.grad(l1, (H, W))
        return [l1, l2, l3, l4], [(H, W), z2, z3, z4]

    def forward_rows(self, x, dino_feat):
        """x [1, Cin, H, W], dino_feat [1, h, w, C4] -> ([out_proj rows, latent_s2, latent_s3, latent_s4] as [H_i W_i, C_i] float32, [(H_i, W_i)]);
        with gradients enabled the autograd graph is recorded (see the module docstring)"""
        if x.dim() != 4 or x.shape[0] != 1 or dino_feat.dim() != 4 or dino_feat.shape[0] != 1:
            raise ValueError(_WHO + "one image per call: x [1, C, H, W], dino_feat [1, h, w, C] (got %s, %s)" % (tuple(x.shape), tuple(dino_feat.shape)))
        if torch.is_grad_enabled():
            return self._forward_rows_grad(x, dino_feat)
        _, Cin, H, W = x.shape
        xr = x.detach().float()
        xr = xr.reshape(H * W, 1) if Cin == 1 else xr[0].permute(1, 2, 0).reshape(H * W, Cin).contiguous()
        dino = dino_feat.detach().float().reshape(-1, dino_feat.shape[3]).contiguous()
        # encoder (:258-261)
        s1, z1 = self.encoder1(xr.contiguous(), (H, W))
        s2, z2 = self._seq(self.encoder2, s1, z1)
        s3, z3 = self._seq(self.encoder3, s2, z2)
        s4, z4 = self._seq(self.encoder4, s3, z3)
        if dino.shape[1] != s4.shape[1]:
            raise ValueError(_WHO + "dino_feat has %d channels, the stage-4 map %d" % (dino.shape[1], s4.shape[1]))
        # decoder (:263-285); every sum is the addend of the kernel that produces its other operand
        l4, _ = self.decoder4_1(lib.resize_rows(dino, dino_feat.shape[1:3], z4, addend=s4), z4)                 # feats_s4 + interp_dino
        l3, _ = self.decoder3_1(s3, z3)
        l3, _ = self._seq(self.decoder3_2, lib.resize_rows(l4, z4, z3, addend=l3), z3)                            # latent_s3 + interp_s3
        l2, _ = self.decoder2_1(s2, z2)
        l2, _ = self._seq(self.decoder2_2, lib.resize_rows(l3, z3, z2, addend=l2), z2)                            # latent_s2 + interp_s2
        l1, _ = self.decoder1_1(s1, z1, addend=l2)                                                                # decoder1_1(feats_s1) + latent_s2
        l1, _ = self._seq(self.decoder1_2, lib.resize_rows(l1, z1, (H, W)), (H, W))
        l1, _ = self.out_proj(l1, (H, W))
        return [l1, l2, l3, l4], [(H, W), z2, z3, z4]

    def forward(self, x, dino_feat=None):
        """the reference's return value: [latent_s1 [1, Cout, H, W], latent_s2, latent_s3, latent_s4], contiguous NCHW"""
        rows, sizes = self.forward_rows(x, dino_feat)
        return [r.view(h, w, r.shape[1]).permute(2, 0, 1).contiguous()[None] for r, (h, w) in zip(rows, sizes)]


def bind(module, grad=False):
    """re-bind module.forward ON THE INSTANCE to the device path.  grad=False: in training mode or with gradients enabled the call goes to the
    module's own forward unchanged.  grad=True: the device path runs there too and records its backward.  Returns the DeviceImageBackbone;
    `del module.__dict__["forward"]` (overlay2d3d's remove()) restores the original."""
    dev = DeviceImageBackbone(module)
    orig = module.forward

    def forward(x, dino_feat=None):
        if not grad and (module.training or torch.is_grad_enabled()):
            return orig(x, dino_feat)
        return dev.forward(x, dino_feat)
    module.forward = forward
    return dev
