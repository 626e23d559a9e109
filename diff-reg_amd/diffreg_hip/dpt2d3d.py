"""The decoder of Depth-Anything on the device: DPTHead.forward (depth_anything/dpt.py:103-136; ResidualConvUnit and FeatureFusionBlock,
depth_anything/blocks.py:37-153), called once per forward of the 2D-3D model through EXP/model.py:343-351, composed from the seventh set's three
entries and dr_resize_rows_f32 (csrc/conv2d.hip).  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.

    head = DeviceDPTHead(model.depth_model.depth_head)     # reads the module by attribute: kernel sizes, strides, channel counts, activations
    depth = head.forward(out_features, patch_h, patch_w)   # the reference's [1, 1, 14 patch_h, 14 patch_w]
    rows, named = head.forward_rows(out_features, patch_h, patch_w)

Inside, every activation is token rows [H W, C] float32 (NHWC), so the ViT's [1, L, C] tokens ARE the rows of the 1 x 1 projections: the
permute + reshape of dpt.py:113 moves nothing.  The launches, in order: the four projections (k = 1), the two transposed convolutions
(kernel = stride = 4 and 2: one GEMM with a pixel-shuffle store each), the stride-2 convolution, the four layerN_rn, the four fusion blocks --
per ResidualConvUnit two launches (conv1 with ReLU on its input and on its output, conv2 with the unit's raw input as addend and, for
resConfUnit1, xs[0] as the second addend: blocks.py:92 and :136 ride on the store), then dr_resize_rows_f32 for F.interpolate(align_corners=True)
and the 1 x 1 out_conv -- output_conv1, the resample to 14 patch_h x 14 patch_w, and ONE launch for the tail conv 3 x 3 -> ReLU -> conv 1 x 1 ->
ReLU (the 32-channel hidden map is never written).  refinenet4 has one input, so only its resConfUnit2 runs; refinenet1 resamples by the scale
factor 2, the others to the next layer's size.

Weights are packed once per convolution and re-packed when the parameter's `_version` or storage changes.  Workspaces come from torch's
allocator; nothing is read back to the host, so the call can be captured into a graph.  Anything without a device form -- use_clstoken,
nclass > 1, batch norm, expand, deconv, groups != 1, an activation other than a not-in-place nn.ReLU inside the units, a reassemble layer that is
not one of the four forms, channel counts outside the kernels' domain, parameters that are not float32 -- raises NotImplementedError when the
module is bound, never at call time.

bind(head) / overlay2d3d.accelerate(depth_head=True): the device path runs in eval mode under torch.no_grad() with CUDA float32 inputs of batch 1;
otherwise the bound forward calls the module's own code unchanged.
"""
import torch
import torch.nn as nn

from . import lib

_WHO = "DPT head on the device: "
NAMES = ("layer_1", "layer_2", "layer_3", "layer_4", "path_4", "path_3", "path_2", "path_1", "output_conv1", "out")


def _no(msg):
    return NotImplementedError(_WHO + msg)


def _one(v, what):
    if isinstance(v, (tuple, list)):
        if len(set(int(a) for a in v)) != 1:
            raise _no("%s %s is not square" % (what, tuple(v)))
        return int(v[0])
    return int(v)


def _check_params(mod, what):
    for name in ("weight", "bias"):
        p = getattr(mod, name, None)
        if p is not None and p.dtype != torch.float32:
            raise _no("%s.%s is %s, the kernels are float32" % (what, name, p.dtype))


class _Packed:
    """a parameter's packed image, rebuilt when the parameter's `_version` or storage changes"""

    def __init__(self, param, pack):
        self.param, self.pack, self._key, self._image = param, pack, None, None

    def __call__(self):
        w = self.param
        key = (w._version, w.data_ptr(), w.device, tuple(w.shape))
        if key != self._key:
            self._image, self._key = self.pack(w), key
        return self._image


class _Conv:
    """one nn.Conv2d of the head on the MFMA arm of dr_conv2d_rows_act_f32"""

    def __init__(self, conv, what):
        if not isinstance(conv, nn.Conv2d):
            raise _no("%s is %s, not a Conv2d" % (what, type(conv).__name__))
        if conv.groups != 1:
            raise _no("%s: groups = %d has no device form" % (what, conv.groups))
        if conv.padding_mode != "zeros" or isinstance(conv.padding, str):
            raise _no("%s: padding %r / %r has no device form" % (what, conv.padding_mode, conv.padding))
        _check_params(conv, what)
        self.conv = conv
        self.k = _one(conv.kernel_size, what + " kernel")
        self.stride, self.padding, self.dilation = (_one(v, what) for v in (conv.stride, conv.padding, conv.dilation))
        self.cin, self.cout = conv.in_channels, conv.out_channels
        if self.cin % 4 != 0 or self.cin > (1 << 16) or self.cout > (1 << 16) or self.k * self.k * self.cin > (1 << 20) or self.k > 31:
            raise _no("%s: %d -> %d channels, k = %d is outside the kernels' domain (Cin %% 4 == 0)" % (what, self.cin, self.cout, self.k))
        self.weight = _Packed(conv.weight, lib.pack_conv_weight)

    def bias(self):
        b = self.conv.bias
        return None if b is None else b.detach()

    def __call__(self, x, size, relu_in=False, relu_out=False, addend=None, addend2=None):
        return lib.conv2d_rows_act(x, size, self.weight(), self.k, self.bias(), self.stride, self.padding, self.dilation, relu_in, relu_out, addend,
                                   addend2)


class _ConvT:
    """nn.ConvTranspose2d with kernel = stride (dr_conv_transpose2d_rows_f32)"""

    def __init__(self, conv, what):
        _check_params(conv, what)
        k, s = _one(conv.kernel_size, what + " kernel"), _one(conv.stride, what + " stride")
        if k != s or _one(conv.padding, what) != 0 or _one(conv.output_padding, what) != 0 or _one(conv.dilation, what) != 1 or conv.groups != 1:
            raise _no("%s: a transposed convolution other than kernel = stride, padding 0, dilation 1, groups 1 has no device form" % what)
        self.conv, self.s, self.cin, self.cout = conv, s, conv.in_channels, conv.out_channels
        if s > 8 or self.cin % 4 != 0 or self.cin > (1 << 16) or s * s * self.cout > (1 << 16):
            raise _no("%s: %d -> %d channels, stride %d is outside the kernels' domain" % (what, self.cin, self.cout, s))
        self.weight = _Packed(conv.weight, lib.pack_conv_transpose_weight)

    def __call__(self, x, size):
        b = self.conv.bias
        return lib.conv_transpose2d_rows(x, size, self.weight(), self.s, None if b is None else b.detach())


def _relu(act, what, inplace_ok):
    if not isinstance(act, nn.ReLU):
        raise _no("%s: activation %s has no device form" % (what, type(act).__name__))
    if act.inplace and not inplace_ok:
        raise _no("%s: an in-place ReLU changes the residual the unit adds; only nn.ReLU(False) has a device form" % what)


class _Unit:
    """ResidualConvUnit (blocks.py:69-92): conv2(relu(conv1(relu(x)))) + x, the residual (and a fusion block's xs[0]) on conv2's store"""

    def __init__(self, unit, what):
        if getattr(unit, "bn", False):
            raise _no("%s: batch norm has no device form" % what)
        if getattr(unit, "groups", 1) != 1:
            raise _no("%s: groups = %d has no device form" % (what, unit.groups))
        _relu(unit.activation, what, inplace_ok=False)
        self.conv1, self.conv2 = _Conv(unit.conv1, what + ".conv1"), _Conv(unit.conv2, what + ".conv2")

    def __call__(self, x, size, extra=None):
        h, _ = self.conv1(x, size, relu_in=True, relu_out=True)
        y, _ = self.conv2(h, size, addend=x, addend2=extra)
        return y


class _Fusion:
    """FeatureFusionBlock (blocks.py:126-153)"""

    def __init__(self, blk, what):
        if getattr(blk, "deconv", False) or getattr(blk, "expand", False):
            raise _no("%s: deconv / expand have no device form" % what)
        if getattr(blk, "groups", 1) != 1:
            raise _no("%s: groups = %d has no device form" % (what, blk.groups))
        if not getattr(blk, "align_corners", True):
            raise _no("%s: align_corners=False has no device form" % what)
        self.size = None if getattr(blk, "size", None) is None else tuple(int(v) for v in blk.size)
        self.unit1, self.unit2 = _Unit(blk.resConfUnit1, what + ".resConfUnit1"), _Unit(blk.resConfUnit2, what + ".resConfUnit2")
        self.out_conv = _Conv(blk.out_conv, what + ".out_conv")

    def __call__(self, x0, size, x1=None, to=None):
        out = x0 if x1 is None else self.unit1(x1, size, extra=x0)           # xs[0] + resConfUnit1(xs[1])
        out = self.unit2(out, size)
        dst = to if to is not None else (self.size if self.size is not None else (2 * size[0], 2 * size[1]))
        out = lib.resize_rows(out, size, dst)
        return self.out_conv(out, dst)[0], tuple(dst)


class DeviceDPTHead:
    def __init__(self, head):
        """binds every layer of `head` (the reference's DPTHead, or any module with its attribute names); NotImplementedError for anything the
        device path does not cover"""
        self.module = head
        if getattr(head, "use_clstoken", False):
            raise _no("use_clstoken=True (the readout projections) has no device form")
        if int(getattr(head, "nclass", 1)) > 1:
            raise _no("nclass > 1 (the segmentation tail) has no device form")
        if len(head.projects) != 4 or len(head.resize_layers) != 4:
            raise _no("the head takes four feature levels")
        self.projects = [_Conv(c, "projects[%d]" % i) for i, c in enumerate(head.projects)]
        self.resize = []
        for i, layer in enumerate(head.resize_layers):
            what = "resize_layers[%d]" % i
            if isinstance(layer, nn.Identity):
                self.resize.append(None)
            elif isinstance(layer, nn.ConvTranspose2d):
                self.resize.append(_ConvT(layer, what))
            elif isinstance(layer, nn.Conv2d):
                self.resize.append(_Conv(layer, what))
            else:
                raise _no("%s is %s: not a transposed convolution with kernel = stride, an identity or a convolution" % (what, type(layer).__name__))
        sc = head.scratch
        if getattr(sc, "stem_transpose", None) is not None:
            raise _no("scratch.stem_transpose has no device form")
        self.rn = [_Conv(getattr(sc, "layer%d_rn" % i), "scratch.layer%d_rn" % i) for i in (1, 2, 3, 4)]
        self.fusion = {i: _Fusion(getattr(sc, "refinenet%d" % i), "scratch.refinenet%d" % i) for i in (1, 2, 3, 4)}
        if not hasattr(sc, "output_conv1") or not hasattr(sc, "output_conv2"):
            raise _no("the head has no output_conv1 / output_conv2 (the nclass > 1 tail has no device form)")
        self.output_conv1 = _Conv(sc.output_conv1, "scratch.output_conv1")
        tail = [m for m in sc.output_conv2 if not isinstance(m, nn.Identity)]
        if len(tail) != 4:
            raise _no("scratch.output_conv2 is not conv, ReLU, conv, ReLU")
        self.tail1, self.tail2 = _Conv(tail[0], "scratch.output_conv2[0]"), _Conv(tail[2], "scratch.output_conv2[2]")
        _relu(tail[1], "scratch.output_conv2[1]", inplace_ok=True)
        _relu(tail[3], "scratch.output_conv2[3]", inplace_ok=True)
        t2 = self.tail2
        if self.tail1.cout > 64 or t2.k != 1 or t2.cout != 1 or t2.stride != 1 or t2.padding != 0 or t2.cin != self.tail1.cout:
            raise _no("scratch.output_conv2: the tail must be conv to <= 64 channels, ReLU, 1 x 1 conv to one channel, ReLU")
        self.tail_w2 = _Packed(t2.conv.weight, lambda w: w.detach().float().reshape(-1).contiguous())

    def forward_rows(self, out_features, patch_h, patch_w):
        """out_features: what get_intermediate_layers(x, 4, return_class_token=True) returns, four (tokens [1, L, C], class token) pairs.
        -> (depth rows [14 patch_h * 14 patch_w], {name: (rows [H W, C], (H, W))} for NAMES)"""
        ph, pw = int(patch_h), int(patch_w)
        if len(out_features) != 4:
            raise ValueError(_WHO + "four feature levels, got %d" % len(out_features))
        named, layers = {}, []
        for i, feat in enumerate(out_features):
            x = feat[0]
            if x.dim() != 3 or x.shape[0] != 1 or x.shape[1] != ph * pw or x.dtype != torch.float32:
                raise ValueError(_WHO + "level %d: tokens %s %s are not float32 [1, %d, C]" % (i, tuple(x.shape), x.dtype, ph * pw))
            y, size = self.projects[i](x.detach()[0].contiguous(), (ph, pw))
            if self.resize[i] is not None:
                y, size = self.resize[i](y, size)
            layers.append((y, size))
            named["layer_%d" % (i + 1)] = (y, size)
        rn = [(self.rn[i](y, size)[0], size) for i, (y, size) in enumerate(layers)]
        p4, z = self.fusion[4](rn[3][0], rn[3][1], to=rn[2][1])
        named["path_4"] = (p4, z)
        p3, z = self.fusion[3](p4, z, rn[2][0], to=rn[1][1])
        named["path_3"] = (p3, z)
        p2, z = self.fusion[2](p3, z, rn[1][0], to=rn[0][1])
        named["path_2"] = (p2, z)
        p1, z = self.fusion[1](p2, z, rn[0][0])
        named["path_1"] = (p1, z)
        oc1, _ = self.output_conv1(p1, z)
        named["output_conv1"] = (oc1, z)
        dst = (14 * ph, 14 * pw)
        up = lib.resize_rows(oc1, z, dst)
        t1, t2 = self.tail1, self.tail2
        depth, dz = lib.conv2d_rows_project(up, dst, t1.weight(), t1.k, t1.bias(), self.tail_w2(), t2.bias(), t1.stride, t1.padding, t1.dilation,
                                            relu_out=True)
        named["out"] = (depth.view(-1, 1), dz)
        return depth, named

    def forward(self, out_features, patch_h, patch_w):
        """the reference's return value: [1, 1, 14 patch_h, 14 patch_w]"""
        depth, named = self.forward_rows(out_features, patch_h, patch_w)
        h, w = named["out"][1]
        return depth.view(1, 1, h, w)


def _device_inputs(out_features):
    try:
        return all(f[0].is_cuda and f[0].dtype == torch.float32 and f[0].dim() == 3 and f[0].shape[0] == 1 for f in out_features)
    except (AttributeError, IndexError, TypeError):
        return False


def bind(head):
    """re-bind head.forward ON THE INSTANCE: the device path in eval mode under torch.no_grad() with CUDA float32 inputs of batch 1, the module's own
    forward unchanged otherwise.  Refuses (NotImplementedError) before anything is bound.  Returns the undo; the DeviceDPTHead is its `.device`."""
    dev = DeviceDPTHead(head)
    orig = head.forward

    def forward(out_features, patch_h, patch_w):
        if head.training or torch.is_grad_enabled() or not _device_inputs(out_features):
            return orig(out_features, patch_h, patch_w)
        return dev.forward(out_features, patch_h, patch_w)
    head.forward = forward

    def undo():
        head.__dict__.pop("forward", None)
    undo.device = dev
    return undo
