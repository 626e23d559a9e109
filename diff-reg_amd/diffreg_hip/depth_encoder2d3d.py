"""Depth-Anything's float32 ViT-L/14 encoder on the device, in exact fp32 products (csrc/vit_f32.hip).

`DPT_DINOv2.forward` (depth_anything/dpt.py:155-166, reached through predict_depth at EXP/model.py:339-345, eval mode under torch.no_grad()) runs
`self.pretrained.get_intermediate_layers(x, 4, return_class_token=True)` on a float32 `DinoVisionTransformer`
(torchhub/facebookresearch_dinov2_main/vision_transformer.py, built by hubconf._make_dinov2_model: NestedTensorBlock, block_chunks=0,
init_values=1.0, ffn_layer="mlp", no register tokens).  DeviceViTF32 reads such a module BY ATTRIBUTE (nothing of the reference is imported):

    patch_embed.proj, cls_token, pos_embed, blocks[i].{norm1, attn.qkv, attn.proj, ls1, norm2, mlp.fc1, mlp.fc2, ls2}, norm, num_heads, patch_size

and runs dr_vit_forward_f32: float32 GEMM operands on the f32-input MFMA, fp32 accumulation, the float32 attention of dr_attention_f32 on the
packed qkv rows, a float32 residual stream.  It refuses at bind time (NotImplementedError) what diffreg_hip.vit2d3d.DeviceViT refuses -- a SwiGLU or
identity FFN, an activation other than exact nn.GELU, a head dim other than 64, a patch_embed.norm, dropout -- and a module that is not entirely
torch.float32 or that has register tokens.  The kernels read the module's own weight matrices in place (no packed image); only the patch embedding's flattened weight is copied, padded
to a multiple of 32 columns, and re-made when the parameter's `_version` or storage changes.  The position rows of an image size
come from the module's own `interpolate_pos_encoding`, called once per size and cached.

    dev = DeviceViTF32(depth_model.pretrained)          # or bind(depth_model) / overlay2d3d.accelerate(model, depth_encoder=True)
    feats = dev.get_intermediate_layers(x, 4, return_class_token=True)
"""
import ctypes

import torch
import torch.nn as nn

from . import lib
from .vit2d3d import _flat_blocks, _no_dropout

MODES = dict(colscale=0, gelu=1, scale_resid=2, addend=3)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- the C entries on tensors -----------------------------------------------------------------------------------------------------------------
def gemm_rows_f32_raw(a, M, K, N, lda, w, ldw, out, ldo, mode, bias=None, colscale=1.0, colscale_cols=0, gamma=None, addend=None, ld_addend=0):
    """dr_gemm_rows_f32 on raw geometry; returns the status code (the tests of the refusals read it)"""
    lib.ensure_init()
    args = lib.GemmRowsF32Args(_p(a), _p(w), _p(bias), _p(gamma), _p(addend), _p(out), M, K, N, lda, ldw, ldo, ld_addend, MODES[mode], colscale_cols,
                               colscale)
    return lib.raw().dr_gemm_rows_f32(ctypes.byref(args), lib.stream_of(a))


def gemm_rows_f32(a, w, mode, out=None, bias=None, colscale=1.0, colscale_cols=0, gamma=None, addend=None):
    """out = a w^T (+ bias) with the epilogue `mode` ("colscale", "gelu", "scale_resid" into `out` in place, "addend")   (dr_gemm_rows_f32)"""
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    lib.check(gemm_rows_f32_raw(a, M, K, N, a.stride(0), w, w.stride(0), out, out.stride(0), mode, bias, colscale, colscale_cols, gamma, addend,
                                addend.stride(0) if addend is not None else 0))
    return out


def patch_rows_f32(img, p, out=None):
    """[3, H, W] float32 image -> float32 patch rows [(H / p)(W / p), round_up(3 p p, 32)], pad columns zero   (dr_patch_rows_f32)"""
    lib.ensure_init()
    _, H, W = img.shape
    Kp = (3 * p * p + 31) // 32 * 32
    if out is None:
        out = torch.empty((H // p) * (W // p), Kp, dtype=torch.float32, device=img.device)
    lib.check(lib.raw().dr_patch_rows_f32(H, W, p, lib.ptr(img), _p(out), out.stride(0), lib.stream_of(img)))
    return out


def attention_rows_f32(qkv, H, out=None):
    """softmax(q k^T) v over packed qkv rows [L, 3 H d] float32 (q already scaled) -> [L, H d]: dr_attention_f32 with q, k, v at column offsets
    0, H d, 2 H d of one buffer and its leading dimension"""
    lib.ensure_init()
    L, d = qkv.shape[0], qkv.shape[1] // (3 * H)
    if out is None:
        out = torch.empty(L, qkv.stride(0), dtype=torch.float32, device=qkv.device)      # (the entry has ONE leading dimension, out's included)
    es = qkv.element_size()
    q, k, v = (ctypes.c_void_p(qkv.data_ptr() + i * H * d * es) for i in range(3))
    lib.check(lib.raw().dr_attention_f32(1, H, L, L, d, q, k, v, qkv.stride(0), None, None, 1.0, _p(out), lib.stream_of(qkv)))
    return out[:, :H * d]


def vit_workspace_bytes_f32(H, W, p, D, Dh):
    return lib.raw().dr_vit_workspace_bytes_f32(H, W, p, D, Dh)


# ---- the module ---------------------------------------------------------------------------------------------------------------------------------
def _refuse(why):
    raise NotImplementedError("libdiffreg_hip: DeviceViTF32 has no device form for " + why)


class DeviceViTF32:
    def __init__(self, module):
        self.module = module
        self.blocks = _flat_blocks(module.blocks)
        pe = module.patch_embed
        if not isinstance(getattr(pe, "norm", nn.Identity()), nn.Identity):
            _refuse("a patch_embed.norm")
        ps = module.patch_size if isinstance(module.patch_size, int) else module.patch_size[0]
        if tuple(pe.proj.kernel_size) != (ps, ps) or tuple(pe.proj.stride) != (ps, ps) or pe.proj.in_channels != 3:
            _refuse("a patch embedding other than Conv2d(3, D, p, stride p)")
        if getattr(module, "num_register_tokens", 0) != 0 or getattr(module, "register_tokens", None) is not None:
            _refuse("register tokens (num_register_tokens = %r)" % getattr(module, "num_register_tokens", None))
        self.p = ps
        self.D = D = module.cls_token.shape[-1]
        self.heads = module.num_heads
        if D % 32:
            _refuse("an embedding width that is no multiple of 32 (%d)" % D)
        if D % self.heads or D // self.heads != 64:
            _refuse("a head dim other than 64 (D = %d, heads = %d)" % (D, self.heads))
        if not self.blocks:
            _refuse("an encoder without blocks")
        self.Dh = None
        for i, b in enumerate(self.blocks):
            mlp = b.mlp
            if isinstance(mlp, nn.Identity) or not (hasattr(mlp, "fc1") and hasattr(mlp, "fc2") and hasattr(mlp, "act")):
                _refuse("an FFN other than fc1 / GELU / fc2 (block %d: %s)" % (i, type(mlp).__name__))
            if not isinstance(mlp.act, nn.GELU) or getattr(mlp.act, "approximate", "none") != "none":
                _refuse("an activation other than exact nn.GELU (block %d)" % i)
            if b.attn.num_heads != self.heads or b.attn.qkv.out_features != 3 * D or b.attn.proj.out_features != D:
                _refuse("an attention geometry that differs from the encoder's (block %d)" % i)
            for ls in (b.ls1, b.ls2):
                if not isinstance(ls, nn.Identity) and not hasattr(ls, "gamma"):
                    _refuse("a LayerScale without gamma (block %d)" % i)
            dh = mlp.fc1.out_features
            if dh % 32 or mlp.fc2.in_features != dh or (self.Dh is not None and dh != self.Dh):
                _refuse("this hidden width (block %d: %d)" % (i, dh))
            self.Dh = dh
            if b.norm1.eps != module.norm.eps or b.norm2.eps != module.norm.eps:
                _refuse("different LayerNorm eps values")
            _no_dropout(b, "block %d" % i)
            if getattr(b, "sample_drop_ratio", 0.0):
                _refuse("stochastic depth (block %d)" % i)
        self.eps = float(module.norm.eps)
        for prm in module.parameters():
            if prm.dtype != torch.float32:
                _refuse("a module that is not entirely torch.float32 (the fp16 use of this class is diffreg_hip.vit2d3d.DeviceViT)")
        self._cache = {}
        self._pos = {}
        self._blocks_c = None

    # ---- weights: the module's own matrices, copied once, refreshed when a parameter's version or storage changes
    def _cached(self, name, prm, make):
        key = (prm._version, prm.data_ptr(), prm.device, tuple(prm.shape))
        hit = self._cache.get(name)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                hit = (key, make(prm.detach()))
            self._cache[name] = hit
            self._blocks_c = None
        return hit[1]

    @staticmethod
    def _view(t):
        """the parameter's own storage where the kernels can read it (contiguous, 16-byte aligned), else a copy"""
        t = t.contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()

    def _w(self, name, lin):
        return self._cached(name, lin.weight, lambda w: self._view(w.reshape(w.shape[0], -1)))

    def _f(self, name, prm):
        return None if prm is None else self._cached(name, prm, lambda v: self._view(v.reshape(-1)))

    def _patch_w(self, w):
        flat = w.reshape(w.shape[0], -1)
        Kp = (flat.shape[1] + 31) // 32 * 32
        return torch.nn.functional.pad(flat, (0, Kp - flat.shape[1])).contiguous()

    def _weights(self):
        m = self.module
        W = dict(patch_w=self._cached("patch.w", m.patch_embed.proj.weight, self._patch_w), patch_b=self._f("patch.b", m.patch_embed.proj.bias),
                 cls=self._f("cls", m.cls_token), norm_g=self._f("norm.g", m.norm.weight), norm_b=self._f("norm.b", m.norm.bias))
        rows = []
        for i, b in enumerate(self.blocks):
            n = "b%d." % i
            rows.append([self._f(n + "n1g", b.norm1.weight), self._f(n + "n1b", b.norm1.bias), self._w(n + "qkv", b.attn.qkv),
                         self._f(n + "qkvb", b.attn.qkv.bias), self._w(n + "proj", b.attn.proj), self._f(n + "projb", b.attn.proj.bias),
                         self._f(n + "ls1", getattr(b.ls1, "gamma", None)), self._f(n + "n2g", b.norm2.weight), self._f(n + "n2b", b.norm2.bias),
                         self._w(n + "fc1", b.mlp.fc1), self._f(n + "fc1b", b.mlp.fc1.bias), self._w(n + "fc2", b.mlp.fc2),
                         self._f(n + "fc2b", b.mlp.fc2.bias), self._f(n + "ls2", getattr(b.ls2, "gamma", None))])
        if self._blocks_c is None:
            arr = (lib.VitBlockF32 * len(rows))()
            for i, r in enumerate(rows):
                arr[i] = lib.VitBlockF32(*[None if t is None else t.data_ptr() for t in r])
            self._blocks_c = arr
        return W

    def _pos_rows(self, H, W):
        m = self.module
        pe = m.pos_embed
        key = (H, W, pe._version, pe.data_ptr(), pe.device)
        hit = self._pos.get((H, W))
        if hit is None or hit[0] != key:
            L = 1 + (H // self.p) * (W // self.p)
            with torch.no_grad():
                rows = m.interpolate_pos_encoding(torch.empty(1, L, self.D, dtype=pe.dtype, device=pe.device), H, W)
            hit = (key, rows.detach().reshape(L, self.D).float().contiguous().clone())
            self._pos[(H, W)] = hit
        return hit[1]

    # ---- one image
    def _run(self, img, take=(), norm=True, workspace=None):
        """img [3, H, W] float32 -> (x_prenorm [L, D], x_norm [L, D], [the stream after block i (through the final norm if `norm`) for i in take])"""
        _, H, Wd = img.shape
        if H % self.p or Wd % self.p:
            raise AssertionError("Input image size %d x %d is not a multiple of the patch size %d" % (H, Wd, self.p))
        lib.ensure_init()
        img = img.to(torch.float32).contiguous()
        Wt = self._weights()
        pos = self._pos_rows(H, Wd)
        L, D, dev = pos.shape[0], self.D, img.device
        wsb = vit_workspace_bytes_f32(H, Wd, self.p, D, self.Dh)
        if wsb == 0:
            raise NotImplementedError("libdiffreg_hip: dr_vit_forward_f32 does not take this geometry")
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if workspace is None else workspace
        x_pre = torch.empty(L, D, dtype=torch.float32, device=dev)
        x_norm = torch.empty(L, D, dtype=torch.float32, device=dev)
        outs = [torch.empty(L, D, dtype=torch.float32, device=dev) for _ in take]
        take_c = (ctypes.c_int * max(len(take), 1))(*take)
        out_c = (ctypes.c_void_p * max(len(take), 1))(*[o.data_ptr() for o in outs])
        cfg = lib.VitConfigF32(H, Wd, self.p, D, self.heads, self.Dh, len(self.blocks), self.eps, img.data_ptr(), _p(Wt["patch_w"]),
                               _p(Wt["patch_b"]), _p(Wt["cls"]), _p(pos), self._blocks_c, _p(Wt["norm_g"]), _p(Wt["norm_b"]), _p(x_pre), _p(x_norm),
                               len(take), 1 if norm else 0, take_c, out_c, _p(ws), ws.numel())
        lib.check(lib.raw().dr_vit_forward_f32(ctypes.byref(cfg), lib.stream_of(img)))
        return x_pre, x_norm, outs

    # ---- the reference's interface (vision_transformer.py:253-269, :297-321)
    def forward_features(self, x, masks=None):
        if masks is not None:
            raise NotImplementedError("libdiffreg_hip: DeviceViTF32.forward_features takes no masks")
        if isinstance(x, (list, tuple)):
            raise NotImplementedError("libdiffreg_hip: DeviceViTF32.forward_features takes one batch tensor, not a list")
        pre, nrm = [], []
        for b in range(x.shape[0]):                  # B > 1 loops over the images
            xp, xn, _ = self._run(x[b])
            pre.append(xp)
            nrm.append(xn)
        x_norm, x_pre = torch.stack(nrm), torch.stack(pre)
        return {"x_norm_clstoken": x_norm[:, 0], "x_norm_regtokens": x_norm[:, 1:1], "x_norm_patchtokens": x_norm[:, 1:], "x_prenorm": x_pre,
                "masks": masks}

    def get_intermediate_layers(self, x, n=1, reshape=False, return_class_token=False, norm=True):
        depth = len(self.blocks)
        take = list(range(depth - n, depth)) if isinstance(n, int) else list(n)
        if any(i < 0 or i >= depth for i in take):
            raise AssertionError("only %d blocks" % depth)
        per_layer = [[] for _ in take]
        for b in range(x.shape[0]):
            _, _, outs = self._run(x[b], take, norm)          # the entry writes the final norm of each taken stream itself
            for k, o in enumerate(outs):
                per_layer[k].append(o)
        outputs = [torch.stack(rows) for rows in per_layer]
        class_tokens = [o[:, 0] for o in outputs]
        outputs = [o[:, 1:] for o in outputs]
        if reshape:
            B, _, h, w = x.shape
            outputs = [o.reshape(B, h // self.p, w // self.p, -1).permute(0, 3, 1, 2).contiguous() for o in outputs]
        if return_class_token:
            return tuple(zip(outputs, class_tokens))
        return tuple(outputs)


def bind(depth_model):
    """re-bind depth_model.pretrained.get_intermediate_layers ON THE INSTANCE (depth_anything/dpt.py:158): the device path in eval mode under
    torch.no_grad() with a CUDA float32 batch, the module's own method unchanged otherwise.  Refuses (NotImplementedError) before anything is
    bound.  Returns the undo; the DeviceViTF32 is its `.device`."""
    vit = depth_model.pretrained
    dev = DeviceViTF32(vit)
    orig = vit.get_intermediate_layers

    def get_intermediate_layers(x, n=1, reshape=False, return_class_token=False, norm=True):
        if vit.training or torch.is_grad_enabled() or not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            return orig(x, n, reshape=reshape, return_class_token=return_class_token, norm=norm)
        return dev.get_intermediate_layers(x, n, reshape=reshape, return_class_token=return_class_token, norm=norm)
    vit.get_intermediate_layers = get_intermediate_layers

    def undo():
        vit.__dict__.pop("get_intermediate_layers", None)
    undo.device = dev
    return undo
