"""The frozen DINOv2 ViT encoder of the 2D-3D model on the device, in the reference's own fp16 arithmetic (csrc/vit.hip).

`CNNandDinov2(amp=True)` (EXP/encoders.py:107-119) keeps a `DinoVisionTransformer` (Diff-Reg-2d3d/transformer/dinov2.py) cast to torch.float16 and
calls its `forward_features` once per pair, in eval and in training, under torch.no_grad().  DeviceViT reads such a module BY ATTRIBUTE (nothing of
the reference is imported):

    patch_embed.proj, cls_token, pos_embed, blocks[i].{norm1, attn.qkv, attn.proj, ls1, norm2, mlp.fc1, mlp.fc2, ls2}, norm, num_heads, patch_size

(`BlockChunk` lists are flattened, nn.Identity entries skipped) and runs dr_vit_forward_f16: fp16 GEMM operands with one fp16 MFMA product per MAC
and fp32 accumulation, an fp32 residual stream, fp16 flash attention.  Weights are packed once and re-packed when a parameter's `_version` or
storage changes.  A module the kernels do not cover is refused at bind time with NotImplementedError -- a SwiGLU or identity FFN, an activation other
than exact nn.GELU, a head dim other than 64, a patch_embed.norm, dropout, a module not in torch.float16 -- never at call time.

The position rows of an image size come from the module's own `interpolate_pos_encoding` (the bicubic resample with its +0.1 quirk and the square
early return, dinov2.py:166-188), called once per size and cached: set-up, not hot path.

    dev = DeviceViT(vit)                       # or bind(encoder) / overlay2d3d.accelerate(model, dino=True)
    out = dev.forward_features(x)              # the reference's dict, fp16
    feats = dev.get_intermediate_layers(x, [4, 11, 17, 23], return_class_token=True)
"""
import ctypes

import torch
import torch.nn as nn

from . import lib

_MODES = dict(f16=0, gelu_f16=1, scale_resid_f32=2, f32=3)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ---- the C entries on tensors -----------------------------------------------------------------------------------------------------------------
def pack_weight_f16(w):
    """nn.Linear weight [N, K] fp16 -> the packed image dr_gemm_rows_f16 streams (K padded to a multiple of 32)   (dr_pack_weight_f16)"""
    lib.ensure_init()
    if w.dtype != torch.float16 or w.dim() != 2 or w.stride(1) != 1:
        raise ValueError("pack_weight_f16 takes a [N, K] float16 matrix with contiguous rows")
    N, K = w.shape
    nbytes = lib.raw().dr_pack_weight_f16_bytes(N, K)
    if nbytes == 0:
        raise NotImplementedError("libdiffreg_hip: the fp16 rows GEMM takes N %% 16 == 0 (got N = %d)" % N)
    out = torch.empty(nbytes // 2, dtype=torch.float16, device=w.device)
    lib.check(lib.raw().dr_pack_weight_f16(N, K, lib.ptr(w) if w.is_contiguous() else _p(w), w.stride(0), lib.ptr(out), lib.stream_of(w)))
    return out


def gemm_rows_f16_raw(a, M, K, N, lda, w_packed, out, ldo, mode, bias=None, colscale=1.0, colscale_cols=0, gamma=None, addend=None, ld_addend=0):
    """dr_gemm_rows_f16 on raw geometry; returns the status code (the tests of the refusals read it)"""
    lib.ensure_init()
    args = lib.GemmRowsF16Args(_p(a), _p(w_packed), _p(bias), _p(gamma), _p(addend), _p(out), M, K, N, lda, ldo, ld_addend, _MODES[mode],
                               colscale_cols, colscale)
    return lib.raw().dr_gemm_rows_f16(ctypes.byref(args), lib.stream_of(a))


def gemm_rows_f16(a, w_packed, N, mode, out=None, bias=None, colscale=1.0, colscale_cols=0, gamma=None, addend=None):
    """out = a W^T (+ bias) with the epilogue `mode` ("f16", "gelu_f16", "scale_resid_f32" into `out` in place, "f32")   (dr_gemm_rows_f16)"""
    M, K = a.shape
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16 if mode in ("f16", "gelu_f16") else torch.float32, device=a.device)
    lib.check(gemm_rows_f16_raw(a, M, K, N, a.stride(0), w_packed, out, out.stride(0), mode, bias, colscale, colscale_cols, gamma, addend,
                                addend.stride(0) if addend is not None else 0))
    return out


def layernorm_rows_f16(x, gamma, beta, eps, out_f32=False, out=None):
    """nn.LayerNorm over fp32 rows [rows, C] -> fp16 (or fp32) rows   (dr_layernorm_rows_f16)"""
    lib.ensure_init()
    rows, C = x.shape
    if out is None:
        out = torch.empty(rows, C, dtype=torch.float32 if out_f32 else torch.float16, device=x.device)
    lib.check(lib.raw().dr_layernorm_rows_f16(rows, C, _p(x), x.stride(0), _p(gamma), _p(beta), eps, 1 if out_f32 else 0, _p(out), out.stride(0),
                                              lib.stream_of(x)))
    return out


def attention_rows_f16_raw(qkv, L, H, d, ld, out, ldo):
    lib.ensure_init()
    return lib.raw().dr_attention_rows_f16(L, H, d, _p(qkv), ld, _p(out), ldo, lib.stream_of(qkv))


def attention_rows_f16(qkv, H, out=None):
    """softmax(q k^T) v over packed qkv rows [L, 3 H 64] fp16 (q already scaled) -> [L, H 64] fp16   (dr_attention_rows_f16)"""
    L = qkv.shape[0]
    d = qkv.shape[1] // (3 * H)
    if out is None:
        out = torch.empty(L, H * d, dtype=torch.float16, device=qkv.device)
    lib.check(attention_rows_f16_raw(qkv, L, H, d, qkv.stride(0), out, out.stride(0)))
    return out


def patch_rows_f16(img, p, out=None):
    """[3, H, W] fp16 / fp32 image -> fp16 patch rows [(H / p)(W / p), round_up(3 p p, 32)], pad columns zero   (dr_patch_rows_f16)"""
    lib.ensure_init()
    _, H, W = img.shape
    Kp = (3 * p * p + 31) // 32 * 32
    if out is None:
        out = torch.empty((H // p) * (W // p), Kp, dtype=torch.float16, device=img.device)
    lib.check(lib.raw().dr_patch_rows_f16(H, W, p, lib.ptr(img), 1 if img.dtype == torch.float32 else 0, _p(out), out.stride(0), lib.stream_of(img)))
    return out


def vit_workspace_bytes(H, W, p, D, Dh):
    return lib.raw().dr_vit_workspace_bytes(H, W, p, D, Dh)


# ---- the module ---------------------------------------------------------------------------------------------------------------------------------
def _flat_blocks(blocks):
    out = []
    for b in blocks:
        if isinstance(b, nn.Identity):
            continue
        if hasattr(b, "norm1"):
            out.append(b)
        else:                                   # a BlockChunk: a ModuleList padded with nn.Identity in front
            out.extend(_flat_blocks(b))
    return out


def _refuse(why):
    raise NotImplementedError("libdiffreg_hip: DeviceViT has no device form for " + why)


def _no_dropout(m, where):
    for sub in m.modules():
        if isinstance(sub, nn.Dropout) and sub.p != 0.0:
            _refuse("non-zero dropout (%s)" % where)          # (names DeviceViT for either class: the text is kept as it was)


class DeviceEncoder:
    """What DeviceViT (fp16, below) and depth_encoder2d3d.DeviceViTF32 (float32) share: the bind-time walk of the module, the cache of prepared
    weights and position rows, the per-block pointer rows, one image through the C entry, and the reference's two methods on top.  A subclass states
    its dtype, how a weight is prepared, its ctypes structs and entry, and who applies the final norm to a take ("the policy")."""
    DTYPE = None                # every parameter's dtype, and what the refusal says otherwise
    DTYPE_REFUSAL = None
    X_NORM_DTYPE = None
    BLOCK_C = CONFIG_C = None   # lib's ctypes structs
    ENTRY = WORKSPACE_BYTES = None

    @classmethod
    def _refuse(cls, why):
        raise NotImplementedError("libdiffreg_hip: %s has no device form for %s" % (cls.__name__, why))

    def _refuse_module(self, module):
        """what only this precision refuses, asked right behind the patch embedding's checks"""

    def __init__(self, module):
        self.module = module
        self.blocks = _flat_blocks(module.blocks)
        _refuse = self._refuse
        pe = module.patch_embed
        if not isinstance(getattr(pe, "norm", nn.Identity()), nn.Identity):
            _refuse("a patch_embed.norm")
        ps = module.patch_size if isinstance(module.patch_size, int) else module.patch_size[0]
        if tuple(pe.proj.kernel_size) != (ps, ps) or tuple(pe.proj.stride) != (ps, ps) or pe.proj.in_channels != 3:
            _refuse("a patch embedding other than Conv2d(3, D, p, stride p)")
        self._refuse_module(module)
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
            if prm.dtype != self.DTYPE:
                _refuse(self.DTYPE_REFUSAL)
        self._cache = {}
        self._pos = {}
        self._blocks_c = None

    # ---- weights: prepared once (_matrix, _vector, _patch_w of the subclass), prepared again when a parameter's version or storage changes
    def _cached(self, name, prm, make):
        key = (prm._version, prm.data_ptr(), prm.device, tuple(prm.shape))
        hit = self._cache.get(name)
        if hit is None or hit[0] != key:
            with torch.no_grad():
                hit = (key, make(prm.detach()))
            self._cache[name] = hit
            self._blocks_c = None
        return hit[1]

    def _w(self, name, lin):
        return self._cached(name, lin.weight, self._matrix)

    def _f(self, name, prm):
        return None if prm is None else self._cached(name, prm, self._vector)

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
            arr = (self.BLOCK_C * len(rows))()
            for i, r in enumerate(rows):
                arr[i] = self.BLOCK_C(*[None if t is None else t.data_ptr() for t in r])
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
            # (a copy of its own: at the trained size the module hands back pos_embed itself)
            hit = (key, rows.detach().reshape(L, self.D).to(torch.float32, copy=True).contiguous())
            self._pos[(H, W)] = hit
        return hit[1]

    # ---- one image
    def _run(self, img, take=(), norm=False, workspace=None):
        """img [3, H, W] -> (x_prenorm fp32 [L, D], x_norm [L, D], [the fp32 stream after block i for i in take]); with `norm` (a subclass whose
        entry has norm_take) a take went through the final norm"""
        _, H, Wd = img.shape
        if H % self.p or Wd % self.p:
            raise AssertionError("Input image size %d x %d is not a multiple of the patch size %d" % (H, Wd, self.p))
        lib.ensure_init()
        img = self._image(img).contiguous()
        Wt = self._weights()
        pos = self._pos_rows(H, Wd)
        L, D, dev = pos.shape[0], self.D, img.device
        wsb = getattr(lib.raw(), self.WORKSPACE_BYTES)(H, Wd, self.p, D, self.Dh)
        if wsb == 0:
            raise NotImplementedError("libdiffreg_hip: %s does not take this geometry" % self.ENTRY)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if workspace is None else workspace
        x_pre = torch.empty(L, D, dtype=torch.float32, device=dev)
        x_norm = torch.empty(L, D, dtype=self.X_NORM_DTYPE, device=dev)
        outs = [torch.empty(L, D, dtype=torch.float32, device=dev) for _ in take]
        take_c = (ctypes.c_int * max(len(take), 1))(*take)
        out_c = (ctypes.c_void_p * max(len(take), 1))(*[o.data_ptr() for o in outs])
        cfg = self.CONFIG_C(H=H, W=Wd, p=self.p, D=D, heads=self.heads, Dh=self.Dh, depth=len(self.blocks), eps=self.eps, img=img.data_ptr(),
                            patch_w=_p(Wt["patch_w"]), patch_b=_p(Wt["patch_b"]), cls=_p(Wt["cls"]), pos=_p(pos), blocks=self._blocks_c,
                            norm_g=_p(Wt["norm_g"]), norm_b=_p(Wt["norm_b"]), x_prenorm=_p(x_pre), x_norm=_p(x_norm), n_take=len(take), take=take_c,
                            take_out=out_c, workspace=_p(ws), workspace_bytes=ws.numel(), **self._flags(img, norm))
        lib.check(getattr(lib.raw(), self.ENTRY)(ctypes.byref(cfg), lib.stream_of(img)))
        return x_pre, x_norm, outs

    # ---- the reference's interface (dinov2.py:213-237, :266-292; the hub's vision_transformer.py:253-269, :297-321)
    def forward_features(self, x, masks=None):
        if masks is not None:
            raise NotImplementedError("libdiffreg_hip: %s.forward_features takes no masks" % type(self).__name__)
        if isinstance(x, (list, tuple)):
            raise NotImplementedError("libdiffreg_hip: %s.forward_features takes one batch tensor, not a list" % type(self).__name__)
        pre, nrm = [], []
        for b in range(x.shape[0]):                  # B > 1 loops over the images
            xp, xn, _ = self._run(x[b])
            pre.append(xp.to(self.X_NORM_DTYPE))     # (x_prenorm goes out in the module's dtype: a cast per image in fp16, nothing in float32)
            nrm.append(xn)
        return self._features(torch.stack(nrm), torch.stack(pre), masks)

    def get_intermediate_layers(self, x, n=1, reshape=False, return_class_token=False, norm=True):
        depth = len(self.blocks)
        take = list(range(depth - n, depth)) if isinstance(n, int) else list(n)
        if any(i < 0 or i >= depth for i in take):
            raise AssertionError("only %d blocks" % depth)
        per_layer = [[] for _ in take]
        for b in range(x.shape[0]):
            for k, o in enumerate(self._takes(x[b], take, norm)):
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


class DeviceViT(DeviceEncoder):
    DTYPE, X_NORM_DTYPE = torch.float16, torch.float16
    DTYPE_REFUSAL = "a module that is not in torch.float16 (the fp32 use of this class is Depth-Anything: out of scope)"
    BLOCK_C, CONFIG_C = lib.VitBlockF16, lib.VitConfigF16
    ENTRY, WORKSPACE_BYTES = "dr_vit_forward_f16", "dr_vit_workspace_bytes"

    # weights: packed images and float32 copies
    @staticmethod
    def _matrix(w):
        return pack_weight_f16(w.reshape(w.shape[0], -1).contiguous())

    _patch_w = _matrix

    @staticmethod
    def _vector(v):
        return v.float().reshape(-1).contiguous()

    @staticmethod
    def _image(img):
        return img if img.dtype in (torch.float16, torch.float32) else img.to(torch.float16)

    @staticmethod
    def _flags(img, norm):
        assert not norm, "dr_vit_forward_f16 has no norm_take: _takes norms"
        return dict(img_f32=1 if img.dtype == torch.float32 else 0)

    def _features(self, x_norm, x_pre, masks):
        return {"x_norm_clstoken": x_norm[:, 0], "x_norm_patchtokens": x_norm[:, 1:], "x_prenorm": x_pre, "masks": masks}

    def _takes(self, img, take, norm):
        """the entry hands back the raw fp32 streams: the final norm (or the cast) to fp16 rows is a launch of its own"""
        Wt = self._weights()
        outs = self._run(img, take)[2]
        return [layernorm_rows_f16(o, Wt["norm_g"], Wt["norm_b"], self.eps) if norm else o.to(torch.float16) for o in outs]


class Binding:
    """what bind() returns: `.device` is the DeviceViT, `.remove()` restores the module's own forward_features"""

    def __init__(self, vit, device):
        self.vit, self.device = vit, device

    def remove(self):
        self.vit.__dict__.pop("forward_features", None)


def bind(encoder):
    """re-bind encoder.dinov2_vitl14[0].forward_features ON THE INSTANCE to the device path (EXP/encoders.py:115).  The device path runs with
    gradients enabled as well: the reference wraps the call in torch.no_grad() and every parameter of the network is frozen."""
    vit = encoder.dinov2_vitl14[0]
    dev = DeviceViT(vit)                       # (refuses here, before anything is bound)

    def forward_features(x, masks=None):
        with torch.no_grad():
            return dev.forward_features(x, masks)
    vit.forward_features = forward_features
    return Binding(vit, dev)
