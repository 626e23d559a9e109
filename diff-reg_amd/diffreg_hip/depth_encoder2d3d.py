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

from . import lib
from .vit2d3d import DeviceEncoder

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
class DeviceViTF32(DeviceEncoder):
    DTYPE, X_NORM_DTYPE = torch.float32, torch.float32
    DTYPE_REFUSAL = "a module that is not entirely torch.float32 (the fp16 use of this class is diffreg_hip.vit2d3d.DeviceViT)"
    BLOCK_C, CONFIG_C = lib.VitBlockF32, lib.VitConfigF32
    ENTRY, WORKSPACE_BYTES = "dr_vit_forward_f32", "dr_vit_workspace_bytes_f32"

    def _refuse_module(self, module):
        if getattr(module, "num_register_tokens", 0) != 0 or getattr(module, "register_tokens", None) is not None:
            self._refuse("register tokens (num_register_tokens = %r)" % getattr(module, "num_register_tokens", None))

    # weights: the module's own storage where the kernels can read it (contiguous; 16-byte aligned, which the entry asks of a matrix only), else
    # a copy; the patch embedding's flattened weight is copied, padded to a multiple of 32 columns
    @staticmethod
    def _view(t):
        t = t.contiguous()
        return t if t.data_ptr() % 16 == 0 else t.clone()

    @classmethod
    def _matrix(cls, w):
        return cls._view(w.reshape(w.shape[0], -1))

    @classmethod
    def _vector(cls, v):
        return cls._view(v.reshape(-1))

    @staticmethod
    def _patch_w(w):
        flat = w.reshape(w.shape[0], -1)
        Kp = (flat.shape[1] + 31) // 32 * 32
        return torch.nn.functional.pad(flat, (0, Kp - flat.shape[1])).contiguous()

    @staticmethod
    def _image(img):
        return img.to(torch.float32)

    @staticmethod
    def _flags(img, norm):
        return dict(norm_take=1 if norm else 0)

    def _run(self, img, take=(), norm=True, workspace=None):
        """img [3, H, W] float32 -> (x_prenorm [L, D], x_norm [L, D], [the stream after block i (through the final norm if `norm`) for i in take]);
        `workspace`: the caller's own bytes instead of a fresh allocation"""
        return super()._run(img, take, norm, workspace)

    def _features(self, x_norm, x_pre, masks):
        return {"x_norm_clstoken": x_norm[:, 0], "x_norm_regtokens": x_norm[:, 1:1], "x_norm_patchtokens": x_norm[:, 1:], "x_prenorm": x_pre,
                "masks": masks}

    def _takes(self, img, take, norm):
        return self._run(img, take, norm)[2]          # the entry writes the final norm of each taken stream itself


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
