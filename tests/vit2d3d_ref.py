"""A plain-torch restatement of the DINOv2 ViT encoder the 2D-3D model keeps frozen (Diff-Reg-2d3d/transformer/dinov2.py and its layers), at any
dtype, with the attribute names diffreg_hip.vit2d3d.DeviceViT reads -- and a stand-in for CNNandDinov2 (EXP/encoders.py:78-119) that holds the ViT in a
list.  tests/test_vit2d3d_oracle.py holds it to the reference's own recorded outputs (tests/golden/vit2d3d*.npz), which licenses it as the float64
yardstick for shapes the fixture lacks."""
import glob
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_CFG = dict(patch_size=14, img_size=70, embed_dim=128, depth=2, num_heads=2, mlp_ratio=4)
IMAGES = [(42, 70), (70, 70), (140, 182)]


class Scale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class Attn(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x):
        B, N, C = x.shape
        d = C // self.num_heads
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, d).permute(2, 0, 3, 1, 4)
        a = ((q * d ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1)
        return self.proj((a @ v).transpose(1, 2).reshape(B, N, C))


class FFN(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class EncoderBlock(nn.Module):
    def __init__(self, dim, num_heads, hidden):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attn(dim, num_heads)
        self.ls1 = Scale(dim)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = FFN(dim, hidden)
        self.ls2 = Scale(dim)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class Patches(nn.Module):
    def __init__(self, patch_size, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, patch_size, stride=patch_size)
        self.norm = nn.Identity()

    def forward(self, x):
        return self.norm(self.proj(x).flatten(2).transpose(1, 2))


class ViT(nn.Module):
    def __init__(self, patch_size=14, img_size=518, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4):
        super().__init__()
        self.patch_size, self.num_heads = patch_size, num_heads
        self.patch_embed = Patches(patch_size, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, (img_size // patch_size) ** 2 + 1, embed_dim))
        self.blocks = nn.ModuleList([EncoderBlock(embed_dim, num_heads, int(embed_dim * mlp_ratio)) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        for prm in self.parameters():
            prm.requires_grad = False

    def interpolate_pos_encoding(self, x, w, h):
        """position rows for an image of w x h pixels (first, second spatial extent): the trained grid itself when the patch count matches and the
        image is square, else its bicubic resample in float32 by the scale factors ((extent / patch) + 0.1) / grid"""
        n_grid = self.pos_embed.shape[1] - 1
        if x.shape[1] - 1 == n_grid and w == h:
            return self.pos_embed
        pe = self.pos_embed.float()
        g = int(math.sqrt(n_grid))
        w0, h0 = w // self.patch_size + 0.1, h // self.patch_size + 0.1
        grid = pe[:, 1:].reshape(1, g, g, -1).permute(0, 3, 1, 2)
        grid = F.interpolate(grid, scale_factor=(w0 / math.sqrt(n_grid), h0 / math.sqrt(n_grid)), mode="bicubic")
        assert (int(w0), int(h0)) == tuple(grid.shape[-2:])
        return torch.cat((pe[:, :1], grid.permute(0, 2, 3, 1).reshape(1, -1, pe.shape[-1])), dim=1).to(x.dtype)

    def tokens(self, x):
        _, _, w, h = x.shape
        t = self.patch_embed(x)
        t = torch.cat((self.cls_token.expand(t.shape[0], -1, -1), t), dim=1)
        return t + self.interpolate_pos_encoding(t, w, h)

    def forward_features(self, x, masks=None):
        assert masks is None
        t = self.tokens(x)
        for b in self.blocks:
            t = b(t)
        n = self.norm(t)
        return {"x_norm_clstoken": n[:, 0], "x_norm_patchtokens": n[:, 1:], "x_prenorm": t, "masks": masks}

    def get_intermediate_layers(self, x, n=1, reshape=False, return_class_token=False, norm=True):
        take = range(len(self.blocks) - n, len(self.blocks)) if isinstance(n, int) else n
        t, outs = self.tokens(x), []
        for i, b in enumerate(self.blocks):
            t = b(t)
            if i in take:
                outs.append(self.norm(t) if norm else t)
        cls = [o[:, 0] for o in outs]
        outs = [o[:, 1:] for o in outs]
        if reshape:
            B, _, w, h = x.shape
            outs = [o.reshape(B, w // self.patch_size, h // self.patch_size, -1).permute(0, 3, 1, 2).contiguous() for o in outs]
        return tuple(zip(outs, cls)) if return_class_token else tuple(outs)


class EncoderStandIn(nn.Module):
    """CNNandDinov2's DINOv2 half: the ViT in a list (hidden from .parameters()), key 16 of the returned pyramid = its patch tokens as a map"""

    def __init__(self, vit):
        super().__init__()
        self.dinov2_vitl14 = [vit]

    def forward(self, x):
        B, _, H, W = x.shape
        with torch.no_grad():
            f = self.dinov2_vitl14[0].forward_features(x.to(torch.float16))["x_norm_patchtokens"]
        p = self.dinov2_vitl14[0].patch_size
        return {16: f.permute(0, 2, 1).reshape(B, -1, H // p, W // p)}


def draw_weights(vit, seed):
    """checkpoint-like scales (LayerScale at 1 and zero biases would hide both): Linear / Conv weights x 3, biases N(0, 0.1), LayerScale U(0.2, 1.5),
    LayerNorm weights U(0.5, 1.5), cls N(0, 0.5), pos N(0, 0.02)"""
    dev = next(vit.parameters()).device          # drawn where the module lives
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for name, prm in vit.named_parameters():
            shp = prm.shape
            if name.endswith("gamma"):
                prm.copy_(torch.rand(shp, generator=g, device=dev) * 1.3 + 0.2)
            elif "norm" in name and name.endswith("weight"):
                prm.copy_(torch.rand(shp, generator=g, device=dev) + 0.5)
            elif name.endswith("bias"):
                prm.copy_(torch.randn(shp, generator=g, device=dev) * 0.1)
            elif name == "cls_token":
                prm.copy_(torch.randn(shp, generator=g, device=dev) * 0.5)
            elif name == "pos_embed":
                prm.copy_(torch.randn(shp, generator=g, device=dev) * 0.02)
            else:
                prm.copy_(torch.randn(shp, generator=g, device=dev) * 0.02 * 3)
    return vit


def load_fixture():
    """every array of tests/golden/vit2d3d*.npz in one dict"""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "vit2d3d*.npz"))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def fixture_vit(fx, dtype):
    """the restatement with the fixture's fp16 weights, cast to dtype"""
    vit = ViT(**FIXTURE_CFG)
    sd = {k[2:]: torch.from_numpy(v.astype(np.float32)) for k, v in fx.items() if k.startswith("w.")}
    missing = vit.load_state_dict(sd, strict=True)
    assert not missing.missing_keys
    return vit.to(dtype).eval()
