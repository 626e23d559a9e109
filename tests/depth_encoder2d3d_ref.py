"""A plain-torch restatement of Depth-Anything's ViT encoder (`DPT_DINOv2.pretrained`, the hub's DinoVisionTransformer:
torchhub/facebookresearch_dinov2_main/vision_transformer.py built by hubconf._make_dinov2_model with block_chunks=0, init_values=1.0,
ffn_layer="mlp", no register tokens), at any dtype, with the attribute names diffreg_hip.depth_encoder2d3d.DeviceViTF32 reads.  It is the class
of tests/vit2d3d_ref.py (the same arithmetic: the hub file and transformer/dinov2.py differ in names only) plus what the hub class adds to the
interface: `num_register_tokens`, `register_tokens` and the (empty) `x_norm_regtokens` entry.  tests/test_depth_encoder2d3d_oracle.py holds it to
the reference's own recorded outputs (tests/golden/depth_encoder2d3d_*.npz), which licenses it as the float64 yardstick for shapes the fixture
lacks -- and a stand-in for DPT_DINOv2 (depth_anything/dpt.py:140-166) around it."""
import glob
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import vit2d3d_ref as V

GOLDEN = V.GOLDEN
FIXTURE_CFG = dict(patch_size=14, img_size=70, embed_dim=128, depth=4, num_heads=2, mlp_ratio=4)
IMAGES = [(42, 70), (70, 70), (140, 182)]
TENSORS = ["inter0", "inter0_cls", "inter1", "inter1_cls", "inter2", "inter2_cls", "inter3", "inter3_cls", "x_norm_patchtokens", "x_norm_clstoken",
           "x_prenorm"]
draw_weights = V.draw_weights


class ViTF32(V.ViT):
    num_register_tokens = 0
    register_tokens = None

    def forward_features(self, x, masks=None):
        out = super().forward_features(x, masks)
        n = torch.cat((out["x_norm_clstoken"][:, None], out["x_norm_patchtokens"]), dim=1)
        return {"x_norm_clstoken": out["x_norm_clstoken"], "x_norm_regtokens": n[:, 1:1], "x_norm_patchtokens": out["x_norm_patchtokens"],
                "x_prenorm": out["x_prenorm"], "masks": masks}


class DepthModelStandIn(nn.Module):
    """DPT_DINOv2 (depth_anything/dpt.py:140-166): `pretrained` the ViT, `depth_head` any callable head, forward as the reference's"""

    def __init__(self, vit, head):
        super().__init__()
        self.pretrained, self.depth_head = vit, head

    def forward(self, x):
        h, w = x.shape[-2:]
        features = self.pretrained.get_intermediate_layers(x, 4, return_class_token=True)
        patch_h, patch_w = h // 14, w // 14
        depth = self.depth_head(features, patch_h, patch_w)
        depth = F.interpolate(depth, size=(h, w), mode="bilinear", align_corners=True)
        return F.relu(depth).squeeze(1)


def load_fixture():
    """every array of tests/golden/depth_encoder2d3d_*.npz in one dict"""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "depth_encoder2d3d_*.npz"))):
        with np.load(path) as z:
            out.update({k: z[k] for k in z.files})
    return out


def fixture_vit(fx, dtype, device="cpu"):
    """the restatement with the fixture's float32 weights, cast to dtype"""
    vit = ViTF32(**FIXTURE_CFG)
    sd = {k[2:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("w.")}
    missing = vit.load_state_dict(sd, strict=True)
    assert not missing.missing_keys
    return vit.to(dtype).to(device).eval()


def run_all(vit, x):
    """{tensor name: tensor} of TENSORS for one batch x"""
    with torch.no_grad():
        ff = vit.forward_features(x)
        il = vit.get_intermediate_layers(x, 4, return_class_token=True)
    rec = {"x_norm_patchtokens": ff["x_norm_patchtokens"], "x_norm_clstoken": ff["x_norm_clstoken"], "x_prenorm": ff["x_prenorm"]}
    for k, (o, cl) in enumerate(il):
        rec["inter%d" % k] = o
        rec["inter%d_cls" % k] = cl
    return rec
