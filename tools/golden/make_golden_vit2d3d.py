"""Mint the DINOv2 ViT encoder fixture by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only; xFormers absent, i.e. the
Attention.forward path of layers/attention.py:49-62):

    python tools/golden/make_golden_vit2d3d.py REFERENCE_ROOT    # the directory holding Diff-Reg-2d3d/; writes tests/golden/vit2d3d_*.npz

The reference's own DinoVisionTransformer (Diff-Reg-2d3d/transformer/dinov2.py) is built small -- patch 14, img_size 70, width 128, 2 blocks,
2 heads of 64, mlp_ratio 4, init_values 1.0, ffn_layer "mlp", block_chunks 0, block_fn Block with MemEffAttention -- and its weights are re-drawn at
a checkpoint-like scale (tests/vit2d3d_ref.draw_weights, by parameter name: the two classes share their names) and cast to fp16.  For the three
images of vit2d3d_ref.IMAGES it stores, from the fp16 run and from a float64 copy of the same fp16 weights on the same fp16 input:
forward_features (x_norm_patchtokens, x_norm_clstoken, x_prenorm), get_intermediate_layers(x, [0, 1], return_class_token=True, norm=True) and the
position rows.  Data only: fp16 weights as fp16, the inputs as fp16, every output as float64; one file per (image, run) to stay under the size limit.
"""
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import vit2d3d_ref as R  # noqa: E402


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "Diff-Reg-2d3d"))
    from transformer.dinov2 import DinoVisionTransformer
    from transformer.layers.attention import MemEffAttention
    from transformer.layers.block import Block
    c = R.FIXTURE_CFG
    torch.manual_seed(0)
    vit = DinoVisionTransformer(patch_size=c["patch_size"], img_size=c["img_size"], embed_dim=c["embed_dim"], depth=c["depth"],
                                num_heads=c["num_heads"], mlp_ratio=c["mlp_ratio"], init_values=1.0, ffn_layer="mlp", block_chunks=0,
                                block_fn=partial(Block, attn_class=MemEffAttention)).eval()
    R.draw_weights(vit, seed=20)
    vit = vit.to(torch.float16)
    sd = {k: v for k, v in vit.state_dict().items() if k != "mask_token"}
    out = os.path.join(ROOT, "tests", "golden")
    np.savez(os.path.join(out, "vit2d3d_w.npz"), **{"w." + k: v.numpy() for k, v in sd.items()})
    v64 = DinoVisionTransformer(patch_size=c["patch_size"], img_size=c["img_size"], embed_dim=c["embed_dim"], depth=c["depth"],
                                num_heads=c["num_heads"], mlp_ratio=c["mlp_ratio"], init_values=1.0, ffn_layer="mlp", block_chunks=0,
                                block_fn=partial(Block, attn_class=MemEffAttention)).eval()
    v64.load_state_dict(vit.state_dict())
    v64 = v64.double()
    g = torch.Generator().manual_seed(21)
    for i, (H, W) in enumerate(R.IMAGES):
        x = (torch.randn(1, 3, H, W, generator=g)).to(torch.float16)          # an ImageNet-normalised image has about this spread
        np.savez(os.path.join(out, "vit2d3d_img%d_in.npz" % i), **{"img%d.x" % i: x.numpy()})
        for tag, m, xi in (("f16", vit, x), ("f64", v64, x.double())):
            with torch.no_grad():
                ff = m.forward_features(xi)
                il = m.get_intermediate_layers(xi, [0, 1], return_class_token=True, norm=True)
                L = 1 + (H // 14) * (W // 14)
                pos = m.interpolate_pos_encoding(torch.zeros(1, L, c["embed_dim"], dtype=xi.dtype), H, W)
            rec = {"x_norm_patchtokens": ff["x_norm_patchtokens"], "x_norm_clstoken": ff["x_norm_clstoken"], "x_prenorm": ff["x_prenorm"], "pos": pos}
            for k, (o, cl) in enumerate(il):
                rec["inter%d" % k] = o
                rec["inter%d_cls" % k] = cl
            np.savez_compressed(os.path.join(out, "vit2d3d_img%d_%s.npz" % (i, tag)),
                                **{"img%d.%s.%s" % (i, tag, k): v.double().numpy() for k, v in rec.items()})
    for f in sorted(os.listdir(out)):
        if f.startswith("vit2d3d"):
            print(f, os.path.getsize(os.path.join(out, f)))


if __name__ == "__main__":
    main(sys.argv[1])
