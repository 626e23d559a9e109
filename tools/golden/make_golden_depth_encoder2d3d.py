"""Mint the Depth-Anything ViT encoder fixture by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only; xFormers absent, i.e. the plain
Attention.forward path of dinov2/layers/attention.py:49-62):

    python tools/golden/make_golden_depth_encoder2d3d.py REFERENCE_ROOT    # the directory holding Diff-Reg-2d3d/; writes tests/golden/depth_encoder2d3d_*.npz

The reference's own hub class (Diff-Reg-2d3d/torchhub/facebookresearch_dinov2_main/vision_transformer.py, the class hubconf._make_dinov2_model
builds for DPT_DINOv2.pretrained) is built small -- patch 14, img_size 70, width 128, 4 blocks, 2 heads of 64, mlp_ratio 4, init_values 1.0,
ffn_layer "mlp", block_chunks 0, block_fn NestedTensorBlock with MemEffAttention, no register tokens -- and its weights are re-drawn at a
checkpoint-like scale (tests/vit2d3d_ref.draw_weights, by parameter name).  With 4 blocks the reference's n = 4 takes every block.  For the three
images of depth_encoder2d3d_ref.IMAGES it runs the module in float32 and as a float64 copy of the same weights on the same float32 input and
stores: get_intermediate_layers(x, 4, return_class_token=True), the three forward_features tensors and the position rows as float64, and per
tensor the float32 run's max |deviation| from the float64 one ("dev32").  The float32 tensors themselves are not stored.  Data only: the float32
weights cut per block, the inputs as float32; every file stays well under the size limit.
"""
import os
import sys
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import depth_encoder2d3d_ref as R  # noqa: E402


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "Diff-Reg-2d3d", "torchhub", "facebookresearch_dinov2_main"))
    from vision_transformer import DinoVisionTransformer
    from dinov2.layers import MemEffAttention, NestedTensorBlock
    c = R.FIXTURE_CFG

    def build():
        return DinoVisionTransformer(patch_size=c["patch_size"], img_size=c["img_size"], embed_dim=c["embed_dim"], depth=c["depth"],
                                     num_heads=c["num_heads"], mlp_ratio=c["mlp_ratio"], init_values=1.0, ffn_layer="mlp", block_chunks=0,
                                     block_fn=partial(NestedTensorBlock, attn_class=MemEffAttention)).eval()
    torch.manual_seed(0)
    vit = build()
    R.draw_weights(vit, seed=30)
    print("parameters:", sum(p.numel() for n, p in vit.named_parameters() if n != "mask_token"))
    sd = {k: v for k, v in vit.state_dict().items() if k != "mask_token"}
    out = os.path.join(ROOT, "tests", "golden")
    np.savez(os.path.join(out, "depth_encoder2d3d_w_stem.npz"), **{"w." + k: v.numpy() for k, v in sd.items() if not k.startswith("blocks.")})
    for i in range(c["depth"]):
        pre = "blocks.%d." % i
        np.savez(os.path.join(out, "depth_encoder2d3d_w_block%d.npz" % i), **{"w." + k: v.numpy() for k, v in sd.items() if k.startswith(pre)})
    v64 = build()
    v64.load_state_dict(vit.state_dict())
    v64 = v64.double()
    g = torch.Generator().manual_seed(31)
    for i, (H, W) in enumerate(R.IMAGES):
        x = torch.randn(1, 3, H, W, generator=g)                            # an ImageNet-normalised image has about this spread
        recs = {}
        for tag, m, xi in (("f32", vit, x), ("f64", v64, x.double())):
            rec = R.run_all(m, xi)
            L = 1 + (H // 14) * (W // 14)
            with torch.no_grad():
                rec["pos"] = m.interpolate_pos_encoding(torch.zeros(1, L, c["embed_dim"], dtype=xi.dtype), H, W)
            recs[tag] = rec
        store = {"img%d.x" % i: x.numpy()}
        for k, v in recs["f64"].items():
            store["img%d.f64.%s" % (i, k)] = v.detach().double().numpy()
            if k != "pos":
                store["img%d.dev32.%s" % (i, k)] = np.float64((recs["f32"][k].double() - v).abs().max().item())
        inter = {k: v for k, v in store.items() if ".f64.inter" in k}              # two files per image: each stays under the size limit
        np.savez_compressed(os.path.join(out, "depth_encoder2d3d_img%d_inter.npz" % i), **inter)
        np.savez_compressed(os.path.join(out, "depth_encoder2d3d_img%d_ff.npz" % i), **{k: v for k, v in store.items() if k not in inter})
        print(i, {k: float(v) for k, v in store.items() if ".dev32." in k})
    for f in sorted(os.listdir(out)):
        if f.startswith("depth_encoder2d3d"):
            print(f, os.path.getsize(os.path.join(out, f)))


if __name__ == "__main__":
    main(sys.argv[1])
