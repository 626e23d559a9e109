"""Mint the DPT-head fixture by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_dpt2d3d.py REFERENCE_ROOT    # the directory holding Diff-Reg-2d3d/
    -> tests/golden/dpt2d3d_weights_NN.npz, tests/golden/dpt2d3d_<grid>_NN.npz

The reference's own DPTHead (depth_anything/dpt.py:22-136) built small -- tests/dpt2d3d_ref.SMALL: in_channels 128, features 32, out_channels
[16, 32, 64, 64], use_bn False, use_clstoken False -- with its weights re-drawn by tests/dpt2d3d_ref.draw_weights (a seeded generator, a
checkpoint-like scale, biases away from zero), run as shipped (float32) and as module.double() on float64 copies of the same inputs, on the
patch grids of tests/dpt2d3d_ref.GRIDS.  Inputs: four random [1, L, 128] token tensors with their class tokens (dpt2d3d_ref.make_inputs).
Stored: the weights (float32); per grid the inputs, every named intermediate (the four reassembled layers, path_4 .. path_1, output_conv1: forward
hook outputs) and the output of the float64 run as float64, and `dev32_<name>` = max|t32 - t64| / max|t64| of the float32 run for each of them
(the float32 tensors themselves are not kept: the float64 tensors of the 10 x 13 grid alone are 4.6 MB); over all of it `floor`, the smallest
dev32 (the bound below which no float32 path is held).  Every file stays under 1 MiB: a large array is cut into parts (dpt2d3d_ref.save_parts).
Only data is stored.  depth_anything/dpt.py imports huggingface_hub at its top (installed); cv2 is not needed.
"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)


def main(ref_root):
    import torch
    sys.path.insert(0, os.path.join(ref_root, "Diff-Reg-2d3d"))
    from depth_anything.dpt import DPTHead
    from tests import dpt2d3d_ref as R
    torch.set_num_threads(8)
    S = R.SMALL
    ref = DPTHead(1, S["in_channels"], S["features"], False, out_channels=list(S["out_channels"]), use_clstoken=False).eval()
    own = R.DPTHead(S["in_channels"], S["features"], S["out_channels"])
    assert list(ref.state_dict()) == list(own.state_dict()), "state-dict names differ"
    weights = R.draw_weights(ref, R.WEIGHT_SEED)
    ref.load_state_dict(weights)
    for old in glob.glob(R.golden_prefix(ROOT, "*")):
        os.remove(old)
    floor = float("inf")
    for name, (ph, pw) in R.GRIDS.items():
        feats = R.make_inputs((ph, pw), R.grid_seed(name))
        res = {}
        for i, (tok, cls) in enumerate(feats):
            res["in_tok%d" % i], res["in_cls%d" % i] = tok.numpy(), cls.numpy()
        ref.float()
        t32 = R.run_named(ref, feats, ph, pw)
        ref.double()
        t64 = R.run_named(ref, tuple((a.double(), b.double()) for a, b in feats), ph, pw)
        for n in R.NAMES:
            a, b = t32[n], t64[n]
            assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape
            res[n + "_64"] = b.numpy()
            d = R.rel_dev(a, b)
            res["dev32_" + n] = np.array([d])
            floor = min(floor, d)
            print("grid %s %-12s %-18s |ref32 - ref64| / max = %.2e" % (name, n, tuple(b.shape), d))
        for p in R.save_parts(R.golden_prefix(ROOT, name), res):
            print("wrote", p, os.path.getsize(p), "bytes")
    w = {k: v.numpy() for k, v in weights.items()}
    w["floor"] = np.array([floor])
    print("floor = %.3e" % floor)
    for p in R.save_parts(R.golden_prefix(ROOT, "weights"), w):
        print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
