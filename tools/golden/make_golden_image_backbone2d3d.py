"""Mint the 2D-3D image-backbone fixture by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_image_backbone2d3d.py REFERENCE_ROOT    # the directory holding Diff-Reg-2d3d/
    -> tests/golden/image_backbone2d3d.npz

The reference's own ImageBackbone(1, out, 16) (EXP/image_backbone.py:69-289, built as at EXP/model.py:190-200 but 16 channels wide) on the three
cases of tests/image_backbone2d3d_ref.CASES, once as shipped (float32) and once with module.double() and float64 inputs.  Weights and inputs:
tests/image_backbone2d3d_ref.make_weights / make_inputs (seeded generators; nothing of them is stored beyond the inputs).  Stored per case:
the inputs, the four float64 outputs and `dev32` = max|out32 - out64| / max|out64| of each (the float32 outputs themselves are not kept); over the file, `floor` =
the smallest dev32 (the bound below which no float32 path is held).  Imports need stubs for vision3d.ext, open3d, cv2 and the other packages this
path never calls.  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.  Only reference OUTPUTS are stored.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def main(ref_root):
    import torch
    for m in ("vision3d.ext", "ipdb", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops", "matplotlib",
              "matplotlib.pyplot"):
        sys.modules[m] = MagicMock()
    tree = os.path.join(ref_root, "Diff-Reg-2d3d")
    exp = os.path.join(tree, "experiments", "2d3dmatr.rgbdv2.stage4.level3.stage1")
    sys.path.insert(0, tree)
    sys.path.insert(0, exp)
    from tests import image_backbone2d3d_ref as R
    cwd = os.getcwd()
    os.chdir(exp)
    from image_backbone import ImageBackbone
    os.chdir(cwd)
    torch.set_num_threads(8)
    res, floor = {}, float("inf")
    for name, case in R.CASES.items():
        ref = ImageBackbone(1, case["out"], case["base"]).eval()
        own = R.ImageBackbone(1, case["out"], case["base"])
        assert [n for n, _ in ref.named_parameters()] == [n for n, _ in own.named_parameters()], "state-dict names differ"
        assert len(list(ref.named_buffers())) == 0
        ref.load_state_dict(R.make_weights(ref, case["seed"]))
        x, dino = R.make_inputs(case)
        res[name + "_in_x"], res[name + "_in_dino"] = x.numpy(), dino.numpy()
        with torch.no_grad():
            o32 = ref(x, dino)
            o64 = ref.double()(x.double(), dino.double())
        dev = []
        for i, (a, b) in enumerate(zip(o32, o64)):
            assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape
            res["%s_out%d_64" % (name, i)] = b.numpy()
            dev.append(R.rel_dev(a, b))
            print("case %s out%d %s: |ref32 - ref64| / max = %.2e" % (name, i, tuple(b.shape), dev[-1]))
        res[name + "_dev32"] = np.array(dev)
        floor = min(floor, min(dev))
    res["floor"] = np.array([floor])
    print("floor = %.3e" % floor)
    path = os.path.join(GOLDEN, "image_backbone2d3d.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
