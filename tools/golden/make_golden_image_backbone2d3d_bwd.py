"""Mint the 2D-3D image-backbone GRADIENT fixture by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_image_backbone2d3d_bwd.py REFERENCE_ROOT    # the directory holding Diff-Reg-2d3d/
    -> tests/golden/image_backbone2d3d_bwd.npz, tests/golden/image_backbone2d3d_bwd_<n>.npz

The reference's own ImageBackbone(1, out, 16) (EXP/image_backbone.py:69-289) on cases b and c of tests/image_backbone2d3d_ref.CASES, once as shipped
(float32) and once with module.double() and float64 inputs.  The loss is sum_i <out_i, cot_i> with the cotangents of
tests/image_backbone2d3d_bwd_ref.cotangents (a generator seeded seed + 2000, float32, output order); then backward().  Stored per case: the
float64 gradient of every parameter, of x and of dino_feat ('<case>/<name>'), `<case>_dev32` = max|g32 - g64| / max|g64| per gradient tensor in
the order of `<case>_names`, and `<case>_floor` = the median of that case's dev32.  The float32 gradients themselves are not kept.  The tensors
are spread over several files of at most 900 KiB (the first one holds the index and the deviations): tests/image_backbone2d3d_bwd_ref.load joins
them.  Imports need stubs for vision3d.ext, open3d, cv2 and the other packages this path never calls.
EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.  Only reference OUTPUTS are stored.
"""
import glob
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
    from tests import image_backbone2d3d_bwd_ref as B
    cwd = os.getcwd()
    os.chdir(exp)
    from image_backbone import ImageBackbone
    os.chdir(cwd)
    torch.set_num_threads(8)
    head, big = {}, []
    for name in B.BWD_CASES:
        case = R.CASES[name]
        ref = ImageBackbone(1, case["out"], case["base"]).eval()
        own = R.ImageBackbone(1, case["out"], case["base"])
        assert [n for n, _ in ref.named_parameters()] == [n for n, _ in own.named_parameters()], "state-dict names differ"
        ref.load_state_dict(R.make_weights(ref, case["seed"]))
        x, dino = R.make_inputs(case)
        _, g32 = B.run_backward(ref, x, dino, case)
        g32 = {k: v.clone() for k, v in g32.items()}
        _, g64 = B.run_backward(ref.double(), x, dino, case)
        names, dev, count = B.grad_names(ref), [], 0
        for n in names:
            a, b = g32[n], g64[n]
            assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == b.shape and float(b.abs().max()) > 0, n
            dev.append(R.rel_dev(a, b))
            count += b.numel()
            arr = b.numpy().copy()
            if arr.nbytes > 16 * 1024:
                big.append(("%s/%s" % (name, n), arr))
            else:
                head["%s/%s" % (name, n)] = arr
        head[name + "_names"] = np.array(names)
        head[name + "_dev32"] = np.array(dev)
        head[name + "_floor"] = np.array([float(np.median(dev))])
        print("case %s: %d tensors, %d values, dev32 %.2e .. %.2e, floor (median) %.3e" % (name, len(names), count, min(dev), max(dev), float(np.median(dev))))
    for old in glob.glob(os.path.join(GOLDEN, "image_backbone2d3d_bwd*.npz")):
        os.remove(old)
    parts, cur, size = [], {}, 0
    for key, arr in big:
        if cur and size + arr.nbytes > B.PART_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[key] = arr
        size += arr.nbytes
    if cur:
        parts.append(cur)
    files = [("image_backbone2d3d_bwd.npz", head)] + [("image_backbone2d3d_bwd_%02d.npz" % i, p) for i, p in enumerate(parts)]
    for fn, d in files:
        path = os.path.join(GOLDEN, fn)
        np.savez_compressed(path, **d)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
