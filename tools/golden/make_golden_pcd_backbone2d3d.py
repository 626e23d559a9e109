"""Mint the 2D-3D point-backbone fixture by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_pcd_backbone2d3d.py REFERENCE_ROOT    # the directory holding Diff-Reg-2d3d/
    -> tests/golden/pcd_backbone2d3d.npz (gradients, losses, counts, checksums, output column sums),
       tests/golden/pcd_backbone2d3d_a_out.npz, tests/golden/pcd_backbone2d3d_c_out.npz (the three outputs, quantised)

The reference's own PointBackbone(1, 128, 64, 15, 0.0625, 0.05) (EXP/point_backbone.py:8-95, built as at EXP/model.py:203-210) with vision3d's
KPConv / GroupNorm / pooling / kNN-interpolation code, on the graph pyramids of tests/pcd_backbone2d3d_ref.py (scene "a": 20 000 points, scene "c":
the sparse 600-point scene with a one-entry neighbour list and an all-shadow upsampling row), once as shipped (float32) and once with module.double()
and float64 inputs.  Loss = sum_i <out_i, w_i> (hash-drawn w_i, tests/pcd_backbone2d3d_ref.loss_weights).  EXP =
Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.

One replacement: vision3d.layers.kpconv.load_kernels reads a kernel disposition from a .ply file through Open3D and rotates it at random; here it is
tests/pcd_backbone2d3d_ref.kernel_disposition (the centre plus 14 points on a sphere from the integer hash), the i-th call getting index i.  The
kernel points are registered buffers, i.e. state-dict data, so the device path reads them from the module as it does any other buffer.  Imports need
stubs for vision3d.ext, open3d, cv2 and the other packages this path never calls.  Weights: tests/pcd_backbone2d3d_ref.make_weights (seed 5).

Decision condition, asserted here: the neighbour count of every KPConv call (feature sum > 0) is identical between the float32 and the float64 runs
for every query, and no real neighbour's float64 feature sum lies within 1e-6 max|sum| of zero.  A scene or a seed that fails either is no fixture.
Only reference OUTPUTS are stored.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-6


def main(ref_root):
    import torch
    for m in ("vision3d.ext", "ipdb", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops", "matplotlib",
              "matplotlib.pyplot"):
        sys.modules[m] = MagicMock()
    tree = os.path.join(ref_root, "Diff-Reg-2d3d")
    exp = os.path.join(tree, "experiments", "2d3dmatr.rgbdv2.stage4.level3.stage1")
    sys.path.insert(0, tree)
    sys.path.insert(0, exp)
    from tests import pcd_backbone2d3d_ref as R
    import vision3d.layers.kpconv as kpconv_mod
    calls = [0]

    def load_kernels(radius, num_kpoints, dimension=3, fixed="center", lloyd=False):
        assert num_kpoints == R.KERNEL_SIZE and dimension == 3 and fixed == "center"
        k = R.kernel_disposition(radius, calls[0]).astype(np.float64)
        calls[0] += 1
        return k
    kpconv_mod.load_kernels = load_kernels
    cwd = os.getcwd()
    os.chdir(exp)
    from point_backbone import PointBackbone
    os.chdir(cwd)
    torch.set_num_threads(8)
    ref = PointBackbone(1, 128, 64, 15, 0.025 * 2.5, 0.025 * 2.0)              # EXP/model.py:203-210 with EXP/config.py:96-103
    assert calls[0] == 8
    names = [n for n, _ in ref.named_parameters()]
    assert len(names) == 110, len(names)
    sd = R.make_weights(ref)
    ref.load_state_dict({**ref.state_dict(), **sd})
    # the restatement's module carries the same buffers (kernel_disposition, same call order)
    own = R.PointBackbone()
    for k, v in own.state_dict().items():
        if k.endswith("kernel_points"):
            assert torch.equal(v, ref.state_dict()[k]), k

    rec = []
    orig_fwd = kpconv_mod.KPConv.forward

    def recording_forward(self, q_points, s_points, s_feats, neighbor_indices):
        padded = torch.cat([s_feats, torch.zeros_like(s_feats[:1, :])], 0)
        sums = padded[neighbor_indices].sum(-1)
        real = neighbor_indices < s_feats.shape[0]
        rec.append(((sums > 0).sum(-1).detach().clone(), sums.detach().clone(), real))
        return orig_fwd(self, q_points, s_points, s_feats, neighbor_indices)
    kpconv_mod.KPConv.forward = recording_forward

    main_res, worst = {}, 0.0
    for scene in ("a", "c"):
        pyr = R.make_pyramid(scene)
        main_res[scene + "_pyramid_checksum"] = R.pyramid_checksum(pyr)
        out_res = {}
        runs = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            m = ref.to(dt)
            m.zero_grad(set_to_none=True)
            d = {k: [t.to(dt) if t.is_floating_point() else t for t in v] for k, v in R.to_torch(pyr).items()}
            feats = torch.ones(d["points"][0].shape[0], 1, dtype=dt)
            rec.clear()
            outs = m(feats, d)
            loss = R.loss_of(outs, R.loss_weights(outs))
            loss.backward()
            runs[tag] = (list(rec), [o.detach() for o in outs])
            main_res["%s_loss%s" % (scene, tag)] = np.array([float(loss.detach())])
            for n, p in m.named_parameters():
                main_res["%s_g%s_%s" % (scene, tag, n)] = R.sub_grad(p.grad).double().numpy() if tag == "64" else R.sub_grad(p.grad).numpy()
        # decision condition
        r32, r64 = runs["32"][0], runs["64"][0]
        assert len(r32) == len(r64) == 8, len(r32)
        for ci, ((c32, _, _), (c64, s64, real)) in enumerate(zip(r32, r64)):
            assert torch.equal(c32, c64), (scene, ci, int((c32 != c64).sum()))
            sm = float(s64[real].abs().max())
            near = int(((s64.abs() <= MARGIN * sm) & real).sum())
            assert near == 0, (scene, ci, near)
            main_res["%s_counts_%02d" % (scene, ci)] = c64.numpy().astype(np.int16)
        n = R.OUT_ROWS[scene]
        for i, o in enumerate(runs["64"][1]):
            q, step = R.quantise(o[::n].numpy())
            out_res["out%d_q" % i], out_res["out%d_step" % i] = q, step
            main_res["%s_out%d_colsum64" % (scene, i)] = o.sum(0).numpy()
            main_res["%s_out%d_shape" % (scene, i)] = np.array(o.shape)
            e = float((runs["32"][1][i].double() - o).abs().max() / o.abs().max())
            print("scene %s out%d %s: |ref32 - ref64| / max = %.2e" % (scene, i, tuple(o.shape), e))
        for nme in names:
            g32, g64 = main_res["%s_g32_%s" % (scene, nme)], main_res["%s_g64_%s" % (scene, nme)]
            worst = max(worst, float(np.abs(g32 - g64).max() / max(np.abs(g64).max(), 1e-30)))
        np.savez_compressed(os.path.join(GOLDEN, "pcd_backbone2d3d_%s_out.npz" % scene), **out_res)
        print("scene", scene, "losses", main_res[scene + "_loss32"], main_res[scene + "_loss64"])
    kpconv_mod.KPConv.forward = orig_fwd
    print("largest |g32 - g64| / max|g64| over the gradient tensors: %.3e" % worst)
    np.savez_compressed(os.path.join(GOLDEN, "pcd_backbone2d3d.npz"), **main_res)
    for f in ("pcd_backbone2d3d.npz", "pcd_backbone2d3d_a_out.npz", "pcd_backbone2d3d_c_out.npz"):
        print("wrote", f, os.path.getsize(os.path.join(GOLDEN, f)), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
