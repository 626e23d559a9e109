"""Mint the fixture of the 2D-3D geometry head by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_front2d3d.py REFERENCE_ROOT    # the directory holding Diff-Reg-2d3d/; writes tests/golden/front2d3d.npz

The reference's own vision3d.ops.back_project, vision3d.ops.render and MATR2D3D.back_project_depth (taken unbound from the class: the model
itself cannot be constructed offline) run on the deterministic cases of tests/front2d3d_ref.py in float32 and in float64 (inputs cast).
vision3d.ops.create_meshgrid calls `.cuda()` and is not minted: the tests pin it to its definition (cartesian_prod of arange / linspace).
EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.  Stored: the inputs of every case and, per dtype tag 32 / 64, every output.
The fixture rules (front2d3d_ref.fixture_rules) are asserted here.  Stubs as tools/golden/make_golden_finenoise2d3d.py.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "front2d3d.npz")
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)


def main(ref_root):
    import torch
    for m in ("vision3d.ext", "ipdb", "IPython", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops"):
        sys.modules[m] = MagicMock()
    tree = os.path.join(ref_root, "Diff-Reg-2d3d")
    exp = os.path.join(tree, "experiments", "2d3dmatr.rgbdv2.stage4.level3.stage1")
    sys.path.insert(0, tree)
    sys.path.insert(0, exp)
    cwd = os.getcwd()
    os.chdir(exp)
    while True:                                                             # model.py imports the backbones' dependencies: stub whichever is absent
        try:
            from vision3d.ops import back_project, render
            import model as ref_model
            break
        except ModuleNotFoundError as e:
            sys.modules[e.name] = MagicMock()
    os.chdir(cwd)
    back_project_depth = ref_model.MATR2D3D.back_project_depth               # unbound: `self` is not read
    from tests import front2d3d_ref as F
    assert F.fixture_rules() == [], F.fixture_rules()
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    res = {}
    for name, kw in F.BACK_PROJECT_CASES.items():
        c = F.make_back_project(**kw)
        for k in ("depth", "intrinsics", "a", "b"):
            res["%s_in_%s" % (name, k)] = np.asarray(c[k])
        for tag, tdt in (("32", torch.float32), ("64", torch.float64)):
            d, K = t(c["depth"], tdt), t(c["intrinsics"], tdt)
            if kw["mode"] == 0:
                pts, mask = back_project(d, K, scaling_factor=float(c["a"]), depth_limit=F.DEPTH_LIMIT, transposed=True, return_mask=True)
            else:
                pts, mask = back_project_depth(None, d, K, scaling_factor_a=t(c["a"], tdt), scaling_factor_b=t(c["b"], tdt),
                                               depth_limit=F.DEPTH_LIMIT, transposed=True, return_mask=True)
            assert pts.dtype == tdt and mask.dtype == torch.bool and tuple(pts.shape) == (1, kw["H"], kw["W"], 3)
            res["%s_points%s" % (name, tag)] = pts.reshape(-1, 3).numpy()
            res["%s_mask%s" % (name, tag)] = mask.reshape(-1).numpy()
        assert np.array_equal(res[name + "_mask32"], res[name + "_mask64"]), name
        print(name, "float32 from float64 %.3e" % F.rel_dev(res[name + "_points32"], res[name + "_points64"]), "kept", int(res[name + "_mask64"].sum()))
    for name, kw in F.RENDER_CASES.items():
        c = F.make_render(**kw)
        res["%s_in_points" % name], res["%s_in_intrinsics" % name] = c["points"], c["intrinsics"]
        if c["extrinsics"] is not None:
            res["%s_in_extrinsics" % name] = c["extrinsics"]
        for tag, tdt in (("32", torch.float32), ("64", torch.float64)):
            T = None if c["extrinsics"] is None else t(c["extrinsics"], tdt)
            pix, z = render(t(c["points"], tdt), t(c["intrinsics"], tdt), extrinsics=T, rounding=False, return_depth=True)
            assert pix.dtype == tdt and tuple(pix.shape) == (kw["N"], 2)
            res["%s_pixels%s" % (name, tag)], res["%s_depth%s" % (name, tag)] = pix.numpy(), z.numpy()
        print(name, "float32 from float64 %.3e" % F.rel_dev(res[name + "_pixels32"], res[name + "_pixels64"]))
    np.savez_compressed(OUT, **res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(res), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
