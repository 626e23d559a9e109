"""Mint the 2D-3D training-branch fixture by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_train2d3d.py REFERENCE_ROOT     # the directory holding Diff-Reg-2d3d/; writes tests/golden/train2d3d_branch.npz

The reference's own CrossModalFusionModule (EXP/fusion_module.py), Matching (EXP/matching.py) and CoarseMatchingLoss (EXP/loss.py, with
vision3d's CircleLoss) compose the differentiable part of MATR2D3D.forward's training branch (EXP/model.py:386-392, 548-553, 615-631; the GT
search and q_sample replaced by given inputs) and OverallLoss's coarse term (EXP/loss.py:226-238: loss_circle + loss_matrix_gt_hat) is
back-propagated, once with the modules as shipped (float32) and once with module.double() and float64 inputs.  Stored, per dtype tag 32 / 64:
the four losses, every parameter gradient (entries [::16, ::16] of a matrix, all entries of a vector)
and the three backbone-feature gradients ([::16, ::16]); conf_matrix_pred and conf_matrix_gt_hat of the float64 run.  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.

Weights: diffreg_hip.synth.make_weights_2d3d, seed 9 for transformer / coarse_matching and seed 10 for the denoising pair (prefixes renamed;
head gain 4).  Inputs: tests/train2d3d_ref.make_batch(96, 160, 31, nv=90, mv=150) -- deterministic (integer hash + a seeded CPU generator);
a checksum of them is stored and checked by the tests.  Only reference OUTPUTS are stored.  Imports need the same stubs as
oracle/make_golden.py (open3d, cv2, ipdb, pykeops, pytorch3d, easydict, vision3d.ext are not needed on this path).
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "train2d3d_branch.npz")
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)
N, M, SEED, NV, MV = 96, 160, 31, 90, 150
STRIDE = 16


class Cfg(dict):
    """config object readable as cfg.a.b and cfg['a']"""
    def __getattr__(self, k):
        return self[k]


def sub(g):
    return (g[::STRIDE, ::STRIDE] if g.dim() == 2 else g).detach().numpy().copy()


def main(ref_root):
    import torch
    for m in ("vision3d.ext", "ipdb", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops"):
        sys.modules[m] = MagicMock()
    torch.Tensor.cuda = lambda self, *a, **k: self
    tree = os.path.join(ref_root, "Diff-Reg-2d3d")
    exp = os.path.join(tree, "experiments", "2d3dmatr.rgbdv2.stage4.level3.stage1")
    sys.path.insert(0, tree)
    sys.path.insert(0, exp)
    cwd = os.getcwd()
    os.chdir(exp)
    from fusion_module import CrossModalFusionModule
    from matching import Matching
    from loss import CoarseMatchingLoss
    os.chdir(cwd)
    from diffreg_hip import synth
    from tests.train2d3d_ref import make_batch, input_checksum
    torch.set_num_threads(8)
    v = synth.VARIANTS["2d3d"]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    mcfg = Cfg(feature_dim=v["C"], confidence_threshold=0.2, entangled=False, dsmax_temperature=0.1, match_type="sinkhorn",
               skh_init_bin_score=1.0, skh_iters=3, skh_prefilter=False)
    lcfg = Cfg(loss=Cfg(coarse_loss=Cfg(positive_margin=0.1, negative_margin=1.4, positive_optimal=0.1, negative_optimal=1.4, log_scale=40,
                                        positive_overlap=0.3, negative_overlap=0.2, weight=1.0)))   # EXP/config.py:155-163
    mods = {}
    for seed, (tp, mp) in zip((9, 10), (("transformer", "coarse_matching"), ("denoising_transformer", "denoising_coarse_matching"))):
        W = synth.make_weights_2d3d(seed=seed, head_gain=4.0)
        fus = CrossModalFusionModule(v["img_dim"], v["pcd_dim"], v["C"], v["C"], v["H"], ["self", "cross"] * 3, use_embedding=True)
        fus.load_state_dict({k[len("denoising_transformer."):]: T(a) for k, a in W.items() if k.startswith("denoising_transformer.")})
        head = Matching(mcfg)
        head.load_state_dict({k[len("denoising_coarse_matching."):]: T(a) for k, a in W.items() if k.startswith("denoising_coarse_matching.")})
        mods[tp], mods[mp] = fus.train(), head.train()
    b0 = make_batch(N, M, SEED, nv=NV, mv=MV)
    res = dict(input_checksum=input_checksum(b0))
    for tag, dt in (("32", torch.float32), ("64", torch.float64)):
        ms = {k: m.to(dt) for k, m in mods.items()}
        for m in ms.values():
            m.zero_grad(set_to_none=True)
        b = {k: (x.to(dt) if x.is_floating_point() else x) for k, x in b0.items()}
        for k in ("img_feats", "img_dino", "pcd_feats"):
            b[k] = b[k].clone().requires_grad_(True)
        sm, tm = b["src_mask"], b["tgt_mask"]
        img_c, pcd_c = ms["transformer"](b["img_feats"][None], b["img_dino"][None], b["img_pixels"][None], b["pcd_feats"][None], b["pcd_points"][None])
        img_c, pcd_c = img_c[0], pcd_c[0]
        conf_pred = ms["coarse_matching"](pcd_c[None], img_c[None], sm, tm, True)[0]
        img_d, pcd_d = ms["denoising_transformer"](b["img_feats"][None], b["img_dino"][None], b["img_pixels"][None], b["pcd_feats"][None],
                                                   b["warped"][None])
        conf_hat = ms["denoising_coarse_matching"](pcd_d, img_d, sm, tm, True)[0]
        F = torch.nn.functional
        od = dict(img_feats_c=F.normalize(img_c, p=2, dim=1), pcd_feats_c=F.normalize(pcd_c, p=2, dim=1), conf_matrix_pred=conf_pred,
                  img_feats_c_denoising=F.normalize(img_d[0], p=2, dim=1), pcd_feats_c_denoising=F.normalize(pcd_d[0], p=2, dim=1),
                  conf_matrix_gt_hat=conf_hat, src_mask=sm, tgt_mask=tm, matrix_gt=b["matrix_gt"], gt_img_node_corr_indices=b["gt_img"],
                  gt_pcd_node_corr_indices=b["gt_pcd"], gt_node_corr_min_overlaps=b["gt_ov"])
        losses = CoarseMatchingLoss(lcfg)(od)
        (losses[0] + losses[3]).backward()
        res["losses" + tag] = np.array([float(l.detach()) for l in losses])
        if tag == "64":      # (stored as float32: the tests hold the device's conf matrices to 1e-4 of the float64 run)
            res["conf_pred64"] = conf_pred[0].detach().float().numpy()
            res["conf_gt_hat64"] = conf_hat[0].detach().float().numpy()
        n = 0
        for mk, m in ms.items():
            for k, p in m.named_parameters():
                if p.grad is not None:
                    res["g%s_%s.%s" % (tag, mk, k)] = sub(p.grad)
                    n += 1
        for k in ("img_feats", "img_dino", "pcd_feats"):
            res["g%s_input.%s" % (tag, k)] = sub(b[k].grad)
        print("dtype", tag, "losses", res["losses" + tag], "parameter gradients", n)
    worst = max(float(np.abs(res[k].astype(np.float64) - res[k.replace("g32_", "g64_")]).max() / max(np.abs(res[k.replace("g32_", "g64_")]).max(), 1e-30))
                for k in res if k.startswith("g32_"))
    print("largest |g32 - g64| / max|g64| over the gradient tensors: %.3e" % worst)
    np.savez_compressed(OUT, **res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(res), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
