"""Mint the fine-loss / noising fixture by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_finenoise2d3d.py REFERENCE_ROOT    # the directory holding Diff-Reg-2d3d/; writes tests/golden/finenoise2d3d.npz

The reference's own FineMatchingLoss (EXP/loss.py, with vision3d's CircleLoss, pairwise_distance, apply_transform, random_choice),
SoftProcrustesLayer (EXP/procrustes.py), log_optimal_transport (EXP/matching.py) and q_sample (EXP/model.py) run on the deterministic scenes of
tests/finenoise2d3d_ref.py.  get_warped_from_noising_matching3D3D is called UNBOUND on a small object carrying the two modules it reads
(denoising_coarse_matching: bin_score, skh_iters; denoising_soft_procrustes).  float32 and float64 runs, the reference's own `.float()` /
`.type(torch.float32)` casts kept (in the warp's float64 run the scores and bin_score are float64, the points float32: its casts allow no other).  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.

Stored (outputs only), per dtype tag 32 / 64: fine loss, recall and the gradient ROWS of the selected features (every 4th channel) per fine case; R, t, R_forwd,
t_forwd, condition, mask of a ladder (0 / 1) matrix and of the warp per warp case, the warped points, d(sum <warped, w>) / d bin_score and
d / d scores; q_sample at three t.  The fixture rules (tests/finenoise2d3d_ref.fixture_rules, topk_rule) are asserted here: a scene that breaks
one is no fixture.  Stubs as tools/golden/make_golden_train2d3d.py.
"""
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "finenoise2d3d.npz")
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)


class Cfg(dict):
    def __getattr__(self, k):
        return self[k]


def main(ref_root):
    import torch
    for m in ("vision3d.ext", "ipdb", "IPython", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops"):
        sys.modules[m] = MagicMock()
    torch.Tensor.cuda = lambda self, *a, **k: self
    tree = os.path.join(ref_root, "Diff-Reg-2d3d")
    exp = os.path.join(tree, "experiments", "2d3dmatr.rgbdv2.stage4.level3.stage1")
    sys.path.insert(0, tree)
    sys.path.insert(0, exp)
    cwd = os.getcwd()
    os.chdir(exp)
    from loss import FineMatchingLoss
    from procrustes import SoftProcrustesLayer
    from matching import log_optimal_transport  # noqa: F401  (model.py's warp reads it from its own globals)
    while True:                                                             # model.py imports the backbones' dependencies: stub whichever is absent
        try:
            import model as ref_model
            break
        except ModuleNotFoundError as e:
            sys.modules[e.name] = MagicMock()
    os.chdir(cwd)
    from tests import finenoise2d3d_ref as F
    torch.set_num_threads(8)
    c = F.FINE_CFG
    lcfg = Cfg(loss=Cfg(fine_loss=Cfg(max_correspondences=c["max_correspondences"], positive_radius_3d=c["pos_radius_3d"],
                                      negative_radius_3d=c["neg_radius_3d"], positive_radius_2d=c["pos_radius_2d"],
                                      negative_radius_2d=c["neg_radius_2d"], positive_margin=c["pos_margin"], negative_margin=c["neg_margin"],
                                      positive_optimal=c["pos_optimal"], negative_optimal=c["neg_optimal"], log_scale=c["log_scale"])))
    floss = FineMatchingLoss(lcfg)
    res = {}
    for name, kw in F.FINE_CASES.items():
        sc = F.make_fine_scene(**kw)
        px, idx = F.select(sc)
        bad = F.fixture_rules(sc, px, idx)
        assert not bad, (name, bad)
        rows_i, rows_p = px[:, 0] * sc["image_w"] + px[:, 1], idx
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            f = lambda k: sc[k].to(dt)
            fi, fp = f("img_feats").clone().requires_grad_(True), f("pcd_feats").clone().requires_grad_(True)
            dd = dict(batch_size=1, transform=f("transform"), img_corr_pixels=sc["img_corr_pixels"], pcd_corr_indices=sc["pcd_corr_indices"],
                      image_w=sc["image_w"])
            od = dict(img_points_f=f("img_points"), img_feats_f=fi, pcd_points_f=f("pcd_points"), pcd_pixels_f=f("pcd_pixels"), pcd_feats_f=fp)
            np.random.seed(0)                                               # F.select's seed: the reference draws the same sub-sample
            loss, recall = floss(dd, od)
            if torch.isfinite(loss):
                loss.backward()
            gi = fi.grad if fi.grad is not None else torch.zeros_like(fi)
            gp = fp.grad if fp.grad is not None else torch.zeros_like(fp)
            touched = torch.zeros(gi.shape[0], dtype=torch.bool); touched[rows_i] = True
            assert float(gi[~touched].abs().max()) == 0.0
            res["fine_%s_loss%s" % (name, tag)] = np.array(float(loss.detach()))
            res["fine_%s_recall%s" % (name, tag)] = np.array(float(recall))
            res["fine_%s_gimg%s" % (name, tag)] = gi[rows_i][:, ::F.GRAD_COL_STRIDE].detach().numpy().astype(np.float32 if tag == "32" else np.float64)
            res["fine_%s_gpcd%s" % (name, tag)] = gp[rows_p][:, ::F.GRAD_COL_STRIDE].detach().numpy().astype(np.float32 if tag == "32" else np.float64)
            print("fine", name, tag, "M", px.shape[0], "loss", float(loss.detach()), "recall", float(recall))
    hp = F.WARP_HP
    proc = SoftProcrustesLayer(Cfg(sample_rate=hp["sample_rate"], max_condition_num=hp["max_cond"]))
    sets = {}
    for name, kw in F.WARP_CASES.items():
        wc = F.make_warp_case(**kw)
        sm, tm = wc["src_mask"], wc["tgt_mask"]
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            # the warp casts conf, R_forwd and t_forwd to float32 (EXP/model.py:841-843), so the points are float32 in both runs; the float64 run
            # has float64 scores and bin_score -- the Sinkhorn of a training step, whose scores q_sample makes float64
            f = lambda k: wc[k].to(dt if k == "scores" else torch.float32)
            with torch.no_grad():                                           # a ladder rung (EXP/model.py:583): the fit on the 0 / 1 matrix
                lad = proc(wc["matrix_gt"].clone(), f("s_pcd"), f("t_pcd"), sm, tm)
            for k, v in zip(("R", "t", "R_forwd", "t_forwd", "condition", "mask"), lad):
                res["ladder_%s_%s%s" % (name, k, tag)] = v.detach().cpu().numpy()
            head = types.SimpleNamespace(bin_score=torch.tensor(hp["bin_score"], dtype=dt, requires_grad=True), skh_iters=hp["iters"])
            conf_seen = {}
            def spy(conf, *a, _p=proc):
                conf_seen["conf"] = conf.detach().clone()
                out = _p(conf, *a)
                conf_seen["out"] = out
                return out
            host = types.SimpleNamespace(denoising_coarse_matching=head, denoising_soft_procrustes=spy)
            x = f("scores").clone().requires_grad_(True)
            xin = x * 1.0                                                   # (the warp fills its argument in place: a leaf cannot be)
            warped, _, Rf, tf = ref_model.MATR2D3D.get_warped_from_noising_matching3D3D(host, f("s_pcd"), f("t_pcd"), sm, tm, xin)
            (warped * f("w")).sum().backward()
            ok, sel = F.topk_rule(conf_seen["conf"].double(), sm, tm, hp["sample_rate"])
            assert ok, (name, tag, "K-th and (K+1)-th confidences within 1e-6")
            sets[(name, tag)] = sel
            for k, v in zip(("R", "t", "R_forwd", "t_forwd", "condition", "mask"), conf_seen["out"]):
                res["warp_%s_%s%s" % (name, k, tag)] = v.detach().cpu().numpy()
            res["warp_%s_warped%s" % (name, tag)] = warped.detach().numpy()
            z = lambda g, like: torch.zeros_like(like) if g is None else g
            res["warp_%s_gbin%s" % (name, tag)] = z(head.bin_score.grad, head.bin_score).numpy()
            res["warp_%s_gscores%s" % (name, tag)] = z(x.grad, x).numpy().astype(np.float32)
            print("warp", name, tag, "condition", float(conf_seen["out"][4][0]), "mask", bool(conf_seen["out"][5][0]), "g_bin", float(res["warp_%s_gbin%s" % (name, tag)]))
        assert sets[(name, "32")] == sets[(name, "64")], (name, "float32 and float64 select different sets")
    g = F._gauss((1, 24, 40), 21)
    x0 = (torch.from_numpy(F._hash01(np.arange(24 * 40), 22).reshape(1, 24, 40)) > 0.9).float()
    for t in (0, 417, 999):
        res["qsample_t%d" % t] = ref_model.q_sample(x_start=x0, t=torch.tensor([t]), noise=torch.from_numpy(g).float(), timesteps=1000).numpy()
    np.savez_compressed(OUT, **res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(res), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
