"""Mint the 2D-3D evaluation fixture by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_eval2d3d.py REFERENCE_ROOT    # the directory holding Diff-Reg-2d3d/; writes tests/golden/eval2d3d.npz

The reference's own vision3d.array_ops functions (evaluate_sparse_correspondences, evaluate_correspondences with its scipy KD-tree,
registration_rmse, isotropic_registration_error) and EXP/loss.py::EvalFunction (`.cuda()` made a no-op) run on the deterministic scenes of
tests/eval2d3d_ref.py in float32 and in float64 (inputs cast; torch's default dtype switched for the float64 run, so that the matrix
evaluate_coarse_matching allocates is float64 too.  evaluate_fine_matching casts its mask with `.float()` whatever the inputs are: its IR is a
float32 mean in BOTH runs -- the counts behind it are stored beside it, from the restatement, after asserting that they reproduce the
reference's float32 value bit for bit).  vision3d.utils.summary_board.SummaryBoard replays eval.py:27-330's updates on the three-scene table of
eval2d3d_ref.make_table.  EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.

Stored: the inputs of every scene, per dtype tag 32 / 64 every real-valued output, the integer counts, and the summary of the table.  The fixture
rules (eval2d3d_ref.fixture_rules) are asserted here: a scene that breaks one is no fixture.  Stubs as tools/golden/make_golden_finenoise2d3d.py.
"""
import os
import sys
import warnings
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "eval2d3d.npz")
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)


class Cfg(dict):
    def __getattr__(self, k):
        return self[k]


def replay_summary(SummaryBoard, table, ir_thr):
    """eval.py:27-330 on a table of per-pair results: the same meters, the same resets (the one of "scene_overlap" names no meter, so scene_OR
    is never reset), the same updates"""
    cm, fm, rm = SummaryBoard(), SummaryBoard(), SummaryBoard()
    for k in ("PIR", "PMR>0", "PMR>=0.1", "PMR>=0.3", "PMR>=0.5"):
        cm.register_meter(k)
    for k in ("PIR", "PMR>0", "PMR>=0.1", "PMR>=0.3", "PMR>=0.5"):
        cm.register_meter("scene_" + k)
    for k in ("FMR", "IR", "OR", "scene_FMR", "scene_IR", "scene_OR"):
        fm.register_meter(k)
    for k in ("RR", "mean_RRE", "mean_RTE", "median_RRE", "median_RTE", "scene_RR", "scene_RRE", "scene_RTE"):
        rm.register_meter(k)
    for scene in sorted(table):
        for k in ("PIR", "PMR>0", "PMR>=0.1", "PMR>=0.3", "PMR>=0.5"):
            cm.reset_meter("scene_" + k)
        fm.reset_meter("scene_FMR"); fm.reset_meter("scene_IR"); fm.reset_meter("scene_overlap")
        rm.reset_meter("scene_RR"); rm.reset_meter("scene_RRE"); rm.reset_meter("scene_RTE")
        for p in table[scene]:
            c = p["PIR"]
            cm.update("scene_PIR", c)
            cm.update("scene_PMR>0", float(c > 0)); cm.update("scene_PMR>=0.1", float(c >= 0.1))
            cm.update("scene_PMR>=0.3", float(c >= 0.3)); cm.update("scene_PMR>=0.5", float(c >= 0.5))
            fm.update("scene_IR", p["IR"]); fm.update("scene_OR", p["OR"]); fm.update("scene_FMR", float(p["IR"] >= ir_thr))
            rm.update("scene_RR", p["RR"])
            if p["RR"] > 0.0:
                rm.update("scene_RRE", p["RRE"]); rm.update("scene_RTE", p["RTE"])
        for k in ("PIR", "PMR>0", "PMR>=0.1", "PMR>=0.3", "PMR>=0.5"):
            cm.update(k, cm.mean("scene_" + k))
        fm.update("FMR", fm.mean("scene_FMR")); fm.update("IR", fm.mean("scene_IR")); fm.update("OR", fm.mean("scene_OR"))
        rm.update("RR", rm.mean("scene_RR"))
        rm.update("mean_RRE", rm.mean("scene_RRE")); rm.update("mean_RTE", rm.mean("scene_RTE"))
        rm.update("median_RRE", rm.median("scene_RRE")); rm.update("median_RTE", rm.median("scene_RTE"))
    out = {k: cm.mean(k) for k in ("PIR", "PMR>0", "PMR>=0.1", "PMR>=0.3", "PMR>=0.5")}
    out.update({k: fm.mean(k) for k in ("FMR", "IR", "OR")})
    out["FMR_std"] = fm.std("FMR")
    out.update({k: rm.mean(k) for k in ("RR", "mean_RRE", "mean_RTE", "median_RRE", "median_RTE")})
    return out


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
    while True:                                                             # stub whichever optional dependency is absent
        try:
            from loss import EvalFunction
            from vision3d.array_ops import (evaluate_correspondences, evaluate_sparse_correspondences, isotropic_registration_error,
                                            registration_rmse)
            from vision3d.utils.summary_board import SummaryBoard
            break
        except ModuleNotFoundError as e:
            sys.modules[e.name] = MagicMock()
    os.chdir(cwd)
    from tests import eval2d3d_ref as F
    c = F.CFG
    ev = EvalFunction(Cfg(eval=Cfg(acceptance_overlap=c["acceptance_overlap"], acceptance_radius=c["acceptance_radius"],
                                   rmse_threshold=c["rmse_threshold"])))
    res = {}
    warnings.simplefilter("ignore")                                         # means of nothing
    for name, kw in F.SCENES.items():
        s = F.make_scene(**kw)
        bad = F.fixture_rules(s)
        assert not bad, (name, bad)
        for k in F.INPUT_KEYS:
            res["%s_in_%s" % (name, k)] = np.asarray(s[k])
        res["%s_in_num_corr" % name] = np.int64(-1 if s["num_corr"] is None else s["num_corr"])
        sel = F.selection(s)
        want = {tag: F.restate(s, dt) for tag, dt in (("32", np.float32), ("64", np.float64))}
        for tag, npdt, tdt in (("32", np.float32, torch.float32), ("64", np.float64, torch.float64)):
            o = {}
            sp = evaluate_sparse_correspondences(int(s["img_num_nodes"]), int(s["pcd_num_nodes"]), s["img_node_corr_indices"],
                                                 s["pcd_node_corr_indices"], s["gt_img_node_corr_indices"], s["gt_pcd_node_corr_indices"])
            o["sp_precision"], o["sp_recall"], o["sp_hit_ratio"] = sp["precision"], sp["recall"], sp["hit_ratio"]
            P, Q = s["pcd_corr_points"].astype(npdt), s["img_corr_points"].astype(npdt)
            if sel is not None:
                P, Q = P[sel], Q[sel]
            if P.shape[0] > 0:                                              # eval.py:153-158
                ec = evaluate_correspondences(P, Q, s["transform"].astype(npdt), positive_radius=c["acceptance_radius"])
            else:
                ec = {"inlier_ratio": 0.0, "overlap": 0.0, "distance": 0.0}
            o["ec_overlap"], o["ec_inlier_ratio"], o["ec_distance"] = ec["overlap"], ec["inlier_ratio"], ec["distance"]
            G, E = s["transform"].astype(npdt), s["estimated_transform"].astype(npdt)
            o["rmse"] = registration_rmse(s["pcd_points"].astype(npdt), G, E)
            o["rre"], o["rte"] = isotropic_registration_error(G, E)
            t = lambda a: torch.from_numpy(np.asarray(a))
            torch.set_default_dtype(tdt)
            try:
                dd = dict(transform=t(G))
                od = dict(img_num_nodes=int(s["img_num_nodes"]), pcd_num_nodes=int(s["pcd_num_nodes"]),
                          gt_node_corr_min_overlaps=t(s["gt_node_corr_min_overlaps"].astype(npdt)),
                          gt_img_node_corr_indices=t(s["gt_img_node_corr_indices"]), gt_pcd_node_corr_indices=t(s["gt_pcd_node_corr_indices"]),
                          img_node_corr_indices=t(s["img_node_corr_indices"]), pcd_node_corr_indices=t(s["pcd_node_corr_indices"]),
                          img_corr_points=t(s["img_corr_points"].astype(npdt)), pcd_corr_points=t(s["pcd_corr_points"].astype(npdt)),
                          estimated_transform=t(E), pcd_points=t(s["pcd_points"].astype(npdt)))
                r = ev(dd, od)
                o["ev_PIR"], o["ev_IR"] = float(r["PIR"]), float(r["IR"])
                rre, rte, rmse, recall = ev.evaluate_registration(dd, od)
                o["ev_rre"], o["ev_rte"], o["ev_rmse"], o["ev_recall"] = float(rre), float(rte), float(rmse), int(recall)
                assert r["IR"].dtype == torch.float32                       # `.float()` in either run
            finally:
                torch.set_default_dtype(torch.float32)
            w = want[tag]
            # the reference exposes no integer count: the restatement's are stored, after they reproduce every ratio the reference returns
            assert o["ev_recall"] == w["ev_recall"] and int(o["rmse"] < c["rmse_threshold"]) == w["rr"], (name, tag)
            assert np.float32(o["ev_IR"]) == np.float32(w["n_kept_inlier"] / w["n_kept"] if w["n_kept"] else 0.0), (name, tag, "EvalFunction IR")
            if P.shape[0] > 0:
                assert abs(o["ec_inlier_ratio"] - w["n_inlier"] / P.shape[0]) < 1e-12 and abs(o["ec_overlap"] - w["n_overlap"] / P.shape[0]) < 1e-12
            assert abs(o["sp_precision"] - w["n_pos"] / (w["n_pred"] + 1e-12)) < 1e-12 and abs(o["sp_recall"] - w["n_pos"] / (w["n_gt"] + 1e-12)) < 1e-12
            K = s["img_node_corr_indices"].shape[0]
            if K:
                assert abs(o["ev_PIR"] - w["n_listed_pos"] / K) < 1e-6, (name, tag, "EvalFunction PIR")
            for k in F.REAL_KEYS:
                res["%s_%s%s" % (name, k, tag)] = np.float64(o[k])
            print(name, tag, {k: float("%.6g" % o[k]) for k in F.REAL_KEYS})
        for k in F.INT_KEYS:                                                # fixture_rules asserted them equal between the two runs
            res["%s_%s" % (name, k)] = np.int64(want["64"][k])
    table = F.make_table()
    for k, v in replay_summary(SummaryBoard, table, c["inlier_ratio_threshold"]).items():
        res["summary_%s" % k] = np.float64(v)
    np.savez_compressed(OUT, **res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(res), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
