"""Time the 2D-3D evaluation metrics on one GPU:

    python tools/eval2d3d_time.py [--out FILE.json]

Method of DESIGN 5f-5j: 5 warm-up runs, then 30 runs alternating the two sides, each between two device synchronisations; median [p10-p90] in
milliseconds.  Rows: (a) EvalFunction.forward at 1 530 x 1 024 nodes, 96 predicted node pairs, 400 ground-truth pairs and 2 048 correspondences:
the device path against the same two functions in PLAIN PyTorch on the same GPU (a dense float matrix and a scatter, as EXP/loss.py:247-278);
(b) metrics2d3d.evaluate_pair without PnP (the estimated pose is handed in on both sides; n = 2 304 correspondences cut to num_corr = 2 048,
N = 20 000 points): the public function on device-resident inputs with its vector read back once, against eval.py's per-pair body through the
numpy restatement on the host (tests/eval2d3d_ref.py, with scipy's KD-tree for the overlap when scipy is importable, as the reference) INCLUDING
the device-to-host copies of the inputs the reference pays."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


class Cfg(dict):
    def __getattr__(self, k):
        return self[k]


def measure(sides, warm=5, runs=30):
    out = {k: [] for k in sides}
    for i in range(warm + runs):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warm:
                out[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90))) for k, v in out.items()}


def torch_eval_forward(dd, od, c):
    mat = torch.zeros(od["img_num_nodes"], od["pcd_num_nodes"], device=DEV)
    keep = od["gt_node_corr_min_overlaps"] > c["acceptance_overlap"]
    mat[od["gt_img_node_corr_indices"][keep], od["gt_pcd_node_corr_indices"][keep]] = 1.0
    pir = mat[od["img_node_corr_indices"], od["pcd_node_corr_indices"]].mean()
    img, pcd, T = od["img_corr_points"], od["pcd_corr_points"], dd["transform"].float()
    m = img[:, 2] > 0
    d = torch.linalg.norm(pcd[m] @ T[:3, :3].T + T[:3, 3] - img[m], dim=1)
    return {"PIR": pir, "IR": (d < c["acceptance_radius"]).float().mean().nan_to_num_()}


def main():
    from diffreg_hip import metrics2d3d as M
    from tests import eval2d3d_ref as F
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    c = F.CFG
    cfg = Cfg(eval=Cfg(c), ransac=Cfg(num_iterations=50000, distance_tolerance=8.0))
    s = F.make_scene(img=1530, pcd=1024, K=96, dup=8, G=400, n=2048, num_corr=None, N=20000, angle=2.0, shift=0.02, nodepth=0.2, seed=9)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    od = {k: t(s[k]) for k in F.INPUT_KEYS[2:]}
    od.update(img_num_nodes=1530, pcd_num_nodes=1024)
    dd = dict(transform=od["transform"])
    ev = M.EvalFunction(cfg)
    a, b = ev(dd, od), torch_eval_forward(dd, od, c)
    assert abs(float(a["PIR"]) - float(b["PIR"])) < 1e-6 and abs(float(a["IR"]) - float(b["IR"])) < 1e-6
    res = {"eval_function_forward": measure({"torch": lambda: torch_eval_forward(dd, od, c), "device": lambda: ev(dd, od)})}

    s2 = F.make_scene(img=1530, pcd=1024, K=96, dup=8, G=400, n=2304, num_corr=2048, N=20000, angle=2.0, shift=0.02, nodepth=0.2, seed=10)
    pd = {k: t(s2[k]) for k in F.INPUT_KEYS[2:]}
    pd.update(img_num_nodes=1530, pcd_num_nodes=1024)

    def host_pair():
        h = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in pd.items()}          # the copies the reference's .npz round trip pays
        sel = np.argsort(-h["corr_scores"])[:2048]
        sp = F.evaluate_sparse_correspondences(1530, 1024, h["img_node_corr_indices"], h["pcd_node_corr_indices"], h["gt_img_node_corr_indices"],
                                               h["gt_pcd_node_corr_indices"])
        P, Q, T = h["pcd_corr_points"][sel].astype(np.float64), h["img_corr_points"][sel].astype(np.float64), h["transform"]
        moved = F.apply_transform(P, T)
        d = np.sqrt(((Q - moved) ** 2).sum(1))
        nn = cKDTree(moved).query(Q, k=1)[0] if cKDTree is not None else F._nn_dist(Q, moved)
        rmse = F.registration_rmse(h["pcd_points"], T, h["estimated_transform"])
        rre, rte = F.isotropic_registration_error(T, h["estimated_transform"])
        return sp["precision"], float((d < 0.05).mean()), float((nn < 0.05).mean()), float(d.mean()), rmse, rre, rte

    def device_pair():
        out = M.evaluate_pair(pd, cfg, num_corr=2048, estimated_transform=pd["estimated_transform"])
        return out, out["vector"].cpu().tolist()                        # the one read-back of the pair's numbers

    h, (o, v) = host_pair(), device_pair()
    g, g_rmse = dict(zip(M.VECTOR_NAMES, v)), float(o["RMSE"])
    assert abs(h[0] - g["sum_PIR"]) < 1e-9 and abs(h[1] - g["sum_inlier_ratio"]) < 1e-9 and abs(h[2] - g["sum_overlap"]) < 1e-9
    assert abs(h[3] - g["sum_residual"]) < 1e-9 and abs(h[4] - g_rmse) < 1e-9
    res["evaluate_pair_without_pnp"] = measure({"host_numpy": host_pair, "device": device_pair})
    res["kd_tree"] = cKDTree is not None
    for k, v in res.items():
        if isinstance(v, dict):
            print("%-28s" % k, "  ".join("%s %.3f [%.3f-%.3f] ms" % (s_, r["median"], r["p10"], r["p90"]) for s_, r in v.items()))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
