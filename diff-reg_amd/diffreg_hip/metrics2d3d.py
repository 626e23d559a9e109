"""The evaluation metrics of the 2D-3D model on the HIP kernels (csrc/eval2d3d.hip, ABI 0.7.0).

Same names and arguments as the two consumers of MATR2D3D.forward's output dict in the reference
(EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1):

    EvalFunction                                                                 EXP/loss.py:241-301      (after every training / test step)
    evaluate_sparse_correspondences, evaluate_correspondences                    vision3d/array_ops/registration_utils.py:151-225
    registration_rmse, isotropic_registration_error                              vision3d/array_ops/metrics.py:25-121
    evaluate_pair / summarize                                                    EXP/eval.py:86-200 / :205-330 (the offline evaluator)

so that the two imports named in INTEGRATION.md section C are the only edits.  Everything runs on the device through libdiffreg_hip.so
(dr_sparse_corr_eval_i64, dr_corr_eval_f32, dr_registration_eval_f64, dr_pnp_ransac_f64); there is no CPU path and no scipy / OpenCV dependency.
The four array functions take numpy arrays (-> Python floats, as the reference's numpy scalars; one device round trip) or device tensors
(-> 0-d float64 device tensors, no synchronisation).  An index outside its range is skipped and reported by lib.device_status() (the
reference raises an IndexError there)."""
import numpy as np
import torch

from . import lib

DEVICE = "cuda:0"          # where numpy inputs are evaluated


def _dev(x, like=None):
    """-> (device tensor, came from the host)"""
    if torch.is_tensor(x) and x.is_cuda:
        return x, False
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(DEVICE if like is None else like), True


def _ret(d, host):
    return {k: float(v) for k, v in d.items()} if host else d


def evaluate_sparse_correspondences(src_length, tgt_length, src_corr_indices, tgt_corr_indices, gt_src_corr_indices, gt_tgt_corr_indices):
    """-> {"precision", "recall", "hit_ratio"} (duplicates count once; registration_utils.py:202-225)"""
    si, host = _dev(src_corr_indices)
    args = [_dev(a, si.device)[0] for a in (tgt_corr_indices, gt_src_corr_indices, gt_tgt_corr_indices)]
    out, _ = lib.sparse_corr_eval(int(src_length), int(tgt_length), si, *args)
    return _ret({"precision": out[1], "recall": out[2], "hit_ratio": out[3]}, host)


def evaluate_correspondences(src_corr_points, tgt_corr_points, transform, positive_radius=0.1):
    """src = cloud, tgt = image points (eval.py:153-155) -> {"overlap", "inlier_ratio", "distance"}; no correspondences -> zeros (eval.py:157)"""
    src, host = _dev(src_corr_points)
    tgt, T = _dev(tgt_corr_points, src.device)[0], _dev(transform, src.device)[0]
    out, _ = lib.corr_eval(src, tgt, T, positive_radius)
    return _ret({"overlap": out[2], "inlier_ratio": out[0], "distance": out[1]}, host)


def registration_rmse(src_points, gt_transform, est_transform):
    """sqrt(mean |T_gt p - T_est p|^2)   (array_ops/metrics.py:102-121)"""
    p, host = _dev(src_points)
    out, _ = lib.registration_eval(p, _dev(gt_transform, p.device)[0], _dev(est_transform, p.device)[0], 0.0)
    return float(out[0]) if host else out[0]


def isotropic_registration_error(gt_transform, est_transform):
    """-> (rre in degrees, rte)   (array_ops/metrics.py:59-74)"""
    G, host = _dev(gt_transform)
    out, _ = lib.registration_eval(None, G, _dev(est_transform, G.device)[0], 0.0)
    return (float(out[2]), float(out[3])) if host else (out[2], out[3])


class EvalFunction(torch.nn.Module):
    """EXP/loss.py:241-301 on the device: forward(data_dict, output_dict) -> {"PIR", "IR"} as 0-d device tensors (float64: the kernels sum in
    double; the reference's are float32 means of the same counts), no dense img_num_nodes x pcd_num_nodes matrix, no synchronisation."""

    def __init__(self, cfg):
        super().__init__()
        self.acceptance_overlap = cfg.eval.acceptance_overlap
        self.acceptance_radius = cfg.eval.acceptance_radius
        self.acceptance_rmse = cfg.eval.rmse_threshold

    @torch.no_grad()
    def evaluate_coarse_matching(self, output_dict):
        o = output_dict
        out, _ = lib.sparse_corr_eval(int(o["img_num_nodes"]), int(o["pcd_num_nodes"]), o["img_node_corr_indices"], o["pcd_node_corr_indices"],
                                      o["gt_img_node_corr_indices"], o["gt_pcd_node_corr_indices"], o["gt_node_corr_min_overlaps"],
                                      self.acceptance_overlap)
        return out[0]

    @torch.no_grad()
    def evaluate_fine_matching(self, data_dict, output_dict):
        out, _ = lib.corr_eval(output_dict["pcd_corr_points"], output_dict["img_corr_points"], data_dict["transform"], self.acceptance_radius,
                               depth_mask=True)
        return out[3]

    @torch.no_grad()
    def evaluate_registration(self, data_dict, output_dict):
        """-> (rre, rte, rmse, recall) with rmse = mean |inv(T_gt) T_est p - p|"""
        out, rec = lib.registration_eval(output_dict["pcd_points"], data_dict["transform"], output_dict["estimated_transform"], self.acceptance_rmse)
        return out[2], out[3], out[1], rec[1].to(torch.float64)

    def forward(self, data_dict, output_dict):
        return {"PIR": self.evaluate_coarse_matching(output_dict), "IR": self.evaluate_fine_matching(data_dict, output_dict)}


# the fixed layout of evaluate_pair's metric vector: per-pair terms that are summed over pairs and, by one all_reduce, over ranks.  The first five
# slots are shard.METRIC_NAMES, so shard.reduce_metrics reads IR, FMR, RR and the pair count there -- and ONLY those: it names five slots.
# reduce_pair_metrics below names all fifteen.  RRE / RTE enter only where the pair is recalled (eval.py:190-193)
VECTOR_NAMES = ("sum_inlier_ratio", "sum_fmr", "sum_registration_recall", "n_pairs", "sum_seconds", "sum_PIR", "sum_PMR>0", "sum_PMR>=0.1",
                "sum_PMR>=0.3", "sum_PMR>=0.5", "sum_overlap", "sum_residual", "sum_RRE_recalled", "sum_RTE_recalled", "sum_num_correspondences")


def reduce_pair_metrics(local_vec):
    """The one collective of a sharded 2D-3D evaluation: all_reduce(SUM) of this rank's summed evaluate_pair vectors (shard.gather_metrics) -> dict
    with every sum under its VECTOR_NAMES name and the means over ALL pairs: PIR, the PMR fractions, IR, FMR, OR, residual, RR, and RRE / RTE over the
    recalled pairs (NaN without one).  These are pair means; eval.py's table averages scene means (summarize)."""
    from . import shard
    g = shard.gather_metrics(local_vec, local_vec.device if torch.is_tensor(local_vec) else None).tolist()
    d = dict(zip(VECTOR_NAMES, g))
    n, nr = max(d["n_pairs"], 1.0), d["sum_registration_recall"]
    d.update({"IR": d["sum_inlier_ratio"] / n, "FMR": d["sum_fmr"] / n, "RR": nr / n, "PIR": d["sum_PIR"] / n, "OR": d["sum_overlap"] / n,
              "residual": d["sum_residual"] / n, "mean_RRE": d["sum_RRE_recalled"] / nr if nr > 0 else float("nan"),
              "mean_RTE": d["sum_RTE_recalled"] / nr if nr > 0 else float("nan")})
    d.update({k: d["sum_" + k] / n for k in ("PMR>0", "PMR>=0.1", "PMR>=0.3", "PMR>=0.5")})
    return d


def evaluate_pair(data, cfg, num_corr=2048, seed=0, estimated_transform=None):
    """eval.py:86-200 for one pair: `data` holds the keys of the evaluator's .npz (numpy or device tensors; `intrinsics` a HOST 3 x 3 array -- PnP takes
    it as a host argument, a device tensor is read back first, which synchronises).  The num_corr best correspondences by corr_scores; PIR and the
    four PMR flags; IR, OR, residual, FMR; with at least 4 correspondences PnP-RANSAC (lib.pnp_ransac, seeded), RMSE and RR, RRE and RTE.
    estimated_transform (4 x 4, optional): a pose the caller already has; it is evaluated in place of PnP's.  -> dict of device tensors (0-d float64;
    "estimated_transform" [4,4] or None; "num_correspondences" an int) and "vector" (float64 [len(VECTOR_NAMES)]).  With device-resident inputs and
    host intrinsics nothing is read back: the registration recall stays a device flag, so RRE / RTE are always returned and enter the vector
    multiplied by it."""
    g = lambda k: _dev(data[k])[0]
    f64 = lambda x: x.to(torch.float64)
    sp, _ = lib.sparse_corr_eval(int(data["img_num_nodes"]), int(data["pcd_num_nodes"]), g("img_node_corr_indices"), g("pcd_node_corr_indices"),
                                 g("gt_img_node_corr_indices"), g("gt_pcd_node_corr_indices"))
    pir = sp[1]
    pcd_c, img_c, T = g("pcd_corr_points"), g("img_corr_points"), g("transform")
    scores = g("corr_scores")
    n = scores.shape[0]
    sel = None
    if num_corr is not None and n > num_corr:
        sel = torch.sort(scores, descending=True, stable=True).indices[:num_corr]       # np.argsort(-corr_scores)[:num_corr]
        n = num_corr
    fine, _ = lib.corr_eval(pcd_c, img_c, T, cfg.eval.acceptance_radius, sel_indices=sel)
    ir, resid, ovl = fine[0], fine[1], fine[2]
    dev = fine.device
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    est, rmse, rr, rre, rte = None, None, zero, zero, zero
    if n >= 4:
        if estimated_transform is not None:
            est = _dev(estimated_transform, dev)[0].to(torch.float64)
        else:
            pix = g("img_corr_pixels")
            pts = pcd_c if sel is None else pcd_c[sel]
            pix = pix if sel is None else pix[sel]
            K = data["intrinsics"]
            K = K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)
            est = lib.pnp_ransac(pts, pix, K, num_iterations=cfg.ransac.num_iterations, distance_tolerance=cfg.ransac.distance_tolerance,
                                 seed=seed)["transform"]
        reg, rec = lib.registration_eval(g("pcd_points"), T, est, cfg.eval.rmse_threshold)
        rmse, rr, rre, rte = reg[0], f64(rec[0]), reg[2], reg[3]
    fmr = f64(ir >= cfg.eval.inlier_ratio_threshold)
    one = torch.ones((), dtype=torch.float64, device=dev)
    out = {"PIR": pir, "PMR>0": f64(pir > 0), "PMR>=0.1": f64(pir >= 0.1), "PMR>=0.3": f64(pir >= 0.3), "PMR>=0.5": f64(pir >= 0.5),
           "recall": sp[2], "hit_ratio": sp[3], "IR": ir, "OR": ovl, "residual": resid, "FMR": fmr, "num_correspondences": n,
           "estimated_transform": est, "RMSE": rmse, "RR": rr, "RRE": rre, "RTE": rte}
    out["vector"] = torch.stack([ir, fmr, rr, one, zero, pir, out["PMR>0"], out["PMR>=0.1"], out["PMR>=0.3"], out["PMR>=0.5"], ovl, resid,
                                 rre * rr, rte * rr, one * n])
    return out


_COARSE = ("PIR", "PMR>0", "PMR>=0.1", "PMR>=0.3", "PMR>=0.5")


def summarize(per_scene_results, inlier_ratio_threshold=0.1):
    """eval.py:205-330 on the host: {scene: [per-pair dicts with PIR, IR, OR, RR, RRE, RTE (floats or 0-d tensors; evaluate_pair's output fits)]} ->
    {"scenes": {scene: {...}}, and the summary.json numbers}: per scene the means over its pairs (the PMR flags from PIR, FMR from IR >= inlier_ratio_threshold;
    mean / median RRE and RTE over the pairs with RR > 0 -- NaN for a scene without one, as np.mean of nothing), then the mean of the scene values
    in sorted scene order.  One reference quirk is kept: eval.py:77 resets a meter named "scene_overlap" that does not exist, so its scene OR is
    the mean over every pair seen SO FAR, not over the scene's pairs."""
    f = lambda v: float(v)
    mean = lambda xs: float(np.mean(xs)) if len(xs) else float("nan")
    median = lambda xs: float(np.median(xs)) if len(xs) else float("nan")
    scenes, seen_or = {}, []
    for name in sorted(per_scene_results):
        rows = per_scene_results[name]
        pir = [f(r["PIR"]) for r in rows]
        ir = [f(r["IR"]) for r in rows]
        seen_or += [f(r["OR"]) for r in rows]
        rr = [f(r["RR"]) for r in rows]
        rre = [f(r["RRE"]) for r, ok in zip(rows, rr) if ok > 0.0]
        rte = [f(r["RTE"]) for r, ok in zip(rows, rr) if ok > 0.0]
        scenes[name] = {"PIR": mean(pir), "PMR>0": mean([float(c > 0) for c in pir]), "PMR>=0.1": mean([float(c >= 0.1) for c in pir]),
                        "PMR>=0.3": mean([float(c >= 0.3) for c in pir]), "PMR>=0.5": mean([float(c >= 0.5) for c in pir]),
                        "FMR": mean([float(x >= inlier_ratio_threshold) for x in ir]), "IR": mean(ir), "OR": mean(seen_or), "RR": mean(rr), "mean_RRE": mean(rre),
                        "mean_RTE": mean(rte), "median_RRE": median(rre), "median_RTE": median(rte)}
    out = {"scenes": scenes}
    for k in _COARSE + ("FMR", "IR", "OR", "RR", "mean_RRE", "mean_RTE", "median_RRE", "median_RTE"):
        out[k] = mean([s[k] for s in scenes.values()])                  # a NaN scene makes the mean NaN, as np.mean does in the reference
    out["FMR_std"] = float(np.std([s["FMR"] for s in scenes.values()])) if scenes else float("nan")
    return out
