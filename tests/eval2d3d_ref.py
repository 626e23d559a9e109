"""Deterministic scenes and a numpy float64 RESTATEMENT of the 2D-3D evaluation metrics (csrc/eval2d3d.hip, diffreg_hip/metrics2d3d.py):

    evaluate_sparse_correspondences, evaluate_correspondences, registration_rmse,      vision3d/array_ops/registration_utils.py:151-225,
    isotropic_registration_error                                                       vision3d/array_ops/metrics.py:25-166
    EvalFunction.evaluate_coarse_matching / evaluate_fine_matching / evaluate_registration    EXP/loss.py:247-294

written from their definitions (sets of pairs instead of dense matrices, an exhaustive nearest-neighbour search instead of a KD-tree), pinned to the
reference's own outputs by tests/test_eval2d3d_oracle.py through tests/golden/eval2d3d.npz (minted by tools/golden/make_golden_eval2d3d.py).
`mutant=` selects one of the value-only mutants the GPU tests show their bars to reject.  No reference code is imported here."""
import numpy as np

CFG = dict(acceptance_overlap=0.3, acceptance_radius=0.05, inlier_ratio_threshold=0.1, rmse_threshold=0.1)     # EXP/config.py:52-56

# name -> scene parameters.  angle: rotation error of the estimate in degrees ("clip0": estimate == ground truth with a rotation block scaled
# by 1 + 1e-6, so (trace - 1) / 2 > 1 in either precision and the upper clip decides: RRE exactly 0; "clip180": the same times diag(1, -1, -1):
# (trace - 1) / 2 < -1, the lower clip, RRE exactly 180)
SCENES = {
    "base": dict(img=40, pcd=70, K=30, dup=6, G=50, n=300, num_corr=None, N=400, angle=3.0, shift=0.02, nodepth=0.2, seed=1),
    "topk": dict(img=24, pcd=33, K=12, dup=0, G=20, n=300, num_corr=128, N=257, angle=20.0, shift=0.3, nodepth=0.1, seed=2),
    "clip0": dict(img=8, pcd=8, K=1, dup=0, G=3, n=5, num_corr=None, N=64, angle="clip0", shift=0.0, nodepth=0.0, seed=3),
    "clip180": dict(img=65, pcd=33, K=40, dup=40, G=30, n=64, num_corr=None, N=100, angle="clip180", shift=0.05, nodepth=1.0, seed=4),
    "empty": dict(img=5, pcd=7, K=0, dup=0, G=0, n=0, num_corr=None, N=1, angle=1.5, shift=0.001, nodepth=0.0, seed=5),
}
INPUT_KEYS = ("img_num_nodes", "pcd_num_nodes", "img_node_corr_indices", "pcd_node_corr_indices", "gt_img_node_corr_indices",
              "gt_pcd_node_corr_indices", "gt_node_corr_min_overlaps", "img_corr_points", "pcd_corr_points", "corr_scores", "transform",
              "estimated_transform", "pcd_points")


def rodrigues(axis, deg):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def make_scene(img, pcd, K, dup, G, n, num_corr, N, angle, shift, nodepth, seed):
    """inputs of one pair with the keys of MATR2D3D.forward's output dict / eval.py's .npz.  Points are float32, transforms float64 holding float32
    values (so that a float32 and a float64 run read the same numbers)."""
    r = np.random.RandomState(seed)
    s = dict(img_num_nodes=np.int64(img), pcd_num_nodes=np.int64(pcd), num_corr=num_corr)
    cells = r.permutation(img * pcd)
    gt = cells[:G]
    # predictions: half of them ground truth (where there is any), the rest elsewhere; `dup` of them repeated
    pred = np.zeros(0, np.int64)
    if K:
        uniq = K - dup if dup < K else max(K // 2, 1)                  # distinct predictions
        h = min((uniq + 1) // 2, G)
        base = np.concatenate([gt[:h], cells[G:G + uniq - h]]).astype(np.int64)
        pred = np.concatenate([base, base[r.randint(0, uniq, K - uniq)]])[r.permutation(K)]
    s["img_node_corr_indices"], s["pcd_node_corr_indices"] = pred // pcd, pred % pcd
    s["gt_img_node_corr_indices"], s["gt_pcd_node_corr_indices"] = (gt // pcd).astype(np.int64), (gt % pcd).astype(np.int64)
    ov = r.uniform(0.0, 1.0, G)
    near = np.abs(ov - CFG["acceptance_overlap"]) < 1e-3
    ov[near] += 0.01
    s["gt_node_corr_min_overlaps"] = ov.astype(np.float32)
    R = rodrigues(r.normal(size=3), 25.0 + 10 * seed)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, r.normal(size=3) * 0.3 + np.array([0, 0, 2.0])
    if angle in ("clip0", "clip180"):
        T[:3, :3] *= 1.0 + 1e-6
    T = T.astype(np.float32).astype(np.float64)
    E = T.copy()
    if angle == "clip180":
        E[:3, :3] = T[:3, :3] @ np.diag([1.0, -1.0, -1.0])
    elif angle != "clip0":
        E[:3, :3] = rodrigues(r.normal(size=3), angle) @ T[:3, :3]
    E[:3, 3] += shift * np.array([0.6, -0.48, 0.64])
    E = E.astype(np.float32).astype(np.float64)
    s["transform"], s["estimated_transform"] = T, E
    P = (r.uniform(-1, 1, (n, 3)) * np.array([0.8, 0.6, 0.5])).astype(np.float32)
    noise = r.normal(size=(n, 3)) * np.where(r.uniform(size=(n, 1)) < 0.6, 0.012, 0.15)
    Q = (P.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + noise).astype(np.float32)
    Q[r.uniform(size=n) < nodepth] = 0.0                               # pixels without depth back-project to the origin
    s["pcd_corr_points"], s["img_corr_points"] = P, Q
    s["corr_scores"] = r.permutation(n).astype(np.float32) / max(n, 1) + np.float32(0.25)      # distinct
    s["pcd_points"] = (r.uniform(-1, 1, (N, 3)) * np.array([1.0, 0.8, 0.6])).astype(np.float32)
    return s


def selection(s):
    """eval.py:121-127: the num_corr best by score (None: all of them in order)"""
    sc = s["corr_scores"]
    if s["num_corr"] is not None and sc.shape[0] > s["num_corr"]:
        return np.argsort(-sc, kind="stable")[: s["num_corr"]]
    return None


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------
def apply_transform(p, T):
    return p @ T[:3, :3].T + T[:3, 3]


def _pairs(a, b, width):
    return np.asarray(a, dtype=np.int64) * int(width) + np.asarray(b, dtype=np.int64)


def evaluate_sparse_correspondences(src_length, tgt_length, src_idx, tgt_idx, gt_src_idx, gt_tgt_idx, mutant=None):
    """-> dict(precision, recall, hit_ratio) + the integer counts"""
    W = int(tgt_length)
    listed, gt = _pairs(src_idx, tgt_idx, W), np.unique(_pairs(gt_src_idx, gt_tgt_idx, W))
    pred = np.unique(listed)
    pos = np.intersect1d(pred, gt)
    n_pos, n_pred = pos.shape[0], pred.shape[0]
    if mutant == "dup_twice":                                          # duplicates counted each time they are listed
        n_pos, n_pred = int(np.isin(listed, gt).sum()), listed.shape[0]
    rows = lambda x: np.unique(x // W).shape[0]
    cols = lambda x: np.unique(x % W).shape[0]
    return dict(precision=n_pos / (n_pred + 1e-12), recall=n_pos / (gt.shape[0] + 1e-12),
                hit_ratio=0.5 * (rows(pos) / (rows(gt) + 1e-12) + cols(pos) / (cols(gt) + 1e-12)),
                n_pred=pred.shape[0], n_gt=gt.shape[0], n_pos=pos.shape[0])


def coarse_precision(img_n, pcd_n, img_idx, pcd_idx, gt_img_idx, gt_pcd_idx, gt_overlaps, acceptance_overlap, mutant=None):
    """EvalFunction.evaluate_coarse_matching: the mean over the LISTED predictions (NaN for none) -> (precision, listed positives, GT kept)"""
    ov = np.asarray(gt_overlaps)
    keep = ov >= ov.dtype.type(acceptance_overlap) if mutant == "ge_overlap" else ov > ov.dtype.type(acceptance_overlap)
    gt = np.unique(_pairs(np.asarray(gt_img_idx)[keep], np.asarray(gt_pcd_idx)[keep], pcd_n))
    hit = np.isin(_pairs(img_idx, pcd_idx, pcd_n), gt)
    return (float(hit.mean()) if hit.shape[0] else float("nan")), int(hit.sum()), int(gt.shape[0])


def _nn_dist(q, s):
    """distance from every q to its nearest s (exhaustive, float64)"""
    out = np.empty(q.shape[0])
    for a in range(0, q.shape[0], 512):
        d = q[a:a + 512, None, :] - s[None, :, :]
        out[a:a + 512] = np.sqrt((d * d).sum(-1).min(1))
    return out


def evaluate_correspondences(src_corr_points, tgt_corr_points, transform, positive_radius=0.1, mutant=None, dtype=np.float64):
    """src = cloud, tgt = image (eval.py:153-155) -> dict(overlap, inlier_ratio, distance) + counts + the distances the fixture rules read"""
    src, tgt, T = (np.asarray(x, dtype=dtype) for x in (src_corr_points, tgt_corr_points, transform))
    if src.shape[0] == 0:
        return dict(overlap=0.0, inlier_ratio=0.0, distance=0.0, n_inlier=0, n_overlap=0, corr_dist=np.zeros(0), nn_dist=np.zeros(0))
    moved = apply_transform(src, T)
    d = np.sqrt(((tgt - moved) ** 2).sum(1))
    nn = _nn_dist(moved, tgt) if mutant == "overlap_wrong_direction" else _nn_dist(tgt, moved)
    r = dtype(positive_radius)
    return dict(overlap=float((nn < r).mean()), inlier_ratio=float((d < r).mean()), distance=float(d.mean()), n_inlier=int((d < r).sum()),
                n_overlap=int((nn < r).sum()), corr_dist=d, nn_dist=nn)


def fine_precision(img_corr_points, pcd_corr_points, transform, acceptance_radius, mutant=None, dtype=np.float64):
    """EvalFunction.evaluate_fine_matching -> (precision, kept, inliers among the kept)"""
    img, pcd, T = (np.asarray(x, dtype=dtype) for x in (img_corr_points, pcd_corr_points, transform))
    keep = np.ones(img.shape[0], dtype=bool) if mutant == "no_depth_mask" else img[:, 2] > 0
    d = np.sqrt(((apply_transform(pcd[keep], T) - img[keep]) ** 2).sum(1))
    inl = int((d < dtype(acceptance_radius)).sum())
    kept = int(keep.sum())
    return (inl / kept if kept else 0.0), kept, inl


def registration_rmse(src_points, gt_transform, est_transform, mutant=None, dtype=np.float64):
    p, G, E = (np.asarray(x, dtype=dtype) for x in (src_points, gt_transform, est_transform))
    d2 = ((apply_transform(p, G) - apply_transform(p, E)) ** 2).sum(1)
    return float(np.sqrt(d2).mean()) if mutant == "mean_of_norms" else float(np.sqrt(d2.mean()))


def isotropic_registration_error(gt_transform, est_transform, dtype=np.float64):
    G, E = np.asarray(gt_transform, dtype=dtype), np.asarray(est_transform, dtype=dtype)
    x = 0.5 * ((E[:3, :3] * G[:3, :3]).sum() - 1.0)
    return float(np.degrees(np.arccos(min(max(x, -1.0), 1.0)))), float(np.sqrt(((G[:3, 3] - E[:3, 3]) ** 2).sum()))


def evaluate_registration(pcd_points, transform, est_transform, acceptance_rmse, dtype=np.float64):
    """EvalFunction.evaluate_registration -> (rre, rte, rmse, recall)"""
    p, G, E = (np.asarray(x, dtype=dtype) for x in (pcd_points, transform, est_transform))
    rre, rte = isotropic_registration_error(G, E, dtype)
    moved = apply_transform(p, np.linalg.inv(G) @ E)
    rmse = float(np.sqrt(((moved - p) ** 2).sum(1)).mean())
    return rre, rte, rmse, float(rmse < acceptance_rmse)


def restate(s, dtype=np.float64):
    """every fixture quantity of one scene through the restatement: name -> float / int"""
    o = {}
    sp = evaluate_sparse_correspondences(s["img_num_nodes"], s["pcd_num_nodes"], s["img_node_corr_indices"], s["pcd_node_corr_indices"],
                                         s["gt_img_node_corr_indices"], s["gt_pcd_node_corr_indices"])
    o.update(sp_precision=sp["precision"], sp_recall=sp["recall"], sp_hit_ratio=sp["hit_ratio"], n_pred=sp["n_pred"], n_gt=sp["n_gt"], n_pos=sp["n_pos"])
    o["ev_PIR"], o["n_listed_pos"], o["n_gt_kept"] = coarse_precision(s["img_num_nodes"], s["pcd_num_nodes"], s["img_node_corr_indices"],
                                                                     s["pcd_node_corr_indices"], s["gt_img_node_corr_indices"],
                                                                     s["gt_pcd_node_corr_indices"], s["gt_node_corr_min_overlaps"].astype(dtype),
                                                                     CFG["acceptance_overlap"])
    sel = selection(s)
    P, Q = (s["pcd_corr_points"], s["img_corr_points"]) if sel is None else (s["pcd_corr_points"][sel], s["img_corr_points"][sel])
    ec = evaluate_correspondences(P, Q, s["transform"], CFG["acceptance_radius"], dtype=dtype)
    o.update(ec_overlap=ec["overlap"], ec_inlier_ratio=ec["inlier_ratio"], ec_distance=ec["distance"], n_inlier=ec["n_inlier"], n_overlap=ec["n_overlap"])
    o["ev_IR"], o["n_kept"], o["n_kept_inlier"] = fine_precision(s["img_corr_points"], s["pcd_corr_points"], s["transform"], CFG["acceptance_radius"],
                                                               dtype=dtype)
    o["rmse"] = registration_rmse(s["pcd_points"], s["transform"], s["estimated_transform"], dtype=dtype)
    o["rr"] = int(o["rmse"] < CFG["rmse_threshold"])
    o["rre"], o["rte"] = isotropic_registration_error(s["transform"], s["estimated_transform"], dtype)
    o["ev_rre"], o["ev_rte"], o["ev_rmse"], rec = evaluate_registration(s["pcd_points"], s["transform"], s["estimated_transform"], CFG["rmse_threshold"],
                                                                       dtype)
    o["ev_recall"] = int(rec)
    return o


REAL_KEYS = ("sp_precision", "sp_recall", "sp_hit_ratio", "ev_PIR", "ec_overlap", "ec_inlier_ratio", "ec_distance", "ev_IR", "rmse", "rre", "rte",
             "ev_rre", "ev_rte", "ev_rmse")
INT_KEYS = ("n_pred", "n_gt", "n_pos", "n_listed_pos", "n_gt_kept", "n_inlier", "n_overlap", "n_kept", "n_kept_inlier", "rr", "ev_recall")


def fixture_rules(s):
    """-> list of broken rules (empty = the scene may be a fixture): no decision of the metrics sits within reach of a rounding"""
    bad = []
    r = CFG["acceptance_radius"]
    sel = selection(s)
    P, Q = (s["pcd_corr_points"], s["img_corr_points"]) if sel is None else (s["pcd_corr_points"][sel], s["img_corr_points"][sel])
    ec = evaluate_correspondences(P, Q, s["transform"], r)
    full = evaluate_correspondences(s["pcd_corr_points"], s["img_corr_points"], s["transform"], r)
    for what, d in (("correspondence distance", ec["corr_dist"]), ("nearest-neighbour distance", ec["nn_dist"]),
                    ("correspondence distance (unselected)", full["corr_dist"])):
        if d.shape[0] and np.abs(d - r).min() < 1e-5:
            bad.append("%s within 1e-5 of acceptance_radius" % what)
    ov = s["gt_node_corr_min_overlaps"].astype(np.float64)
    if ov.shape[0] and np.abs(ov - CFG["acceptance_overlap"]).min() < 1e-6:
        bad.append("GT overlap within 1e-6 of acceptance_overlap")
    sc = np.sort(s["corr_scores"])[::-1]
    k = s["num_corr"]
    if k is not None and sc.shape[0] > k and sc[k - 1] == sc[k]:
        bad.append("num_corr-th and (num_corr + 1)-th scores equal")
    a, b = restate(s, np.float64), restate(s, np.float32)
    for key in ("rmse", "ev_rmse"):
        if abs(a[key] - CFG["rmse_threshold"]) < 1e-5:
            bad.append("%s within 1e-5 of rmse_threshold" % key)
    for key in INT_KEYS:
        if a[key] != b[key]:
            bad.append("%s differs between float32 (%d) and float64 (%d)" % (key, b[key], a[key]))
    if not (a["rre"] == 0.0 or a["rre"] >= 1.0):
        bad.append("rotation error %.3g neither 0 nor >= 1 degree" % a["rre"])
    return bad


# ---- the three-scene table of the summarize() test -----------------------------------------------------------------------------------------------
def make_table(seed=7):
    """{scene: [per-pair dict(PIR, IR, OR, n_corr, RR, RRE, RTE)]}: every scene keeps a recalled pair (a scene without one makes eval.py's summary NaN)"""
    r = np.random.RandomState(seed)
    table = {}
    for name, pairs, p_rr in (("kitchen", 5, 0.7), ("office", 3, 0.6), ("stairs", 4, 0.5)):
        rows = []
        for _ in range(pairs):
            rr = float(r.uniform() < p_rr)
            rows.append(dict(PIR=float(r.choice([0.0, 0.05, 0.1, 0.2, 0.3, 0.45, 0.5, 0.8])), IR=float(r.uniform(0, 0.6)), OR=float(r.uniform(0, 1)),
                             RR=rr, RRE=float(r.uniform(0.2, 4.0)), RTE=float(r.uniform(0.01, 0.2))))
        table[name] = rows
    return table
