"""Time the point-to-point ICP on one GPU against baselines that are NOT the code under test:

    python tools/icp_time.py [--runs 30] [--out profiles/icp_time.jsonl]

Shapes: one pair of 30 000 x 30 000 points at threshold 0.05 and 30 iterations with relative_* = 0; eight such pairs in one call; a
three-scale multi_scale_icp (voxel 0.1 / 0.05 / 0.025, 30 iterations each).
Baselines: (i) the same loop in plain PyTorch float32 on the same GPU -- chunked cdist + argmin, masked Kabsch with torch.linalg.svd, and the
convergence values read back per iteration, as the loop shape of Open3D's registration_icp implies; (ii) the library's own composition of
older entries -- dr_knn_points_f32 with k = 1 (brute force) plus dr_weighted_procrustes_f32 per iteration, with the same read; every GPU
baseline runs the device call's 31 evaluations and 30 fits, and the eight-pair shape is timed against eight baseline loops; (iii) the
numpy / cKDTree statement on the host (three runs: it takes seconds).  Each device / baseline pair alternates run by run; a device-synchronised
clock; median with p10 - p90 in milliseconds.  The launch floor of a call is 2 * max_iteration dependent launches."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)
LAUNCH_US = 4.7


def apply(T, p):
    return p @ T[:3, :3].T + T[:3, 3]


def kabsch(p, q, w):
    n = w.sum()
    pc, qc = (w[:, None] * p).sum(0) / n, (w[:, None] * q).sum(0) / n
    H = (p - pc).T @ (w[:, None] * (q - qc))
    U, _, Vh = torch.linalg.svd(H)
    V = Vh.T
    D = torch.eye(3, device=p.device)
    D[2, 2] = torch.sign(torch.det(V @ U.T))
    R = V @ D @ U.T
    T = torch.eye(4, device=p.device)
    T[:3, :3], T[:3, 3] = R, qc - R @ pc
    return T


def torch_nn(moved, tgt, chunk=4096):
    d, j = [], []
    for lo in range(0, moved.shape[0], chunk):
        m = torch.cdist(moved[lo:lo + chunk], tgt)
        v, i = m.min(1)
        d.append(v), j.append(i)
    return torch.cat(d), torch.cat(j)


def loop(src, tgt, T, r, iters, nn, kabsch=kabsch):
    """Open3D's loop shape: evaluate, then per iteration fit, compose, evaluate and read fitness / rmse back"""
    last = None
    for k in range(iters + 1):                               # iters + 1 evaluations, iters fits: what the device call runs
        moved = apply(T, src)
        d, j = nn(moved, tgt)
        w = (d < r).float()
        res = (float(w.sum()) / src.shape[0], float(torch.sqrt((w * d * d).sum() / w.sum())))     # the read per iteration
        if k == iters or (last is not None and abs(res[0] - last[0]) < 0.0 and abs(res[1] - last[1]) < 0.0):
            break
        last = res
        T = kabsch(moved, tgt[j], w) @ T
    return T


def host_loop(src, tgt, T, r, iters):
    from scipy.spatial import cKDTree
    from tests import icp_ref as R
    tree = cKDTree(tgt)
    for _ in range(iters):
        moved = src @ T[:3, :3].T + T[:3, 3]
        d, j = tree.query(moved, distance_upper_bound=r)
        keep = np.isfinite(d)
        T = R.fit(moved[keep], tgt[j[keep]])[0] @ T
    return T


def alternate(fa, fb, runs):
    ta, tb = [], []
    for f in (fa, fb):
        f()
    torch.cuda.synchronize()
    for _ in range(runs):
        for f, acc in ((fa, ta), (fb, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            acc.append((time.perf_counter() - t0) * 1e3)
    st = lambda t: dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)))
    return st(ta), st(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--points", type=int, default=30000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_time.jsonl"))
    a = ap.parse_args()
    from diffreg_hip import lib, metrics_nonrigid, registration as G
    from tests import icp_ref as R
    rng = np.random.default_rng(0)
    N, r, iters = a.points, 0.05, 30
    # a surface-like cloud: the density a registration user meets (a 2 m x 2 m x 0.4 m slab of 30 000 points)
    base = rng.uniform(0, 1, (N, 3)) * [2.0, 2.0, 0.4]
    Gt = R.pose([0.2, 1.0, 0.3], 20.0, [0.4, -0.3, 0.2])
    tgt_np = (base[rng.permutation(N)] @ Gt[:3, :3].T + Gt[:3, 3] + rng.normal(size=(N, 3)) * 0.002).astype(np.float32)
    src_np = base.astype(np.float32)
    init_np = (R.pose([1, 0, 1], 1.5, [0.01, -0.01, 0.01]) @ Gt).astype(np.float32)
    src, tgt, init = [torch.from_numpy(x).cuda() for x in (src_np, tgt_np, init_np)]
    off = torch.tensor([0, N], dtype=torch.int32, device="cuda")
    rows = []

    def record(name, fa, fb, baseline, **kw):
        da, db = alternate(fa, fb, a.runs)
        rows.append(dict(name=name, device=da, baseline=db, baseline_is=baseline, launch_floor_ms=2 * iters * LAUNCH_US * 1e-3, **kw))
        print("%-34s device %.3f ms (%.3f - %.3f)   %s %.3f ms (%.3f - %.3f)" % (name, da["median_ms"], da["p10_ms"], da["p90_ms"], baseline,
                                                                              db["median_ms"], db["p10_ms"], db["p90_ms"]), flush=True)
    dev1 = lambda: G.icp_pairs(src, tgt, off, off, init[None], r, iters, 0.0, 0.0)

    def knn_nn(moved, t):                                    # dr_knn_points_f32 returns the squared distance: nothing is recomputed
        d2, j, _ = metrics_nonrigid.knn_points(moved, t, 1)
        return torch.sqrt(d2[:, 0]), j[:, 0]
    out = dev1()
    torch.cuda.synchronize()
    print("device: fitness %.4f rmse %.5f iterations %d; pose error %.2e" % (float(out["fitness"]), float(out["inlier_rmse"]),
                                                                           int(out["iterations"]), float((out["transforms"][0].cpu().double()
                                                                                                          - torch.from_numpy(Gt)).abs().max())))
    record("icp_1x%dx%d_30it" % (N, N), dev1, lambda: loop(src, tgt, init, r, iters, torch_nn), "torch_cdist_svd_read")
    fit = lambda p, q, w: G.weighted_procrustes(p, q, weights=w, eps=0.0)
    record("icp_1x%dx%d_30it_vs_composition" % (N, N), dev1, lambda: loop(src, tgt, init, r, iters, knn_nn, fit),
           "knn_points_k1+weighted_procrustes_composition")
    s8, t8 = src.repeat(8, 1), tgt.repeat(8, 1)
    off8 = torch.arange(9, device="cuda", dtype=torch.int32) * N
    record("icp_8x%dx%d_30it_one_call" % (N, N), lambda: G.icp_pairs(s8, t8, off8, off8, init[None].repeat(8, 1, 1), r, iters, 0.0, 0.0),
           lambda: [loop(src, tgt, init, r, iters, torch_nn) for _ in range(8)], "torch_cdist_svd_read_8_loops", baseline_pairs=8)
    cfgs = [dict(voxel_size=v, max_iteration=iters) for v in (0.1, 0.05, 0.025)]

    def torch_scales():
        T = init
        for cfg in cfgs:
            s, t = G.voxel_down_sample(src, cfg["voxel_size"]), G.voxel_down_sample(tgt, cfg["voxel_size"])
            T = loop(s, t, T, r, iters, torch_nn)
        return T
    record("multi_scale_icp_3_scales", lambda: G.multi_scale_icp(src, tgt, init, cfgs, r, relative_fitness=0.0, relative_rmse=0.0), torch_scales,
           "device_downsample+torch_loop")
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_loop(src_np.astype(np.float64), tgt_np.astype(np.float64), init_np.astype(np.float64), r, iters)
        t.append((time.perf_counter() - t0) * 1e3)
    rows.append(dict(name="host_numpy_ckdtree_1x%dx%d_30it" % (N, N), host=dict(median_ms=float(np.median(t)), runs=3)))
    print("host numpy / cKDTree statement: %.1f ms" % np.median(t))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
