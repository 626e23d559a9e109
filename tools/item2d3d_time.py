"""Time the 2D-3D dataset item's ground truth on one GPU:

    python tools/item2d3d_time.py [--out FILE.jsonl] [--host-runs K]

Method of tools/eval2d3d_time.py: 5 warm-up runs, then 30 runs alternating the sides, each between two device synchronisations; median [p10-p90]
in milliseconds.  One item at the reference's crop: 476 x 630 pixels, 30 000 points, matching_radius_2d = 8, matching_radius_3d = 0.0375.
Rows: the mutual variant, the radius variant, prepare_item as a whole (augmentation, mutual pairs).  Sides: `device` = diffreg_hip.item2d3d;
`torch` = a chunked brute-force statement in plain PyTorch float64 on the same GPU (4 096 pixels x all points per chunk); `host` = the
reference's procedure in numpy with scipy's cKDTree on this machine's CPU (two trees and two k = 1 queries; a tree and query_ball_point), when
scipy is importable -- fewer runs (--host-runs, default 5 / 2): one run of the radius variant takes seconds.  The lists of the three sides are
compared before anything is timed."""
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
DEV = "cuda:0"
H, W, N, R2D, R3D, LIMIT = 476, 630, 30000, 8.0, 0.0375, 6.0


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
    return {k: dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), runs=len(v))
            for k, v in out.items()}


def make_scene(seed=3):
    from tests import item2d3d_ref as F
    rng = np.random.RandomState(seed)
    K = np.array([[585.0, 0.0, 320.0], [0.0, 585.0, 240.0], [0.0, 0.0, 1.0]])
    col, row = np.arange(W)[None, :], np.arange(H)[:, None]
    d = 1500.0 + 1.5 * col + 1.0 * row + np.where(col >= W // 2, 600.0, 0.0) + rng.randint(-15, 16, size=(H, W))
    d = np.where(rng.rand(H, W) < 0.10, 0.0, d).astype(np.float32)
    T = F.rigid(rng)
    ip, _ = F.image_points(d, K)
    base = ip[rng.randint(0, len(ip), size=N)] + 0.02 * rng.randn(N, 3)
    pts = ((base - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    return d, pts, K, T


def torch_tables(depth, pts, K, T):
    z = depth.double().reshape(-1) / 1000.0
    z = torch.where(z > LIMIT, torch.zeros_like(z), z)
    flat = torch.arange(H * W, device=DEV)
    rowf = flat.double() / W                 # back_project's true division, in float64 (an int64 / int division would give float32)
    keep = z > 0
    x = ((flat % W) - K[0, 2]) * z / K[0, 0]
    y = (rowf - K[1, 2]) * z / K[1, 1]
    ip = torch.stack([x, y, z], 1)[keep]
    px = torch.stack([flat // W, flat % W], 1)[keep]
    q = pts.double() @ T[:3, :3].T + T[:3, 3]
    rp = torch.stack([(K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]).trunc(), (K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2]).trunc()], 1)
    return ip, px, q, rp


def torch_mutual(depth, pts, K, T, chunk=4096):
    ip, px, q, rp = torch_tables(depth, pts, K, T)
    nn_i = torch.empty(ip.shape[0], dtype=torch.int64, device=DEV)
    d_i = torch.empty(ip.shape[0], dtype=torch.float64, device=DEV)
    best_d = torch.full((N,), float("inf"), dtype=torch.float64, device=DEV)
    best_i = torch.zeros(N, dtype=torch.int64, device=DEV)
    for s in range(0, ip.shape[0], chunk):
        d2 = torch.cdist(ip[s:s + chunk], q, compute_mode="donot_use_mm_for_euclid_dist")
        d_i[s:s + chunk], nn_i[s:s + chunk] = d2.min(1)
        cd, ci = d2.min(0)
        better = cd < best_d
        best_d = torch.where(better, cd, best_d)
        best_i = torch.where(better, ci + s, best_i)
    i = torch.arange(ip.shape[0], device=DEV)
    keep = (best_i[nn_i] == i) & (d_i < R3D) & ((px - rp[nn_i]).double().norm(dim=1) < R2D)
    return px[keep], nn_i[keep]


def torch_radius(depth, pts, K, T, chunk=4096):
    ip, px, q, rp = torch_tables(depth, pts, K, T)
    pix, idx = [], []
    for s in range(0, ip.shape[0], chunk):
        d = torch.cdist(ip[s:s + chunk], q, compute_mode="donot_use_mm_for_euclid_dist")
        i, j = torch.nonzero(d < R3D, as_tuple=True)
        ok = (px[s + i] - rp[j]).double().norm(dim=1) < R2D
        pix.append(px[s + i[ok]])
        idx.append(j[ok])
    return torch.cat(pix), torch.cat(idx)


def host_sides(d, pts, K, T):
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    from tests import item2d3d_ref as F

    def tables():
        ip, px = F.image_points(d, K)
        q = F.transformed(pts, T)
        return ip, px, q

    def mutual():
        ip, px, q = tables()
        nn_i = cKDTree(q).query(ip, k=1)[1]
        nn_j = cKDTree(ip).query(q, k=1)[1]
        i = np.arange(len(ip))
        i = i[nn_j[nn_i] == i]
        j = nn_i[i]
        rp, _ = F.render(q[j], K)
        keep = (np.linalg.norm(ip[i] - q[j], axis=1) < R3D) & (np.linalg.norm(px[i] - rp, axis=1) < R2D)
        return px[i[keep]], j[keep]

    def radius():
        ip, px, q = tables()
        lists = cKDTree(q).query_ball_point(ip, R3D)
        corr = np.array([(j, i) for i, l in enumerate(lists) for j in l], dtype=np.int64)
        j, i = corr[:, 0], corr[:, 1]
        rp, _ = F.render(q[j], K)
        keep = np.linalg.norm(px[i] - rp, axis=1) < R2D
        return px[i[keep]], j[keep]

    return mutual, radius


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "item2d3d_time.jsonl"))
    ap.add_argument("--host-runs", type=int, nargs=2, default=(5, 2))
    a = ap.parse_args()
    from diffreg_hip import item2d3d as it
    d, pts, K, T = make_scene()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    depth, points, Kd, Td = t(d), t(pts), t(K), t(T)
    args = (depth, points, Kd, Td, R2D, R3D)
    mp, mi = it.get_2d3d_correspondences_mutual(*args)
    rp, ri = it.get_2d3d_correspondences_radius(*args)
    tp, ti = torch_mutual(depth, points, Kd, Td)
    same_m = bool(torch.equal(mp, tp) and torch.equal(mi, ti))
    tp, ti = torch_radius(depth, points, Kd, Td)
    same_r = bool(torch.equal(rp, tp) and torch.equal(ri, ti))
    print("pairs: mutual %d, radius %d; equal to the brute-force torch lists: %s %s" % (len(mi), len(ri), same_m, same_r), flush=True)
    host = host_sides(d, pts, K, T)
    rows = []
    res = measure({"device": lambda: it.get_2d3d_correspondences_mutual(*args), "torch": lambda: torch_mutual(depth, points, Kd, Td)})
    rows.append(dict(row="mutual", pairs=len(mi), equal_to_torch=same_m, **res))
    print(rows[-1], flush=True)
    res = measure({"device": lambda: it.get_2d3d_correspondences_radius(*args), "torch": lambda: torch_radius(depth, points, Kd, Td)}, runs=10)
    rows.append(dict(row="radius", pairs=len(ri), equal_to_torch=same_r, **res))
    print(rows[-1], flush=True)
    raw = dict(depth=d.astype(np.float64), image=np.zeros((H, W, 3)), image_gray=np.zeros((H, W)), ori_image=np.zeros((H, W, 3), np.uint8), points=pts,
               intrinsics=K, cloud_to_image=T)
    raw_dev = {k: t(v) for k, v in raw.items()}
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    opt = dict(max_points=None, use_augmentation=True, augmentation_noise=0.005, return_corr_indices=True, matching_method="mutual_nearest",
               matching_radius_2d=R2D, matching_radius_3d=R3D, return_overlap_indices=False)
    res = measure({"device_inputs_on_device": lambda: it.prepare_item(raw_dev, device=DEV, generator=gen, **opt),
                   "device_inputs_on_host": lambda: it.prepare_item(raw, device=DEV, generator=gen, **opt)})
    rows.append(dict(row="prepare_item", **res))
    print(rows[-1], flush=True)
    if host is not None:
        for name, fn, runs in (("mutual", host[0], a.host_runs[0]), ("radius", host[1], a.host_runs[1])):
            hp, hi = fn()
            if name == "radius":
                order = np.lexsort((hi, hp[:, 0] * W + hp[:, 1]))
                hp, hi = hp[order], hi[order]
            dev_p, dev_i = (mp, mi) if name == "mutual" else (rp, ri)
            same = bool(np.array_equal(hp, dev_p.cpu().numpy()) and np.array_equal(hi, dev_i.cpu().numpy()))
            res = measure({"host": fn}, warm=1, runs=runs)
            rows.append(dict(row=name + "_host_ckdtree", equal_to_device=same, **res))
            print(rows[-1], flush=True)
    else:
        rows.append(dict(row="host_ckdtree", note="scipy is not importable here: not measured"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
