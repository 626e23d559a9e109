"""Time the device non-rigid ICP solver (dr_nicp_adam_f32) against the same loop in plain PyTorch-ROCm float32 on the same GPU.

    python tools/nonrigid_time.py [--runs 30] [--iters 500] [--out profiles/nonrigid_time.jsonl]

Scene: a synthetic 4DMatch-style pair -- a source cloud of 4096 points, 512 of them graph nodes, 2048 correspondences, K = 6; the target is the source
moved by a smooth scene flow (sin of an affine map, as diffreg_hip.synth.make_metric_points draws it) plus noise.  Timed once for one pair per call
and once for 8 pairs per call (the device solver in one ragged launch, the torch loop once per pair).  Median of --runs alternated runs with
p10-p90 on a device-synchronised host clock.  Per path the end-point error of the warped source cloud against the known flow, before (no warp) and
after.  Reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
from diffreg_hip import nonrigid as nr, synth  # noqa: E402

DEV = "cuda:0"
C, M, N, K, COVERAGE = 4096, 512, 2048, 6, 0.15


def make_pair(seed):
    src = synth.hash_uniform(seed, 1, (C, 3)).astype(np.float64)
    A = 0.8 * synth.hash_normal(seed, 2, (3, 3))
    b = 0.05 * synth.hash_normal(seed, 3, (3,))
    flow = 0.1 * np.sin(src @ A.T) + b
    order = np.argsort(synth.hash_u01(seed, 4, C), kind="stable")
    nodes, corr = order[:M], np.sort(order[M:M + N])
    tgt = src[corr] + flow[corr] + 0.002 * synth.hash_normal(seed, 5, (N, 3))
    f = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)
    return dict(src=f(src), gt=f(src + flow), nodes=f(src[nodes]), corr=torch.from_numpy(corr).to(DEV), tgt=f(tgt))


def torch_solver(nodes, src, tgt, ai, aw, edges, ew, iters):
    """nonrigid_icp_adam.py:76-131 restated in plain torch float32 on the device (autograd + Adam + ExponentialLR); anchors without holes"""
    rot = torch.nn.Parameter(torch.eye(3, device=DEV).repeat(nodes.shape[0], 1, 1))
    trn = torch.nn.Parameter(torch.zeros_like(nodes))
    opt = torch.optim.Adam([rot, trn], lr=0.5)
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.999)
    w = (aw / (aw.sum(1, keepdim=True) + 1e-6))[..., None]
    d = src[:, None] - nodes[ai]
    i, j = edges[:, 0], edges[:, 1]
    dl = nodes[j] - nodes[i]
    for _ in range(iters):
        warped = ((torch.einsum("nkij,nkj->nki", rot[ai], d) + trn[ai] + nodes[ai]) * w).sum(1)
        lm = (warped - tgt).pow(2).sum(1).mean()
        df = torch.einsum("eij,ej->ei", rot[i], dl) + nodes[i] + trn[i] - (nodes[j] + trn[j])
        ar = (df.pow(2).sum(1) * ew).mean()
        G = torch.einsum("mab,mac->mbc", rot, rot)
        orth = (G[:, 0, 1] ** 2 + G[:, 0, 2] ** 2 + G[:, 1, 2] ** 2 + (G[:, 0, 0] - 1) ** 2 + (G[:, 1, 1] - 1) ** 2 + (G[:, 2, 2] - 1) ** 2).mean()
        (lm + 0.1 * ar + 0.1 * orth).backward()
        opt.step()
        opt.zero_grad()
        sch.step()
    T = torch.eye(4, device=DEV).repeat(nodes.shape[0], 1, 1)
    T[:, :3, :3], T[:, :3, 3] = rot.detach(), trn.detach()
    return T


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return dict(median=float(np.median(xs)), p10=float(np.percentile(xs, 10)), p90=float(np.percentile(xs, 90)))


def measure(P, runs, iters):
    pairs = [make_pair(100 + p) for p in range(P)]
    src, nodes = torch.cat([p["src"] for p in pairs]), torch.cat([p["nodes"] for p in pairs])
    g = nr.ed_graph(src, nodes, K, COVERAGE, point_lengths=[C] * P, node_lengths=[M] * P)
    rows = torch.cat([p["corr"] + C * k for k, p in enumerate(pairs)])
    ai, aw = g["anchor_indices"][rows].contiguous(), g["anchor_weights"][rows].contiguous()
    pb = nr.Problem(nodes, src[rows], torch.cat([p["tgt"] for p in pairs]), ai, aw, g["edge_indices"], g["edge_weights"], node_lengths=[M] * P,
                    corr_lengths=[N] * P, edge_lengths=g["edge_lengths"])
    per_pair, e0 = [], 0
    for k, p in enumerate(pairs):
        e1 = e0 + g["edge_lengths"][k]
        per_pair.append((p["nodes"], p["src"][p["corr"]], p["tgt"], ai[k * N:(k + 1) * N], aw[k * N:(k + 1) * N], g["edge_indices"][e0:e1],
                         g["edge_weights"][e0:e1]))
        e0 = e1
    device = lambda: nr.nicp_adam(pb, num_iterations=iters)[0]
    plain = lambda: torch.cat([torch_solver(*a, iters) for a in per_pair])
    device(); torch_solver(*per_pair[0], 3)                 # warm-up: kernel load, allocator
    t_dev, t_tor = [], []
    for _ in range(runs):
        ms, T_dev = clock(device); t_dev.append(ms)
        ms, T_tor = clock(plain); t_tor.append(ms)
    gt = torch.cat([p["gt"] for p in pairs])
    epe = lambda T: float((nr.ed_warp(src, nodes, T, g["anchor_indices"], g["anchor_weights"], point_lengths=[C] * P, node_lengths=[M] * P)[0]
                           - gt).norm(dim=1).mean())
    return dict(pairs=P, nodes=M, correspondences=N, K=K, edges=g["edge_lengths"], iterations=iters, runs=runs, device_ms=stats(t_dev),
                torch_ms=stats(t_tor), speedup_median=float(np.median(t_tor) / np.median(t_dev)), epe_before=float((src - gt).norm(dim=1).mean()),
                epe_after_device=epe(T_dev), epe_after_torch=epe(T_tor), max_abs_diff_transforms=float((T_dev - T_tor).abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nonrigid_time.jsonl"))
    a = ap.parse_args()
    with open(a.out, "w") as f:
        for P in (1, 8):
            rec = dict(tool="nonrigid_time", device=torch.cuda.get_device_name(0), **measure(P, a.runs, a.iters))
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
