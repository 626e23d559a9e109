"""Time the device Gauss-Newton non-rigid ICP (dr_nicp_gn_f32) against (b) the same algorithm in the reference's dense shape in plain
PyTorch-ROCm float32 on the same GPU and (c) the device Adam solver at 500 iterations.

    python tools/nonrigid_gn_time.py [--runs 30] [--out profiles/nonrigid_gn_time.jsonl]

Scene and clock are tools/nonrigid_time.py's: 512 nodes, 2 048 correspondences, K = 6, one pair and eight pairs per call; median of --runs
alternated runs with p10-p90 on a device-synchronised host clock; per path the end-point error of the warped source cloud against the known
flow.  (b) is the dense twin of tests/nonrigid_gn_ref.py's block-wise statement: the (3 C + 3 E) x 6 M Jacobian by indexed assignment, J^T J,
torch.linalg.solve, Rodrigues -- what vision3d/layers/nonrigid_icp.py does, restated here; it runs once per pair.  The function's defaults
(corr 1.0, arap 0.1, lm 0.1), 5 iterations.  Reads nothing outside the repository."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
from diffreg_hip import nonrigid as nr  # noqa: E402

_spec = importlib.util.spec_from_file_location("nonrigid_time", os.path.join(ROOT, "tools", "nonrigid_time.py"))
nt = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(nt)
DEV, C, M, N, K, COVERAGE = nt.DEV, nt.C, nt.M, nt.N, nt.K, nt.COVERAGE
LAMBDAS = dict(corr_lambda=1.0, arap_lambda=0.1, lm_lambda=0.1)


def skew(v):
    z = torch.zeros_like(v[:, 0])
    return torch.stack([z, -v[:, 2], v[:, 1], v[:, 2], z, -v[:, 0], -v[:, 1], v[:, 0], z], dim=1).view(-1, 3, 3)


def exp_so3(phi):
    theta = phi.norm(dim=-1)
    Kx = skew(phi / theta.clamp(min=1e-6)[:, None])
    eye = torch.eye(3, device=phi.device).expand_as(Kx)
    return eye + torch.sin(theta)[:, None, None] * Kx + (1.0 - torch.cos(theta))[:, None, None] * (Kx @ Kx)


def dense_gn(nodes, src, tgt, ai, aw, edges, ew, iters, corr_lambda, arap_lambda, lm_lambda):
    """the reference-shaped dense Gauss-Newton in float32 torch on the device; anchors without holes"""
    Mn, Nc = nodes.shape[0], src.shape[0]
    u, v = edges[:, 0], edges[:, 1]
    keep = u != v
    u, v, s = u[keep], v[keep], arap_lambda * ew[keep].sqrt()
    dl, E = nodes[v] - nodes[u], int(keep.sum())
    e_idx = torch.arange(E, device=DEV)
    ci, col = torch.nonzero((ai != -1) & (aw > 0), as_tuple=True)
    ni, cw = ai[ci, col], aw[ci, col]
    cd = src[ci] - nodes[ni]
    wn = (aw / (aw.sum(1, keepdim=True) + 1e-6))[..., None]
    eye3 = torch.eye(3, device=DEV)
    rot, trn = eye3.repeat(Mn, 1, 1), torch.zeros_like(nodes)
    for _ in range(iters):
        Jc = torch.zeros(2, Nc, Mn, 3, 3, device=DEV)
        Jc[0, ci, ni] = -corr_lambda * cw[:, None, None] * skew(torch.einsum("nij,nj->ni", rot[ni], cd))
        Jc[1, ci, ni] = corr_lambda * cw[:, None, None] * eye3
        Jc = Jc.permute(1, 3, 0, 2, 4).reshape(Nc * 3, Mn * 6)
        warped = ((torch.einsum("nkij,nkj->nki", rot[ai], src[:, None] - nodes[ai]) + trn[ai] + nodes[ai]) * wn).sum(1)
        res = (corr_lambda * (warped - tgt)).flatten()
        rd = torch.einsum("eij,ej->ei", rot[u], dl)
        Ja = torch.zeros(2, E, Mn, 3, 3, device=DEV)
        Ja[0, e_idx, u] = -s[:, None, None] * skew(rd)
        Ja[1, e_idx, u] = s[:, None, None] * eye3
        Ja[1, e_idx, v] = -s[:, None, None] * eye3
        Ja = Ja.permute(1, 3, 0, 2, 4).reshape(E * 3, Mn * 6)
        ra = (s[:, None] * (rd + trn[u] + nodes[u] - nodes[v] - trn[v])).flatten()
        J, r = torch.cat([Jc, Ja]), torch.cat([res, ra])
        del Jc, Ja
        A = J.T @ J + lm_lambda * torch.eye(Mn * 6, device=DEV)
        x = torch.linalg.solve(A, -(J.T @ r))
        del J
        rot, trn = exp_so3(x[:Mn * 3].view(Mn, 3)) @ rot, trn + x[Mn * 3:].view(Mn, 3)
    T = torch.eye(4, device=DEV).repeat(Mn, 1, 1)
    T[:, :3, :3], T[:, :3, 3] = rot, trn
    return T


def build(P):
    """P pairs of the scene stacked: (problem, per-pair argument tuples of the dense twin, stacked cloud, stacked nodes, graph, known warp)"""
    pairs = [nt.make_pair(100 + p) for p in range(P)]
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
    return pb, per_pair, src, nodes, g, torch.cat([p["gt"] for p in pairs])


def measure(P, runs, iters, adam_iters):
    pb, per_pair, src, nodes, g, gt = build(P)
    out = nr.gn_buffers(pb)                                 # outputs and workspace allocated once, as a caller in a loop would
    device = lambda: nr.nicp_gauss_newton(pb, num_iterations=iters, out=out, **LAMBDAS)[0]
    dense = lambda: torch.cat([dense_gn(*a, iters, **LAMBDAS) for a in per_pair])
    adam = lambda: nr.nicp_adam(pb, num_iterations=adam_iters)[0]
    device(); dense_gn(*per_pair[0], 1, **LAMBDAS); adam()   # warm-up: kernel load, allocator, solver handles
    t = dict(device=[], dense=[], adam=[])
    T = {}
    for _ in range(runs):
        for name, fn in (("device", device), ("dense", dense), ("adam", adam)):
            ms, res = nt.clock(fn)
            t[name].append(ms)
            T[name] = res.clone()
    epe = lambda X: float((nr.ed_warp(src, nodes, X, g["anchor_indices"], g["anchor_weights"], point_lengths=[C] * P, node_lengths=[M] * P)[0]
                           - gt).norm(dim=1).mean())
    return dict(pairs=P, nodes=M, correspondences=N, K=K, edges=g["edge_lengths"], gn_iterations=iters, adam_iterations=adam_iters, runs=runs,
                device_gn_ms=nt.stats(t["device"]), torch_dense_gn_ms=nt.stats(t["dense"]), device_adam_ms=nt.stats(t["adam"]),
                dense_over_device=float(np.median(t["dense"]) / np.median(t["device"])),
                adam_over_device=float(np.median(t["adam"]) / np.median(t["device"])), epe_before=float((src - gt).norm(dim=1).mean()),
                epe_device_gn=epe(T["device"]), epe_torch_dense_gn=epe(T["dense"]), epe_device_adam=epe(T["adam"]),
                max_abs_diff_gn_transforms=float((T["device"] - T["dense"]).abs().max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--adam-iters", type=int, default=500)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--once", action="store_true", help="run the device entry once per pair count and exit (for a profiler)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nonrigid_gn_time.jsonl"))
    a = ap.parse_args()
    if a.once:
        for P in a.pairs:
            pb = build(P)[0]
            nr.nicp_gauss_newton(pb, num_iterations=a.iters, **LAMBDAS)
            torch.cuda.synchronize()
        return
    with open(a.out, "w") as f:
        for P in a.pairs:
            rec = dict(tool="nonrigid_gn_time", device=torch.cuda.get_device_name(0), **measure(P, a.runs, a.iters, a.adam_iters))
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
