"""Time the fine loss, one ladder rung's Procrustes and the train-mode warp on one GPU: the device path against the PLAIN PyTorch restatement on
the same GPU (tests/finenoise2d3d_ref.py -- for the fit and the warp with the reference's full sort and its `.cpu()` SVD round trip).

    python tools/finenoise2d3d_time.py [--out FILE.json]

Method of DESIGN 5f-5h: 5 warm-up runs, then 30 runs alternating the two sides, each between two device synchronisations; median [p10-p90] in
milliseconds.  Rows: (a) fine loss forward + backward at M = 256, C = 128, H W = 480 x 640, N = 20 000; (b) the fit on a 0 / 1 matrix at
1 024 x 1 530; (c) the warp at that size, forward and forward + backward."""
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


def cpu_svd_procrustes(F, conf, s, t, sm, tm):
    """tests/finenoise2d3d_ref.soft_procrustes with the reference's device -> host -> device SVD (EXP/procrustes.py:35-45)"""
    B, N, M = conf.shape
    entry_max = (torch.stack([sm.sum(1), tm.sum(1)], 0).max(0)[0] * 1.0).int()
    K = int(entry_max.float().mean().int())
    srt, idx = conf.view(B, -1).sort(descending=True, dim=1)
    w, idx = srt[:, :K].clone(), idx[:, :K]
    X, Y = s[0, (idx // M).view(-1)].view(B, K, -1), t[0, (idx % M).view(-1)].view(B, K, -1)
    w = w[..., None]
    wn = w / (w.abs().sum(1, keepdim=True) + 0.0001)
    mx, my = (wn * X).sum(1, keepdim=True), (wn * Y).sum(1, keepdim=True)
    Sxy = torch.matmul((Y - my).transpose(1, 2), wn * (X - mx)).cpu().double()
    U, D, V = Sxy.svd()
    cond = D.max(1)[0] / D.min(1)[0]
    S = torch.eye(3)[None].repeat(B, 1, 1).double()
    S[:, 2:3, 2:3] = (U.det() * V.det()).view(-1, 1, 1)
    R = torch.matmul(U, torch.matmul(S, V.transpose(1, 2))).float().to(conf.device)
    tt = my.transpose(1, 2) - torch.matmul(R, mx.transpose(1, 2))
    ok = cond < 200.0
    Rf, tf = R.clone(), tt.clone()
    Rf[~ok] = torch.eye(3).type_as(R)
    tf[~ok] = torch.zeros(3, 1).type_as(R)
    return R, tt, Rf, tf, cond, ok


def main():
    from diffreg_hip import autograd2d3d, lib
    from tests import finenoise2d3d_ref as F
    from tests.train2d3d_ref import log_optimal_transport
    res = {}
    # (a) the fine loss
    sc = F.make_fine_scene(H=480, W=640, N=20000, C=128, K=256, seed=3)
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in sc.items()}
    px, idx = d["img_corr_pixels"], d["pcd_corr_indices"]
    c = F.FINE_CFG
    prm = lib.fine_params(c["pos_radius_3d"], c["neg_radius_3d"], c["pos_radius_2d"], c["neg_radius_2d"], c["pos_margin"], c["neg_margin"],
                          c["pos_optimal"], c["neg_optimal"], c["log_scale"])

    def fine(device_path):
        fi, fp = d["img_feats"].requires_grad_(True), d["pcd_feats"].requires_grad_(True)
        fi.grad = fp.grad = None
        if device_path:
            loss, _ = autograd2d3d.fine_loss(fi, fp, d["img_points"], d["pcd_points"], d["pcd_pixels"], d["transform"], px, idx, d["image_w"], prm)
        else:
            loss, _ = F.fine_loss(d, px, idx, torch.float32, c, fi, fp)
        loss.backward()
    res["fine_loss_fwd_bwd"] = measure({"torch": lambda: fine(False), "device": lambda: fine(True)})
    # (b), (c) at the coarse level's size
    N, M = 1024, 1530
    w = F.make_warp_case(N=N, M=M, nv=N, mv=M, seed=7)
    w = {k: v.to(DEV) for k, v in w.items()}
    layer = F.SoftProcrustesLayer()
    with torch.no_grad():
        res["ladder_fit"] = measure({
            "torch": lambda: cpu_svd_procrustes(F, w["matrix_gt"], w["s_pcd"], w["t_pcd"], w["src_mask"], w["tgt_mask"]),
            "device": lambda: autograd2d3d.soft_procrustes(layer, w["matrix_gt"], w["s_pcd"], w["t_pcd"], w["src_mask"], w["tgt_mask"])})
    host = torch.nn.Module()
    host.denoising_coarse_matching = torch.nn.Module()
    host.denoising_coarse_matching.bin_score = torch.nn.Parameter(torch.tensor(1.0, device=DEV))
    host.denoising_coarse_matching.skh_iters = 3
    host.denoising_soft_procrustes = layer
    bs = host.denoising_coarse_matching.bin_score

    def torch_warp(backward):
        x = w["scores"].double().masked_fill(~(w["src_mask"][..., None] * w["tgt_mask"][:, None]).bool(), float("-inf"))
        conf = log_optimal_transport(x, bs, 3, w["src_mask"], w["tgt_mask"]).exp()[:, :-1, :-1].contiguous().type(torch.float32)
        _, _, Rf, tf, _, _ = cpu_svd_procrustes(F, conf, w["s_pcd"], w["t_pcd"], w["src_mask"], w["tgt_mask"])
        out = (torch.matmul(Rf, w["s_pcd"].transpose(1, 2)) + tf).transpose(1, 2)
        if backward:
            bs.grad = None
            (out * w["w"]).sum().backward()

    def device_warp(backward):
        out = autograd2d3d.noising_warp(host, w["s_pcd"], w["t_pcd"], w["src_mask"], w["tgt_mask"], w["scores"].double())[0]
        if backward:
            bs.grad = None
            (out * w["w"]).sum().backward()
    with torch.no_grad():
        res["warp_fwd"] = measure({"torch": lambda: torch_warp(False), "device": lambda: device_warp(False)})
    res["warp_fwd_bwd"] = measure({"torch": lambda: torch_warp(True), "device": lambda: device_warp(True)})
    for k, v in res.items():
        print("%-18s" % k, "  ".join("%s %.3f [%.3f-%.3f] ms" % (s, r["median"], r["p10"], r["p90"]) for s, r in v.items()))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
