"""Time the RANSAC-free rigid estimators on one GPU against the same procedure in plain PyTorch float32 on that GPU:

    python tools/lgr_time.py [--runs 30] [--out profiles/lgr_time.jsonl]

Shapes: one LocalGlobalRegistration.forward at 256 patch pairs of 64 x 64 scores (one problem); the same correspondences, eight problems in
one local_to_global_registration_pairs call (baseline: eight calls); the spatial-consistency row sums and 10 power iterations at N = 5 000.
Baseline: the reference-shaped statement -- topk both ways, torch.nonzero, the chunk list read back to a Python list, padded batches built
with index_put_, every 3 x 3 SVD on the host (H.cpu()), the dense N x N consistency matrix, allclose read back every iteration.  It is NOT
the code under test.  Each pair of timings alternates device / baseline run by run; median with p10 - p90 in milliseconds."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)


def ref_procrustes(src, tgt, w, eps=1e-5):
    w = torch.where(w < 0.0, torch.zeros_like(w), w)
    w = (w / (w.sum(1, keepdim=True) + eps)).unsqueeze(2)
    sc, tc = (src * w).sum(1, keepdim=True), (tgt * w).sum(1, keepdim=True)
    H = (src - sc).permute(0, 2, 1) @ (w * (tgt - tc))
    U, _, V = torch.svd(H.cpu())
    Ut, V = U.transpose(1, 2).cuda(), V.cuda()
    eye = torch.eye(3, device=src.device).unsqueeze(0).repeat(src.shape[0], 1, 1)
    eye[:, -1, -1] = torch.sign(torch.det(V @ Ut))
    Rm = V @ eye @ Ut
    t = tc.permute(0, 2, 1) - Rm @ sc.permute(0, 2, 1)
    T = torch.eye(4, device=src.device).repeat(src.shape[0], 1, 1)
    T[:, :3, :3], T[:, :3, 3] = Rm, t.squeeze(2)
    return T


def ref_lgr(src_all, tgt_all, scores, batch_indices, radius, min_local=3, steps=5):
    cut = (torch.nonzero(batch_indices[1:] != batch_indices[:-1])[:, 0] + 1).cpu().numpy().tolist()
    cut = [0] + cut + [batch_indices.shape[0]]
    chunks = [(x, y) for x, y in zip(cut[:-1], cut[1:]) if y - x >= min_local]
    dev = src_all.device
    apply = lambda T, p: p @ T[..., :3, :3].transpose(-1, -2) + T[..., None, :3, 3]
    mx = max(y - x for x, y in chunks)
    idx = torch.cat([torch.arange(x, y) for x, y in chunks]).to(dev)
    dst = torch.cat([torch.arange(i * mx, i * mx + y - x) for i, (x, y) in enumerate(chunks)]).to(dev)
    bs, bt, bw = torch.zeros(len(chunks) * mx, 3, device=dev), torch.zeros(len(chunks) * mx, 3, device=dev), torch.zeros(len(chunks) * mx, device=dev)
    bs.index_put_([dst], src_all[idx]), bt.index_put_([dst], tgt_all[idx]), bw.index_put_([dst], scores[idx])
    Ts = ref_procrustes(bs.view(len(chunks), mx, 3), bt.view(len(chunks), mx, 3), bw.view(len(chunks), mx))
    res = torch.linalg.norm(tgt_all.unsqueeze(0) - apply(Ts, src_all.unsqueeze(0)), dim=2)
    masks = res < radius
    cur = scores * masks[masks.sum(1).argmax()].float()
    T = ref_procrustes(src_all[None], tgt_all[None], cur[None])[0]
    for _ in range(steps - 1):
        cur = scores * (torch.linalg.norm(tgt_all - apply(T, src_all), dim=1) < radius).float()
        T = ref_procrustes(src_all[None], tgt_all[None], cur[None])[0]
    return T


def ref_forward(sp, tp, sm, tm, score, k, radius, threshold=0.05):
    s = torch.exp(score)
    row = torch.zeros_like(s, dtype=torch.bool).scatter_(2, s.topk(k, dim=2)[1], True)
    col = torch.zeros_like(s, dtype=torch.bool).scatter_(1, s.topk(k, dim=1)[1], True)
    m = row & col & (s > threshold) & sm[:, :, None] & tm[:, None, :]
    b, i, j = torch.nonzero(m, as_tuple=True)
    return ref_lgr(sp[b, i], tp[b, j], s[b, i, j], b, radius)


def ref_sc(src, tgt, sigma):
    d = (torch.cdist(src, src) - torch.cdist(tgt, tgt)).abs()
    return torch.relu(1.0 - d.pow(2) / sigma ** 2)


def ref_power(mat, iters=10):
    v = torch.ones_like(mat[:, :1])
    last = v
    for _ in range(iters):
        v = torch.nn.functional.normalize(mat @ v, p=2, dim=0)
        if torch.allclose(v, last):
            break
        last = v
    return v[:, 0]


def alternate(fa, fb, runs):
    ev = lambda: torch.cuda.Event(enable_timing=True)
    ta, tb = [], []
    for f in (fa, fb, fa, fb):
        f()
    torch.cuda.synchronize()
    for _ in range(runs):
        for f, acc in ((fa, ta), (fb, tb)):
            a, b = ev(), ev()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            acc.append(a.elapsed_time(b))
    st = lambda t: dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)))
    return st(ta), st(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lgr_time.jsonl"))
    a = ap.parse_args()
    from diffreg_hip import registration as G
    from tests import lgr_ref as R
    rng = np.random.default_rng(0)
    patches = [int(rng.integers(8, 40)) * (-1 if rng.uniform() < 0.3 else 1) for _ in range(256)]
    sc = R.make_scene(("time", 64, patches, dict(k=3), 0), 1)
    cu = lambda x: torch.from_numpy(x).cuda()
    sp, tp, sm, tm, score, gs = [cu(sc[k]) for k in ("src_knn_points", "tgt_knn_points", "src_masks", "tgt_masks", "score_mat", "global_scores")]
    mod = G.LocalGlobalRegistration(3, 0.1)
    rows = []

    def record(name, fa, fb, **kw):
        da, db = alternate(fa, fb, a.runs)
        rows.append(dict(name=name, device=da, baseline=db, **kw))
        print("%-28s device %.3f ms (%.3f - %.3f)   baseline %.3f ms (%.3f - %.3f)" % (name, da["median_ms"], da["p10_ms"], da["p90_ms"],
                                                                                       db["median_ms"], db["p10_ms"], db["p90_ms"]))
    src_c, tgt_c, w_c, _ = mod(sp, tp, sm, tm, score, gs)
    n = int(w_c.shape[0])
    record("lgr_forward_256x64x64", lambda: mod(sp, tp, sm, tm, score, gs, padded=True), lambda: ref_forward(sp, tp, sm, tm, score, 3, 0.1),
           correspondences=n)
    b, i, j, w, _, _ = R.extract(sc["score_mat"], 3, sc["src_masks"], sc["tgt_masks"], sc["global_scores"])
    s1, t1, w1, b1 = cu(sc["src_knn_points"][b, i]), cu(sc["tgt_knn_points"][b, j]), cu(w), cu(b)
    s8, t8, w8, b8 = s1.repeat(8, 1), t1.repeat(8, 1), w1.repeat(8), b1.repeat(8).to(torch.int32)
    off = torch.arange(9, device="cuda", dtype=torch.int32) * len(b)
    record("lgr_pairs_8_in_one_call", lambda: G.local_to_global_registration_pairs(s8, t8, w8, b8, off, 0.1),
           lambda: [ref_lgr(s1, t1, w1, b1, 0.1) for _ in range(8)], correspondences=len(b))
    N = 5000
    src = torch.rand(N, 3, device="cuda") * 2 - 1
    tgt = src + 0.02 * torch.randn(N, 3, device="cuda")
    tgt[N // 2:] = torch.rand(N - N // 2, 3, device="cuda") * 2 - 1
    record("sc_row_sums_5000", lambda: G.spatial_consistency_counts(src, tgt, 0.1), lambda: ref_sc(src, tgt, 0.1).sum(1))
    record("sc_power_10_5000", lambda: G.leading_eigenvector(src, tgt_points=tgt, sigma=0.1, num_iterations=10),
           lambda: ref_power(ref_sc(src, tgt, 0.1), 10))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
