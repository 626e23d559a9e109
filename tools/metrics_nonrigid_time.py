"""Time the non-rigid evaluation on one GPU against the same results in plain PyTorch float32 on that GPU:

    python tools/metrics_nonrigid_time.py [--runs 30] [--out profiles/metrics_nonrigid_time.jsonl]

Shapes: knn at 9 000 x 9 000 (k = 1, 3, 16) and 30 000 x 30 000 (k = 1), Chamfer at both sizes, evaluate_nonrigid_pairs for one and eight
pairs of 9 000 points.  Baseline: torch.cdist + topk over chunks of CHUNK query rows (the 30 000 x 30 000 float32 matrix is 3.6 GB; a chunk of
4 096 rows is 0.5 GB), nothing read back.  Each pair of timings alternates device / baseline run by run; median with p10 - p90 in
milliseconds.  The kernel's rate is distance evaluations per second against the float32 vector rate of the part (256 compute units x 128
lanes x 2.4 GHz = 78.6e12 lane operations per second, one multiply or add each; a distance evaluation is 8 of them plus its compare)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
CHUNK = 4096
VALU_LANE_OPS = 256 * 128 * 2.4e9


def torch_knn(q, s, k):
    d, i = [], []
    for lo in range(0, q.shape[0], CHUNK):
        dd, ii = torch.cdist(q[lo:lo + CHUNK], s).topk(k, dim=1, largest=False)
        d.append(dd)
        i.append(ii)
    return torch.cat(d), torch.cat(i)


def torch_chamfer(q, s):
    return torch_knn(q, s, 1)[0].mean() + torch_knn(s, q, 1)[0].mean()


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_nonrigid_time.jsonl"))
    a = ap.parse_args()
    from diffreg_hip import metrics_nonrigid as M
    g = torch.Generator().manual_seed(1)
    cloud = lambda n: (torch.rand(n, 3, generator=g) * 2 - 1).cuda()
    rows = []

    def record(name, dev_fn, ref_fn, pairs=None):
        d, r = alternate(dev_fn, ref_fn, a.runs)
        row = dict(name=name, runs=a.runs, device=d, torch_float32=r, torch_chunk_rows=CHUNK, device_over_torch=d["median_ms"] / r["median_ms"])
        if pairs:
            row["distance_evaluations_per_s"] = pairs / (d["median_ms"] * 1e-3)
            row["share_of_f32_valu_rate"] = row["distance_evaluations_per_s"] * 9 / VALU_LANE_OPS
        rows.append(row)
        print(json.dumps(row), flush=True)

    for n, ks in ((9000, (1, 3, 16)), (30000, (1,))):
        q, s = cloud(n), cloud(n)
        for k in ks:
            dd, di, _ = M.knn_points(q, s, k)
            td, ti = torch_knn(q, s, k)
            assert float((dd - td).abs().max()) < 1e-3      # cdist's float32 matrix form is the looser of the two
            record("knn %d x %d k=%d" % (n, n, k), lambda: M.knn_points(q, s, k), lambda: torch_knn(q, s, k), pairs=float(n) * n)
        record("chamfer %d x %d" % (n, n), lambda: M.compute_chamfer_distance(q, s), lambda: torch_chamfer(q, s), pairs=2.0 * n * n)
    for P in (1, 8):
        src = [cloud(9000) for _ in range(P)]
        flow = [0.05 * cloud(9000) for _ in range(P)]
        tgt = [x + f for x, f in zip(src, flow)]
        warped = [t + 0.01 * cloud(9000) for t in tgt]
        kw = dict(strict=(0.025, 0.025), relaxed=(0.05, 0.05), outlier=(0.3, 0.1))

        def ref():
            out = []
            for x, w, f, t in zip(src, warped, flow, tgt):
                e = torch.linalg.norm((w - x) - f, dim=1)
                rel = e / (torch.linalg.norm(f, dim=1) + 1e-20)
                out += [e.mean(), ((e < 0.025) | (rel < 0.025)).float().mean(), ((e < 0.05) | (rel < 0.05)).float().mean(),
                        ((e > 0.3) | (rel > 0.1)).float().mean(), torch_chamfer(w, t)]
            return torch.stack(out)
        record("evaluate_nonrigid_pairs %d x 9000" % P, lambda: M.evaluate_nonrigid_pairs(src, warped, flow, tgt, **kw), ref)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
