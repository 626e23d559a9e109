"""Time the 2D-3D point backbone on the device (diffreg_hip/pcd_backbone2d3d.py) against the same module in plain PyTorch float32 on the same GPU
(the test suite's restatement, tests/pcd_backbone2d3d_ref.py; the reference tree is not needed), on scene "a" (20 000 points at level 0).

    python tools/pcd_backbone2d3d_time.py [--runs 30] [--warmup 5] [--out FILE.json]

Modes: the eval forward (torch.no_grad) and forward + backward of loss = sum_i <out_i, w_i>.  Each run is timed by a host clock between two device
synchronisations; device and baseline runs alternate.  Prints median and p10-p90 per mode and path, and one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "diff-reg_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from diffreg_hip import pcd_backbone2d3d as P
    from tests import pcd_backbone2d3d_ref as R
    dev = "cuda:0"
    pyr = R.to_torch(R.make_pyramid("a"), dev)
    m = R.PointBackbone()
    m.load_state_dict({**m.state_dict(), **R.make_weights(m)})
    m = m.to(dev)
    feats = torch.ones(pyr["points"][0].shape[0], 1, device=dev)
    ws = None

    def run(path, mode):
        nonlocal ws
        fwd = (lambda: P.point_backbone(m, feats, pyr)) if path == "device" else (lambda: m(feats, pyr))
        if mode == "eval":
            with torch.no_grad():
                return fwd()
        m.zero_grad(set_to_none=True)
        outs = fwd()
        if ws is None:
            ws = [torch.as_tensor(w, dtype=torch.float32, device=dev) for w in R.loss_weights(outs)]
        sum((o * w).sum() for o, w in zip(outs, ws)).backward()

    res = {}
    for mode in ("eval", "train"):
        times = {"device": [], "torch": []}
        for i in range(a.warmup + a.runs):
            for path in ("device", "torch"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(path, mode)
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times[path].append((time.perf_counter() - t0) * 1e3)
        for path, t in times.items():
            t = np.array(t)
            res["%s_%s" % (mode, path)] = dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)),
                                              min_ms=float(t.min()), runs=len(t))
            print("%-5s %-6s median %8.3f ms  p10-p90 %8.3f - %8.3f" % (mode, path, np.median(t), np.percentile(t, 10), np.percentile(t, 90)))
    line = json.dumps(dict(tool="pcd_backbone2d3d_time", points=int(feats.shape[0]), **res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
