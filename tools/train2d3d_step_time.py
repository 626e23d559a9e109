"""Time of the differentiable 2D-3D training step -- both CrossModalFusionModules, both matching heads, the coarse loss (circle + focal),
forward + (loss_circle + loss_matrix_gt_hat).backward() -- at N = 1024 point nodes, M = 34 x 45 = 1530 image tokens, on the device path
(overlay2d3d.accelerate(training=True) + accelerate_loss) and on PyTorch-ROCm, alternating the two, after warm-up, each step between two device
synchronisations.  Prints one JSON line: per path median / p10 / p90 / min in ms over --steps steps.

The PyTorch baseline is tests/train2d3d_ref.py un-overlaid, float32: the test suite's plain-torch restatement of the reference's modules and loss
(it reproduces the reference's own forward and backward: tests/test_train2d3d_oracle.py), including the mutual top-1 read-out of both heads
(torch arg-maxima), so that both paths do the same work.  The reference's own modules need its checkout, which this tool does not assume.

    python tools/train2d3d_step_time.py --steps 30 --warmup 5
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/train2d3d_step_time.py --device-only --steps 10 --warmup 3
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import train2d3d_ref as R  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--M", type=int, default=1530)
    ap.add_argument("--device-only", action="store_true", help="time the device path alone (for a kernel trace)")
    a = ap.parse_args()
    from diffreg_hip.overlay2d3d import accelerate, accelerate_loss
    host = R.load_synth(R.HostTrain2D3D())
    b = R.batch_to(R.make_batch(a.N, a.M, 32), DEV, torch.float32)
    dev_host, dev_loss = R.clone_as(host, torch.float32, DEV).train(), R.CoarseMatchingLoss()
    accelerate(dev_host, training=True)
    accelerate_loss(dev_loss)
    paths = {"device": (dev_host, dev_loss)}
    if not a.device_only:
        paths["torch"] = (R.clone_as(host, torch.float32, DEV).train(), R.CoarseMatchingLoss())
    times = {k: [] for k in paths}
    for it in range(a.warmup + a.steps):
        for name, (h, lm) in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            R.run_step(h, lm, b)
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    out = dict(N=a.N, M=a.M, steps=a.steps, warmup=a.warmup)
    for k, v in times.items():
        v = np.asarray(v)
        out[k + "_ms"] = dict(median=round(float(np.median(v)), 3), p10=round(float(np.percentile(v, 10)), 3),
                              p90=round(float(np.percentile(v, 90)), 3), min=round(float(v.min()), 3))
    if "torch" in times:
        out["speedup_median"] = round(float(np.median(times["torch"]) / np.median(times["device"])), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
