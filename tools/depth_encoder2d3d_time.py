"""Time Depth-Anything's float32 ViT-L/14 encoder forward on the device against plain PyTorch-ROCm float32 on the same GPU.

    python tools/depth_encoder2d3d_time.py [--runs 30] [--warmup 5] [--depth 24] [--size 476 630] [--tile T] [--out FILE.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/depth_encoder2d3d_time.py --profile      # per-kernel times, in a run of its own

ViT-L/14 (D = 1024, 16 heads, 24 blocks, hidden 4096), random float32 weights drawn on the device, one 476 x 630 image (1531 tokens).
DeviceViTF32.get_intermediate_layers(x, 4, return_class_token=True) against the restatement's float32 call (tests/depth_encoder2d3d_ref.ViTF32:
torch's hipBLASLt GEMMs and eager attention), 30 alternated runs after warm-up, device-synchronised host clock; median and p10 - p90.  The GEMM
line: FLOPs of the five linear layers counted from the shapes over the device path's whole time is a LOWER bound of the GEMM kernels' rate; the
kernels' own rates come from the profile run.  --tile forces one rows-GEMM tile (dr_debug_gemm_rows_f32_tile) for the tile rule's record.
--profile runs only the device path (3 forwards) so that the trace holds nothing else."""
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

from diffreg_hip import depth_encoder2d3d, lib  # noqa: E402
from tests import depth_encoder2d3d_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--size", type=int, nargs=2, default=[476, 630])
    ap.add_argument("--tile", type=int, default=-1)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_encoder2d3d_time: needs a GPU (a CPU run says nothing about the device)")
    dev = "cuda:0"
    H, W = a.size
    with torch.device(dev):
        vit = R.ViTF32(patch_size=14, img_size=518, embed_dim=1024, depth=a.depth, num_heads=16, mlp_ratio=4)
    R.draw_weights(vit, seed=1)
    vit = vit.float().eval()
    x = torch.randn(1, 3, H, W, device=dev)
    dv = depth_encoder2d3d.DeviceViTF32(vit)
    lib.ensure_init()
    lib.raw().dr_debug_gemm_rows_f32_tile(a.tile)

    def run_dev():
        with torch.no_grad():
            return dv.get_intermediate_layers(x, 4, return_class_token=True)

    def run_torch():
        with torch.no_grad():
            return vit.get_intermediate_layers(x, 4, return_class_token=True)

    if a.profile:
        for _ in range(3):
            run_dev()
        torch.cuda.synchronize()
        return
    for _ in range(a.warmup):
        run_dev(); run_torch()
    torch.cuda.synchronize()
    t = {"device": [], "torch_fp32": []}
    for _ in range(a.runs):
        for name, fn in (("device", run_dev), ("torch_fp32", run_torch)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3)
    d, r = run_dev(), run_torch()
    dif = max((p[0] - q[0]).abs().max().item() for p, q in zip(d, r))
    L, D, Dh = 1 + (H // 14) * (W // 14), 1024, 4096
    gemm_flop = 2.0 * ((L - 1) * 608 * D + a.depth * L * (D * 3 * D + D * D + 2 * D * Dh))
    attn_flop = a.depth * 4.0 * L * L * D
    res = {"tool": "depth_encoder2d3d_time", "tile": a.tile, "image": [H, W], "tokens": L, "depth": a.depth, "runs": a.runs,
           "gemm_tflop": gemm_flop / 1e12, "attention_tflop": attn_flop / 1e12, "max_abs_diff_device_vs_torch_fp32": dif}
    for name, v in t.items():
        v = np.array(v)
        res[name + "_ms"] = {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}
    med = res["device_ms"]["median"] * 1e-3
    res["device_over_torch"] = res["device_ms"]["median"] / res["torch_fp32_ms"]["median"]
    res["device_whole_forward_gemm_flops_fraction_of_157.3TF"] = gemm_flop / med / 157.3e12
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
