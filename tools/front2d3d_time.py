"""Time the geometry head and the feature-layout glue of the 2D-3D forward on one GPU:

    python tools/front2d3d_time.py [--out FILE.json]

Method of DESIGN 5f-5k: 5 warm-up runs, then 30 runs alternating the two sides, each between two device synchronisations; median [p10-p90] in
milliseconds; the device path against the same operations in PLAIN PyTorch on the same GPU (the reference's statements, restated here: nothing is
read from the reference).  Every item runs in a child process of its own under its own time limit; the first one that fails ends the run.  Items:
 geometry          back_project + create_meshgrid().float() + render + back_project_depth at 480 x 640 with 20 000 points (EXP/model.py:306-351)
 resize_fwd / _fb  resize_tokens 512 x 60 x 80 -> 34 x 45, forward and forward + backward (:374-375)
 norm_fwd          rows_normalized 128 x 480 x 640 forward (:535-538), with the achieved bytes/s against the 2 x 157 MB it has to move
 norm_dense_fb     forward + backward of a dense [307 200, 128] gradient
 norm_sparse_fb    forward + backward of K = 1 024 gradient rows: rows_normalized(x, rows=idx) against torch's normalize + index_select"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
ITEMS = {"geometry": 120, "resize_fwd": 120, "resize_fb": 120, "norm_fwd": 180, "norm_dense_fb": 180, "norm_sparse_fb": 180}   # seconds


def measure(sides, warm=5, runs=30):
    import torch
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


def torch_back_project(depth, K, z_of, limit):
    fx, fy, cx, cy = K[..., 0:1, 0:1], K[..., 1:2, 1:2], K[..., 0:1, 2:3], K[..., 1:2, 2:3]
    _, h, w = depth.shape
    coords = torch_mod.arange(h * w).view(h, w).to(depth.device).unsqueeze(0).expand_as(depth)
    u, v = coords % w, torch_mod.div(coords, w, rounding_mode="floor")
    z = z_of(depth)
    z.masked_fill_(torch_mod.gt(z, limit), 0.0)
    return torch_mod.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], dim=-1), torch_mod.gt(z, 0.0)


def torch_render(p, K, T, eps=1e-8):
    p = torch_mod.matmul(p, T[:3, :3].transpose(-1, -2)) + T[None, :3, 3]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    w = K[0, 0].unsqueeze(-1) * x / z.clamp(min=eps) + K[0, 2].unsqueeze(-1)
    h = K[1, 1].unsqueeze(-1) * y / z.clamp(min=eps) + K[1, 2].unsqueeze(-1)
    return torch_mod.stack([h, w], dim=-1)


def run_item(item):
    import torch
    import torch.nn.functional as TF
    global torch_mod
    torch_mod = torch
    from diffreg_hip import front2d3d as fr, lib
    gen = torch.Generator().manual_seed(3)
    if item == "geometry":
        H, W, N = 480, 640, 20000
        depth = (torch.rand(1, H, W, generator=gen) * 7000).round().to(DEV)
        depth_da = (torch.rand(1, H, W, generator=gen) * 0.08).to(DEV)
        K = torch.tensor([[[585.0, 0.0, 320.0], [0.0, 585.0, 240.0], [0.0, 0.0, 1.0]]], device=DEV)
        T = torch.eye(4, device=DEV)
        T[:3, 3] = torch.tensor([0.1, -0.2, 0.3])
        pts = (torch.rand(N, 3, generator=gen) * 2 + 0.5).to(DEV)
        a, b = torch.tensor(73.5, device=DEV), torch.tensor(0.25, device=DEV)

        def torch_side():
            p, m = torch_back_project(depth, K, lambda d: d / 1000.0, 6.0)
            pix = torch.cartesian_prod(torch.arange(H).cuda(), torch.arange(W).cuda()).view(H, W, 2).float()
            r = torch_render(pts, K[0], T)
            pd, md = torch_back_project(depth_da, K, lambda d: d * a + b, 6.0)
            return p, m, pix, r, pd, md

        def device_side():
            p, m = fr.back_project(depth, K, depth_limit=6.0, transposed=True, return_mask=True)
            pix = fr.create_meshgrid(H, W).float()
            r = fr.render(pts, K[0], extrinsics=T, rounding=False)
            pd, md = fr.back_project_depth(depth_da, K, scaling_factor_a=a, scaling_factor_b=b, depth_limit=6.0, transposed=True, return_mask=True)
            return p, m, pix, r, pd, md

        def device_fused_side():                     # the pixel grid from the back-projection's own pass instead of create_meshgrid
            p, m, pix = lib.back_project_points(depth[0], K[0], depth_limit=6.0, pixels=True)
            r = fr.render(pts, K[0], extrinsics=T, rounding=False)
            pd, md = fr.back_project_depth(depth_da, K, scaling_factor_a=a, scaling_factor_b=b, depth_limit=6.0, transposed=True, return_mask=True)
            return p, m, pix, r, pd, md

        x, y = torch_side(), device_side()
        assert torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) and torch.allclose(x[0], y[0], rtol=1e-5, atol=1e-6)
        assert torch.allclose(x[3], y[3], rtol=1e-4, atol=1e-3) and torch.allclose(x[4], y[4], rtol=1e-5, atol=1e-6)
        return measure({"torch": torch_side, "device": device_side, "device_fused_pixels": device_fused_side})
    if item in ("resize_fwd", "resize_fb"):
        x = torch.randn(1, 512, 60, 80, generator=gen).to(DEV).requires_grad_(True)
        g = torch.randn(34 * 45, 512, generator=gen).to(DEV)
        tf = lambda: TF.interpolate(x, size=(34, 45), mode="bilinear", align_corners=True).squeeze(0).view(-1, 34 * 45).transpose(0, 1).clone()
        df = lambda: fr.resize_tokens(x, (34, 45))
        assert torch.allclose(tf(), df(), rtol=1e-5, atol=1e-5)
        if item == "resize_fwd":
            with torch.no_grad():
                return measure({"torch": tf, "device": df})
        return measure({"torch": lambda: torch.autograd.grad(tf(), x, g), "device": lambda: torch.autograd.grad(df(), x, g)})
    C, H, W = 128, 480, 640
    x = torch.randn(1, C, H, W, generator=gen).to(DEV).requires_grad_(True)
    tf = lambda: TF.normalize(x.squeeze(0).view(C, -1).transpose(0, 1).contiguous(), p=2, dim=1)
    df = lambda: fr.rows_normalized(x)
    assert torch.allclose(tf(), df(), rtol=1e-5, atol=1e-6)
    if item == "norm_fwd":
        with torch.no_grad():
            r = measure({"torch": tf, "device": df})
        moved = 2 * C * H * W * 4
        r["device"]["bytes_moved_minimum"] = moved
        r["device"]["achieved_bytes_per_s"] = moved / (r["device"]["median"] * 1e-3)
        return r
    if item == "norm_dense_fb":
        g = torch.randn(H * W, C, generator=gen).to(DEV)
        return measure({"torch": lambda: torch.autograd.grad(tf(), x, g), "device": lambda: torch.autograd.grad(df(), x, g)})
    rows = torch.randint(0, H * W, (1024,), generator=gen).to(DEV)
    gk = torch.randn(1024, C, generator=gen).to(DEV)
    return measure({"torch": lambda: torch.autograd.grad(tf().index_select(0, rows), x, gk),
                    "device": lambda: torch.autograd.grad(fr.rows_normalized(x, rows=rows)[1], x, gk)})


def main():
    if "--item" in sys.argv:
        print("RESULT " + json.dumps(run_item(sys.argv[sys.argv.index("--item") + 1])))
        return 0
    res = {}
    for item, limit in ITEMS.items():
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--item", item], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping" % (item, limit))
            return 1
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print("%s: exit status %d; stopping\n%s" % (item, p.returncode, p.stderr[-2000:]))
            return 1
        res[item] = json.loads(line[0][len("RESULT "):])
        extra = res[item]["device"].get("achieved_bytes_per_s")
        print("%-16s" % item, "  ".join("%s %.3f [%.3f-%.3f] ms" % (s, r["median"], r["p10"], r["p90"]) for s, r in res[item].items()),
              "" if extra is None else "  %.2f TB/s of the 2-pass minimum" % (extra / 1e12), flush=True)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
