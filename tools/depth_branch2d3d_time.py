"""Time the depth branch of the 2D-3D front end, from the image on the device to the depth map, on one GPU.

    python tools/depth_branch2d3d_time.py [--runs 30] [--warmup 3] [--depth 24] [--source 480 640] [--out FILE.json]

ViT-L/14 (D = 1024, 16 heads, 24 blocks) and the production DPT head (256 features) with random float32 weights, one 480 x 640 x 3 image ->
476 x 630.  Three paths over the SAME bound depth model (device encoder + device head), alternated, 30 runs after warm-up, device-synchronised
host clock; median and p10 - p90:

  (a) host_transform  the reference-shaped path of EXP/model.py:339-342: device-to-host copy, the transform on the host, host-to-device copy, the
                      depth model.  The host transform is cv2.resize(INTER_CUBIC) when cv2 happens to be importable, otherwise torch's CPU
                      bicubic; both are followed by the float64 numpy normalisation.  `host_transform` in the result says which one ran.
  (b) engine_eager    DepthBranch2D3D(image): the transform launch, then encoder and head, launch by launch
  (c) engine_graph    DepthBranch2D3D(image, graph=True): the copy into the static buffer and one graph replay
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
import torch.nn.functional as F  # noqa: E402

from diffreg_hip.depth_branch2d3d import DepthBranch2D3D  # noqa: E402
from diffreg_hip.depth_transform2d3d import MEAN, STD, DeviceTransform  # noqa: E402
from tests import depth_encoder2d3d_ref as R  # noqa: E402
from tests import dpt2d3d_ref as DR  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--source", type=int, nargs=2, default=[480, 640])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("depth_branch2d3d_time: needs a GPU (a CPU run says nothing about the device)")
    dev = "cuda:0"
    Hs, Ws = a.source
    with torch.device(dev):
        vit = R.ViTF32(patch_size=14, img_size=518, embed_dim=1024, depth=a.depth, num_heads=16, mlp_ratio=4)
        P = DR.PRODUCTION
        head = DR.DPTHead(P["in_channels"], P["features"], P["out_channels"])
    R.draw_weights(vit, seed=1)
    head.load_state_dict(DR.draw_weights(head, DR.WEIGHT_SEED, device=dev))
    dm = R.DepthModelStandIn(vit.float(), head.float()).to(dev).eval()
    transform = DeviceTransform()
    branch = DepthBranch2D3D(dm, transform=transform)
    image = torch.rand(Hs, Ws, 3, device=dev)
    w, h = transform.size(Ws, Hs)
    try:
        import cv2
        host_name = "cv2.INTER_CUBIC"
        resize = lambda img: cv2.resize(img, (w, h), interpolation=cv2.INTER_CUBIC)
    except ImportError:
        host_name = "torch CPU bicubic"
        resize = lambda img: F.interpolate(torch.from_numpy(img).permute(2, 0, 1)[None], size=(h, w), mode="bicubic",
                                           align_corners=False)[0].permute(1, 2, 0).numpy()
    mean, std = np.array(MEAN), np.array(STD)

    def run_host():
        img = image.cpu().numpy()
        img = (resize(img) - mean) / std
        img = np.ascontiguousarray(np.transpose(img, (2, 0, 1))).astype(np.float32)
        with torch.no_grad():
            return dm(torch.from_numpy(img).unsqueeze(0).cuda())

    paths = (("host_transform", run_host), ("engine_eager", lambda: branch(image)), ("engine_graph", lambda: branch(image, graph=True)))
    for _ in range(a.warmup):
        for _, fn in paths:
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in paths}
    for _ in range(a.runs):
        for name, fn in paths:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) * 1e3)
    eager, host = branch(image).clone(), run_host()
    res = {"tool": "depth_branch2d3d_time", "source": [Hs, Ws], "network_input": [h, w], "depth": a.depth, "runs": a.runs, "host_transform": host_name,
           "graph_equals_eager": bool(torch.equal(branch(image, graph=True), eager)),
           "max_abs_diff_engine_vs_host_path": (eager - host).abs().max().item(), "max_abs_depth": host.abs().max().item()}
    for name, v in t.items():
        v = np.array(v)
        res[name + "_ms"] = {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
