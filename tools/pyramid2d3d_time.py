"""Time the 2D-3D graph pyramid: the device path (diffreg_hip/pyramid2d3d.py) against the numpy float64 restatement of the loader's pyramid
(tests/pcd_backbone2d3d_ref.build_pyramid) and, where scipy imports, against the same restatement with a cKDTree radius search.

    python tools/pyramid2d3d_time.py [--points 20000] [--runs 30]      -> one JSON line

Scene "a" of tests/partition2d3d_ref.make_scene (20 000 points), 4 stages, LIMITS of tests/pcd_backbone2d3d_ref.py.  The paths are run alternately,
`runs` times each after one warm-up; medians and [min, max] in ms.  The device time includes its host synchronisations (one per data-dependent shape)
and excludes the upload of the points.  Neither CPU path is the reference's compiled extension (a kd-tree in C++): they are what this repository can
run anywhere, and the JSON line names them so."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)


def ckdtree_pyramid(points, B):
    from scipy.spatial import cKDTree

    def search(q, s, radius, limit):
        tree = cKDTree(s.astype(np.float64))
        rows = tree.query_ball_point(q.astype(np.float64), radius, return_sorted=False)
        out = np.full((len(q), limit), len(s), np.int64)
        width = 1
        for i, r in enumerate(rows):
            r = np.asarray(r, dtype=np.int64)
            d2 = ((s[r].astype(np.float64) - q[i].astype(np.float64)) ** 2).sum(1)
            keep = d2 < radius * radius
            r, d2 = r[keep], d2[keep]
            r = r[np.lexsort((r, d2))][:limit]
            out[i, :len(r)] = r
            width = max(width, len(r))
        return out[:, :width]
    pts = [np.ascontiguousarray(points, dtype=np.float32)]
    for i in range(1, B.NUM_STAGES):
        pts.append(B.grid_subsample(pts[-1], B.VOXEL * 2 ** i))
    nb, sub, up = [], [], []
    for i in range(B.NUM_STAGES):
        r = B.RADIUS * 2 ** i
        nb.append(search(pts[i], pts[i], r, B.LIMITS[i]))
        if i < B.NUM_STAGES - 1:
            sub.append(search(pts[i + 1], pts[i], r, B.LIMITS[i]))
            up.append(search(pts[i], pts[i + 1], 2 * r, B.LIMITS[i + 1]))
    return dict(points=pts, neighbors=nb, subsampling=sub, upsampling=up)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--runs", type=int, default=30)
    a = ap.parse_args()
    import torch
    from diffreg_hip import pyramid2d3d as P
    from tests import pcd_backbone2d3d_ref as B
    points = B.scene_points("a")[:a.points]
    dev_points = torch.from_numpy(points).cuda()
    lengths = torch.tensor([len(points)], device="cuda")

    def device():
        P.build_grid_and_radius_graph_pyramid_pack_mode(dev_points, lengths, B.NUM_STAGES, B.VOXEL, B.RADIUS, list(B.LIMITS))
        torch.cuda.synchronize()
    paths = {"device": device, "numpy_float64_restatement": lambda: B.build_pyramid(points)}
    try:
        import scipy  # noqa: F401
        paths["ckdtree_restatement"] = lambda: ckdtree_pyramid(points, B)
    except ImportError:
        pass
    times = {k: [] for k in paths}
    for rep in range(a.runs + 1):
        for k, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                times[k].append((time.perf_counter() - t0) * 1e3)
    out = {"points": len(points), "stages": B.NUM_STAGES, "runs": a.runs}
    for k, t in times.items():
        out[k + "_ms"] = {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
