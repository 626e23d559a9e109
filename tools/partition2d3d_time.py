"""Time the patch partition / ground-truth overlap entries (csrc/partition2d3d.hip) on scene "a" of tests/partition2d3d_ref.py (476 x 630 image, 34 x 45
nodes, stride 2, 20 000 points, 1 024 nodes, point_limit 128) against the SAME functions in plain PyTorch on the same GPU: the float32 restatement of
tests/partition2d3d_ref.py with its dense k-NN (the reference itself needs KeOps and Open3D).

    python tools/partition2d3d_time.py [--calls 50] [--warmup 5] [--out FILE.json]

Per entry and for EXP/model.py:403-495 as a whole: median and p10-p90 of `calls` calls after `warmup`, each call timed by a host clock around work that ends
in a device synchronise (the wrappers' own host reads included: they are part of what a caller pays).  Prints a table and one JSON line."""
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
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from diffreg_hip import partition2d3d as P
    from tests import partition2d3d_ref as R
    dev = "cuda:0"
    sc = R.make_scene("a")
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sc.items()}
    keys = ("point_to_node", "node_sizes", "node_masks", "node_knn_indices", "node_knn_masks")
    f32 = torch.float32

    def dev_partition():
        return dict(zip(keys, P.point_to_node_partition(d["pcd_points"], d["nodes"], d["limit"], return_count=True, gather_points=True)))

    def dev_patchify():
        return P.patchify(d["img_points"], d["img_points_da"], d["img_pixels"], d["img_masks"], d["img_masks_da"], d["H"], d["W"], d["Hc"], d["Wc"], stride=d["stride"])

    def torch_partition():
        return R.partition(d["pcd_points"], d["nodes"], d["limit"], dtype=f32)

    def torch_patchify():
        return R.patchify(d["img_points"], d["img_points_da"], d["img_pixels"], d["img_masks"], d["img_masks_da"], d["H"], d["W"], d["Hc"], d["Wc"], d["stride"])

    part, patches = dev_partition(), dev_patchify()
    args = R.node_corr_inputs(d, part, dev, patches=patches)
    ra = R.reference_args(args)

    def dev_corr():
        return P.get_2d3d_node_correspondences(*ra)

    def torch_corr():
        o = R.ref_node_corr(args, dtype=f32, chunk=2048)
        return o, R.mutual_nn(o["pcd_centers"], o["img_centers"], R.R_MUTUAL, dtype=f32)

    out0 = dev_corr()
    pc, ic = out0[4], out0[5]

    def whole(partition, patchify, corr_from):
        def run():
            pt = partition()
            pa = patchify()
            return corr_from(R.node_corr_inputs(d, pt, dev, patches=pa))
        return run
    dev_whole = whole(dev_partition, dev_patchify, lambda ar: P.get_2d3d_node_correspondences(*R.reference_args(ar)))
    torch_whole = whole(torch_partition, torch_patchify, lambda ar: (R.ref_node_corr(ar, dtype=f32, chunk=2048),))
    cases = [
        ("point_to_node_partition", dev_partition, torch_partition),
        ("patchify", dev_patchify, torch_patchify),
        ("get_2d3d_node_correspondences", dev_corr, torch_corr),
        ("multual_nn_correspondence", lambda: P.multual_nn_correspondence(pc, ic, R.R_MUTUAL), lambda: R.mutual_nn(pc, ic, R.R_MUTUAL, dtype=f32)),
        ("get_correspondences r=0.06", lambda: P.get_correspondences(d["nodes"], ic, d["transform"], 0.06),
         lambda: R.radius_pairs(d["nodes"], ic, d["transform"], 0.06, dtype=f32)[0]),
        ("model.py:403-495 whole", dev_whole, torch_whole),
    ]

    def clock(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = np.array(ts)
        return [float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))]
    res = {}
    print("%-34s %28s %28s" % ("entry (ms: median [p10 - p90])", "libdiffreg_hip", "plain torch, same GPU"))
    for name, f_dev, f_torch in cases:
        td, tt = clock(f_dev), clock(f_torch)
        res[name] = dict(device_ms=td, torch_ms=tt)
        print("%-34s %10.3f [%7.3f - %7.3f] %10.3f [%7.3f - %7.3f]   x%.1f" % (name, *td, *tt, tt[0] / td[0]))
    n_cand = int(R.ref_node_corr(args, dtype=f32, chunk=2048)["cand_i"].shape[0])
    res["scene"] = dict(candidates=n_cand, pairs=int(out0[0].shape[0]), Ki=int(args["img_kp"].shape[1]), Kc=int(args["pcd_kp"].shape[1]), calls=a.calls)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
