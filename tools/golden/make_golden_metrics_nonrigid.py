"""Mint the fixture of the non-rigid evaluation by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_metrics_nonrigid.py REFERENCE_ROOT     # the directory holding Diff-Reg-2d3d/; writes tests/golden/metrics_nonrigid.npz

The reference's own knn (vision3d/ops/knn.py:30-107), knn_interpolate (vision3d/ops/knn_interpolate.py:10-40) and its six non-rigid metrics
(vision3d/ops/metrics.py:258-372) are imported from where they lie and run on the scenes of tests/metrics_nonrigid_ref.make_scene, once in
float32 and once in float64.  Only reference OUTPUTS are stored, next to the inputs, and per float array the float32 run's deviation from
float64.

Imports need the stubs the other mint tools use (MagicMock for open3d, pykeops, vision3d.ext, ...).  ONE SHIM, unavoidable without pykeops:
keops_knn (in vision3d.ops.knn and vision3d.ops.knn_interpolate) is replaced by a FLOAT64 brute-force kNN with a stable sort (ascending by
distance, by index on ties), whatever the precision of the run -- parity with KeOps itself is NOT claimed.

Every scene is regenerated until it passes both screens (none is passed by dropping queries): every gap between consecutive sorted float64
distances of a query through position k + 1 is exactly 0 (duplicated supports, put in on purpose) or at least 1e-5, and no |e|, rel or
neighbour distance lies within 1e-5 of a threshold it is compared with.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "metrics_nonrigid.npz")
sys.path.insert(0, ROOT)


def main(ref_root):
    import torch
    for m in ("vision3d.ext", "ipdb", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops"):
        sys.modules[m] = MagicMock()
    sys.path.insert(0, os.path.join(ref_root, "Diff-Reg-2d3d"))
    import vision3d.ops  # noqa: F401
    kn = sys.modules["vision3d.ops.knn"]
    ki = sys.modules["vision3d.ops.knn_interpolate"]
    mt = sys.modules["vision3d.ops.metrics"]
    from tests import metrics_nonrigid_ref as R

    def knn64(q_points, s_points, k):
        q, s = q_points.double(), s_points.double()
        d = (q[:, None, :] - s[None]).pow(2).sum(-1).sqrt()
        idx = torch.argsort(d, dim=1, stable=True)[:, :k].contiguous()
        return torch.gather(d, 1, idx).to(q_points.dtype), idx
    kn.keops_knn = knn64
    ki.keops_knn = knn64

    def run(sc, dtype):
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
        q, s, feats, T = t(sc["q"]), t(sc["s"]), t(sc["feats"]), t(sc["transform"])
        flow, pred, tgt_c, s_moved = t(sc["flow"]), t(sc["pred"]), t(sc["tgt_c"]), t(sc["s_moved"])
        test = torch.from_numpy(sc["test"])
        out = {}
        for tag, kw in R.KNN_CASES:
            out["knn_%s_dist" % tag], out["knn_%s_idx" % tag] = kn.knn(q, s, return_distance=True, **kw)
        out["interp"] = ki.knn_interpolate(q, s, feats, k=3)
        out["interp_limit"] = ki.knn_interpolate(q, s, feats, k=3, distance_limit=R.INTERP_LIMIT)
        out["nir"] = mt.compute_nonrigid_inlier_ratio(q, tgt_c, flow, T, R.RADIUS)
        out["nir_no_transform"] = mt.compute_nonrigid_inlier_ratio(q, tgt_c, flow, None, R.RADIUS)
        out["nfmr"] = mt.compute_nonrigid_feature_matching_recall(s, s_moved, q, flow, test, T, R.RADIUS, R.NFMR_LIMIT)
        out["acc_strict"] = mt.compute_scene_flow_accuracy(pred, flow, *R.STRICT)
        out["acc_relaxed"] = mt.compute_scene_flow_accuracy(pred, flow, *R.RELAXED)
        out["outlier"] = mt.compute_scene_flow_outlier_ratio(pred, flow, *R.OUTLIER)
        out["outlier_none"] = mt.compute_scene_flow_outlier_ratio(pred, flow, *R.OUTLIER_NONE)
        out["coverage"] = mt.compute_corr_coverage(q, s, R.COVERAGE_LIMIT)
        out["chamfer"] = mt.compute_chamfer_distance(q, s)
        out["chamfer_squared"] = mt.compute_chamfer_distance(q, s, squared=True)
        out["epe"] = torch.linalg.norm(pred - flow, dim=1).mean()       # metrics.py:330 averaged: the end-point error
        return {k: v.detach().numpy().astype(np.int64 if v.dtype == torch.int64 else np.float64) for k, v in out.items()}

    res = {}
    for name, Q, S, dup in R.SCENES:
        for attempt in range(20000):
            sc = R.make_scene(name, attempt)
            gap = R.screen_gaps(sc["q"], sc["s"])
            if gap < R.SCREEN_GAP:
                continue
            margin = R.screen_thresholds(sc)
            if margin < R.SCREEN_GAP:
                continue
            r64, r32 = run(sc, torch.float64), run(sc, torch.float32)
            if all(np.array_equal(v, r32[k]) for k, v in r64.items() if v.dtype == np.int64):
                break
        else:
            raise SystemExit("scene %s: no attempt passed the screens" % name)
        worst = 0.0
        for k, v in r64.items():
            res["%s/%s" % (name, k)] = v.astype(np.int32) if v.dtype == np.int64 else v
            if v.dtype != np.int64:
                dev = np.abs(r32[k] - v)
                res["%s/%s_dev32" % (name, k)] = dev.astype(np.float32)
                worst = max(worst, float(dev.max(initial=0.0)))
        for k, v in sc.items():
            res["%s/in_%s" % (name, k)] = v
        res["%s/screens" % name] = np.array([gap, margin, attempt], np.float64)
        print("scene %s: Q %d, S %d, %d duplicated supports; attempt %d; smallest non-zero gap %.2e, threshold margin %.2e; float32 within %.2e"
              % (name, Q, S, dup, attempt, gap, margin, worst))
    res["provenance"] = np.array("reference functions (vision3d.ops.knn, knn_interpolate, metrics.py:258-372) run on the CPU in float32 and float64; "
                                 "keops_knn replaced by a float64 brute-force kNN with a stable sort (pykeops absent): parity with KeOps itself is "
                                 "not claimed")
    np.savez_compressed(OUT, **res)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main(sys.argv[1])
