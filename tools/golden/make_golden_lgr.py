"""Mint the fixture of the RANSAC-free rigid estimators by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_lgr.py REFERENCE_ROOT     # the directory holding Diff-Reg-2d3d/; writes tests/golden/lgr.npz

The reference's own LocalGlobalRegistration, weighted_procrustes, spatial_consistency, cross_spatial_consistency, SpatialConsistencyFiltering
and leading_eigenvector are imported from where they lie and run on the scenes of tests/lgr_ref.make_scene, once in float32 and once in
float64.  Only inputs, reference OUTPUTS and per float tensor the float32 run's deviation from the float64 run are stored.

What the import needs: the MagicMock stubs of the other mint tools plus IPython; torch.Tensor.cuda replaced by the identity (the reference
calls .cuda() on its index tensors); torch.set_default_dtype set to the run's precision (convert_to_batch and the eye of
weighted_procrustes allocate in the default dtype and fail in float64 otherwise).

Every scene is regenerated until it passes ALL screens of tests/lgr_ref.screens (none is passed by dropping correspondences; the share
left out is 0); the margins are printed and stored.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "lgr.npz")
sys.path.insert(0, ROOT)

PROVENANCE = ("reference outputs of Diff-Reg-2d3d vision3d (LocalGlobalRegistration, weighted_procrustes, spatial_consistency, "
              "cross_spatial_consistency, SpatialConsistencyFiltering, leading_eigenvector) run on the CPU in float32 and float64; "
              "import shims: MagicMock stubs (vision3d.ext, ipdb, open3d, cv2, easydict, pykeops, pytorch3d, IPython), torch.Tensor.cuda = "
              "identity, torch.set_default_dtype = the run's precision; scenes from tests/lgr_ref.py, screened, share left out 0")


def main(ref_root):
    import torch
    for m in ("vision3d.ext", "ipdb", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops", "IPython"):
        sys.modules[m] = MagicMock()
    sys.path.insert(0, os.path.join(ref_root, "Diff-Reg-2d3d"))
    torch.Tensor.cuda = lambda self, *a, **k: self
    import vision3d.ops as vops
    from vision3d.models.geotransformer.local_global_registration import LocalGlobalRegistration
    from vision3d.models.geotransformer.spatial_consistency_filtering import SpatialConsistencyFiltering
    from tests import lgr_ref as R

    def run(sc, dtype):
        torch.set_default_dtype(dtype)
        o = sc["opts"]
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
        lgr = LocalGlobalRegistration(o["k"], o["radius"], mutual=o["mutual"], confidence_threshold=o["threshold"], use_dustbin=o["use_dustbin"],
                                      use_global_score=o["use_global_score"], use_logits=o["use_logits"],
                                      min_local_correspondences=o["min_local"], max_global_correspondences=o["max_global"],
                                      num_refinement_steps=o["steps"])
        src, tgt, scores, T = lgr(t(sc["src_knn_points"]), t(sc["tgt_knn_points"]), torch.from_numpy(sc["src_masks"]),
                                  torch.from_numpy(sc["tgt_masks"]), t(sc["score_mat"]), t(sc["global_scores"]))
        out = dict(src_corr=src, tgt_corr=tgt, corr_scores=scores, transform=T)
        out["procrustes"] = vops.weighted_procrustes(src, tgt, scores)
        out["procrustes_unweighted"] = vops.weighted_procrustes(src, tgt)
        out["sc"] = vops.spatial_consistency(src, tgt, R.SIGMA)
        half = max(src.shape[0] // 2, 1)
        out["cross_sc"] = vops.cross_spatial_consistency(src[:half], tgt[:half], src, tgt, R.SIGMA)
        out["sc_counts"] = out["sc"].sum(dim=1)
        out["scf_topk"] = SpatialConsistencyFiltering(min(R.SCF_K, src.shape[0]), R.SIGMA)(src, tgt)
        out["eig"] = vops.leading_eigenvector(out["sc"], method="power", num_iterations=R.EIG_ITERS)
        torch.set_default_dtype(torch.float32)
        return {k: v.detach().numpy().astype(np.int64 if v.dtype == torch.int64 else np.float64) for k, v in out.items()}

    store = {"provenance": np.array(PROVENANCE)}
    for n, spec in enumerate(R.SCENES + [R.E2E]):
        sc, m, seed = R.find_scene(spec, 1000 * (n + 1))
        name = spec[0]
        r32, r64 = run(sc, torch.float32), run(sc, torch.float64)
        print("%-16s seed %5d  n_corr %3d  n_verify %3d  " % (name, seed, m["n_corr"], m["n_verify"]) +
              "  ".join("%s %.3g" % (k, m[k]) for k in R.MARGIN_KEYS) + "  eig %d%s" % (m["eig_iterations"], "" if m["eig_stopped"] else " (ran out)"))
        for k in ("src_knn_points", "tgt_knn_points", "src_masks", "tgt_masks", "score_mat", "global_scores", "R", "t"):
            store["%s/in_%s" % (name, k)] = sc[k]
        store[name + "/seed"] = np.int64(seed)
        store[name + "/screens"] = np.array([float(m[k]) for k in R.MARGIN_KEYS])
        store[name + "/eig_iterations"] = np.int64(m["eig_iterations"])
        for k, v in r64.items():
            if k in ("sc", "cross_sc") and m["n_verify"] > R.DENSE_MAX:     # the dense matrices of the large scene stay out of the file
                continue
            store["%s/%s" % (name, k)] = v
            if v.dtype == np.float64:
                assert r32[k].shape == v.shape, (name, k)
                store["%s/dev_%s" % (name, k)] = np.float64(np.abs(r32[k] - v).max() if v.size else 0.0)
            else:
                assert np.array_equal(r32[k], v), (name, k)
        rot, trn = R.pose_errors(r64["transform"], sc["R"], sc["t"])
        store[name + "/pose_error"] = np.array([rot, trn])
    np.savez_compressed(OUT, **store)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main(sys.argv[1])
