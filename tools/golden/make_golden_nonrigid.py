"""Mint the fixture of the non-rigid ICP path by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_nonrigid.py REFERENCE_ROOT     # the directory holding Diff-Reg-2d3d/; writes tests/golden/nonrigid.npz

The reference's own build_euclidean_deformation_graph (vision3d/ops/deformation_graph.py:26-103), apply_deformation
(vision3d/ops/embedded_deformation.py:31-66) and non_rigid_icp_adam with its cost functions (vision3d/ops/nonrigid_icp_adam.py:9-131) are imported
from where they lie and run on the scenes "a" .. "e" of tests/nonrigid_ref.make_scene, once in float32 and once in float64 (torch's default dtype
switched, since the reference creates its parameters with torch.eye / zeros_like).  Only reference OUTPUTS are stored, next to the inputs.

Imports need the stubs the other mint tools use (MagicMock for open3d, pykeops, vision3d.ext, ...).  torch.Tensor.cuda is patched to the identity in
this process: the reference calls .cuda() at deformation_graph.py:80-81 and nonrigid_icp_adam.py:102-103.  ONE MORE SHIM, unavoidable without pykeops:
vision3d.ops.deformation_graph.knn is replaced by a FLOAT64 brute-force kNN (ascending by distance, by index on ties), whatever the precision of the
run -- anchor parity with KeOps itself is NOT claimed.  Every scene is screened: in float64 the sorted node distances of every point up to rank
K + 1 differ by more than 1e-5 relative (asserted on every scene, no point skipped).

The Adam state is read from the reference's own optimizer (torch.optim.Adam is wrapped in the reference module's namespace so that the instance can
be found afterwards; nothing it computes changes), the cost trace from a wrapper around compute_cost_function that calls the reference's three cost
functions once more without gradient.  A scene whose float32 transforms deviate from the float64 ones by more than 1e-4 at any recorded iteration
count is rejected.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "nonrigid.npz")
sys.path.insert(0, ROOT)


def main(ref_root):
    import torch
    for m in ("vision3d.ext", "ipdb", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops"):
        sys.modules[m] = MagicMock()
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, os.path.join(ref_root, "Diff-Reg-2d3d"))
    import vision3d.ops  # noqa: F401
    import vision3d.ops.nonrigid_icp_adam  # noqa: F401  (the package's __init__ does not import it)
    dg = sys.modules["vision3d.ops.deformation_graph"]
    ed = sys.modules["vision3d.ops.embedded_deformation"]
    nr = sys.modules["vision3d.ops.nonrigid_icp_adam"]
    from tests import nonrigid_ref as R

    def knn64(q_points, s_points, k, return_distance=False, **kw):
        q, s = q_points.double(), s_points.double()
        d = (q[:, None, :] - s[None]).pow(2).sum(-1).sqrt()
        k = min(k, s.shape[0])
        idx = torch.argsort(d, dim=1, stable=True)[:, :k]
        dist = torch.gather(d, 1, idx).to(q_points.dtype)
        return (dist, idx) if return_distance else idx
    dg.knn = knn64

    made = []

    class Adam(torch.optim.Adam):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)
    trace = []
    orig_cost = nr.compute_cost_function

    def cost_wrapper(rot, trn, nodes, src, tgt, ai, aw, edges, ew):
        with torch.no_grad():
            T = nr.get_transform_from_rotation_translation(rot, trn)
            trace.append([float(nr.compute_landmark_cost(nodes, src, tgt, ai, aw, T)), float(nr.compute_arap_cost(nodes, edges, ew, rot, trn)),
                          float(nr.compute_orthogonal_cost(rot))])
        return orig_cost(rot, trn, nodes, src, tgt, ai, aw, edges, ew)
    nr.optim.Adam = Adam
    nr.compute_cost_function = cost_wrapper

    def run(name, dtype):
        """every recorded tensor of scene `name` in `dtype`, as float64 / int64 numpy"""
        torch.set_default_dtype(dtype)
        sc = R.make_scene(name)
        t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
        cloud, nodes, tgt = t(sc["cloud"]), t(sc["nodes"]), t(sc["tgt"])
        corr = torch.from_numpy(sc["corr"])
        out = {}
        g = dg.build_euclidean_deformation_graph(cloud, nodes, sc["K"], sc["coverage"], return_distance=True)
        names = ("anchor_indices", "anchor_weights", "anchor_distances", "edge_indices", "edge_weights", "edge_distances")
        for k, v in zip(names, g):
            out["graph_" + k] = v
        ai, aw, _, edges, ew, _ = g
        src, c_ai, c_aw = cloud[corr], ai[corr], aw[corr]
        if name == "e":
            c_ai = torch.from_numpy(R.holes(c_ai.numpy()))
        out["corr_anchor_indices"] = c_ai
        args = (nodes, src, tgt, c_ai, c_aw, edges, ew)
        for n in R.STEPS:
            del made[:], trace[:]
            T = nr.non_rigid_icp_adam(*args, num_iterations=n)
            opt = made[-1]
            rot, trn = opt.param_groups[0]["params"]
            assert torch.equal(T[:, :3, :3], rot.detach()) and torch.equal(T[:, :3, 3], trn.detach())
            out["adam%d_rot" % n], out["adam%d_trn" % n] = rot.detach().clone(), trn.detach().clone()
            for tag, p in (("rot", rot), ("trn", trn)):
                out["adam%d_m_%s" % (n, tag)] = opt.state[p]["exp_avg"].clone()
                out["adam%d_v_%s" % (n, tag)] = opt.state[p]["exp_avg_sq"].clone()
            if n == R.STEPS[-1]:
                out["trace"] = torch.tensor(trace, dtype=torch.float64)
        for n in R.STATES:
            if n == 0:
                rot, trn = torch.eye(3).repeat(nodes.shape[0], 1, 1), torch.zeros_like(nodes)
            else:
                rot, trn = out["adam%d_rot" % n].clone(), out["adam%d_trn" % n].clone()
            rot.requires_grad_(True); trn.requires_grad_(True)
            T = nr.get_transform_from_rotation_translation(rot, trn)
            terms = [nr.compute_landmark_cost(nodes, src, tgt, c_ai, c_aw, T), nr.compute_arap_cost(nodes, edges, ew, rot, trn),
                     nr.compute_orthogonal_cost(rot)]
            orig_cost(rot, trn, *args).backward()
            out["state%d_cost" % n] = torch.stack(terms).detach()
            out["state%d_grad_rot" % n], out["state%d_grad_trn" % n] = rot.grad.clone(), trn.grad.clone()
            out["state%d_warp" % n] = ed.apply_deformation(cloud, nodes, T.detach(), ai, aw)
            out["state%d_warp_corr" % n] = ed.apply_deformation(src, nodes, T.detach(), c_ai, c_aw)
        torch.set_default_dtype(torch.float32)
        return sc, {k: v.detach().numpy().astype(np.int64 if v.dtype == torch.int64 else np.float64) for k, v in out.items()}

    res = {}
    for name in R.SCENES:
        sc, r64 = run(name, torch.float64)
        _, r32 = run(name, torch.float32)
        gap = R.screen(sc["cloud"], sc["nodes"], sc["K"])
        assert gap > 1e-5, "scene %s: sorted node distances within %.2e relative" % (name, gap)
        worst = 0.0
        for k, v in r64.items():
            if v.dtype == np.int64:
                assert np.array_equal(v, r32[k]), "scene %s: %s differs between float32 and float64" % (name, k)
                res["%s_%s" % (name, k)] = v.astype(np.int32)
                continue
            res["%s_%s" % (name, k)] = v
            with np.errstate(invalid="ignore"):
                res["%s_%s_dev32" % (name, k)] = (r32[k] - v).astype(np.float32)
            if k.startswith("adam") and (k.endswith("_rot") or k.endswith("_trn")) and "_m_" not in k and "_v_" not in k:
                worst = max(worst, float(np.abs(r32[k] - v).max()))
        assert worst <= 1e-4, "scene %s rejected: float32 transforms deviate from float64 by %.2e" % (name, worst)
        tr = r64["trace"]
        print("scene %s: M %d, N %d, K %d, E %d; relative distance gap %.2e; float32 transforms within %.2e of float64; cost %.3e -> %.3e"
              % (name, sc["nodes"].shape[0], sc["tgt"].shape[0], sc["K"], r64["graph_edge_indices"].shape[0], gap, worst, tr[0].sum(), tr[-1].sum()))
        for k in ("cloud", "nodes", "corr", "tgt"):
            res["%s_in_%s" % (name, k)] = sc[k]
    res["provenance"] = np.array("reference functions run on the CPU in float32 and float64; vision3d.ops.deformation_graph.knn replaced by a float64 "
                                 "brute-force kNN (pykeops absent): anchor parity with KeOps is not claimed")
    np.savez_compressed(OUT, **res)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main(sys.argv[1])
