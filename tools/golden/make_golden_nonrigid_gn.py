"""Mint the fixture of the Gauss-Newton non-rigid ICP by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_nonrigid_gn.py REFERENCE_ROOT     # the directory holding Diff-Reg-2d3d/; writes tests/golden/nonrigid_gn.npz and nonrigid_gn_A.npz

The reference's own non_rigid_icp_gauss_newton (vision3d/layers/nonrigid_icp.py:18-154) is loaded by file path (vision3d/layers/__init__.py pulls
in far more than it needs) and run on every scene and form of tests/nonrigid_gn_ref, once in float32 and once in float64 (torch's default
dtype switched, since the reference creates its state with torch.eye / zeros).  Only reference OUTPUTS are stored, next to the inputs.

The stubs are those of make_golden_nonrigid.py: MagicMock for ipdb, vision3d.ext, pykeops, ...; torch.Tensor.cuda patched to the identity; the
graph's kNN replaced by a float64 brute-force kNN, with the same screen on every scene (sorted node distances up to rank K + 1 differ by more
than 1e-5 relative).  The graph is built ONCE per scene, by the reference's build_euclidean_deformation_graph in float64, and rounded to
float32: those float32 arrays are the inputs of both runs and of the device, so all three read the same numbers.

torch.linalg.solve is wrapped during the call so that A, b and x of the first iterations are recorded; the transforms are recorded after 1, 2
and 5 iterations.  A goes to a file of its own (tests/golden/nonrigid_gn_A.npz): a committed file stays below 1 MiB, so A is kept in full for
scenes with 6 M <= 70 and as its packed lower triangle for the scenes and forms tests/nonrigid_gn_ref.A_PACKED lists -- narrower than every
scene with 6 M <= 300.  The float32 run's deviation is kept per tensor as its largest absolute value, which is all the bar reads.  For the
scenes of nonrigid_gn_ref.WARP the reference's apply_deformation warps the whole cloud with the transforms after 5 iterations, in both precisions.  A scene
whose float32 transforms deviate from the float64 ones by more than 1e-4 at any recorded iteration count is rejected.
"""
import importlib.util
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)


def main(ref_root):
    import torch
    for m in ("vision3d.ext", "ipdb", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops"):
        sys.modules[m] = MagicMock()
    torch.Tensor.cuda = lambda self, *a, **k: self
    base = os.path.join(ref_root, "Diff-Reg-2d3d")
    sys.path.insert(0, base)
    import vision3d.ops  # noqa: F401
    dg = sys.modules["vision3d.ops.deformation_graph"]
    ed = sys.modules["vision3d.ops.embedded_deformation"]
    spec = importlib.util.spec_from_file_location("ref_nonrigid_icp", os.path.join(base, "vision3d", "layers", "nonrigid_icp.py"))
    gn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gn)
    from tests import nonrigid_gn_ref as G
    from tests import nonrigid_ref as R

    def knn64(q_points, s_points, k, return_distance=False, **kw):
        q, s = q_points.double(), s_points.double()
        d = (q[:, None, :] - s[None]).pow(2).sum(-1).sqrt()
        k = min(k, s.shape[0])
        idx = torch.argsort(d, dim=1, stable=True)[:, :k]
        dist = torch.gather(d, 1, idx).to(q_points.dtype)
        return (dist, idx) if return_distance else idx
    dg.knn = knn64

    solves = []
    real_solve = torch.linalg.solve

    def solve(a, b):
        x = real_solve(a, b)
        solves.append((a.clone(), b.clone(), x.clone()))
        return x

    def inputs(name):
        torch.set_default_dtype(torch.float64)
        sc = G.make_scene(name)
        t = lambda a: torch.from_numpy(np.asarray(a)).double()
        ai, aw, edges, ew = dg.build_euclidean_deformation_graph(t(sc["cloud"]), t(sc["nodes"]), sc["K"], sc["coverage"])
        torch.set_default_dtype(torch.float32)
        corr = sc["corr"]
        c_ai = ai.numpy()[corr]
        if name == "e":
            c_ai = R.holes(c_ai)
        return sc, dict(nodes=sc["nodes"], src=sc["cloud"][corr], tgt=sc["tgt"], ai=c_ai.astype(np.int64), aw=aw.numpy()[corr].astype(np.float32),
                        edges=edges.numpy().astype(np.int64), ew=ew.numpy().astype(np.float32), cw=G.corr_weights(corr.shape[0]),
                        cloud=sc["cloud"], all_ai=ai.numpy().astype(np.int64), all_aw=aw.numpy().astype(np.float32))

    def run(inp, form, dtype, warp=False):
        torch.set_default_dtype(dtype)
        kw = G.form_args(inp, form)
        t = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(dtype)
        args = (t(inp["nodes"]), t(inp["src"]), t(inp["tgt"]), torch.from_numpy(inp["ai"]), t(inp["aw"]), torch.from_numpy(inp["edges"]))
        out = {}
        for n in G.ITERS:
            del solves[:]
            torch.linalg.solve = solve
            try:
                T = gn.non_rigid_icp_gauss_newton(*args, corr_weights=t(kw["corr_weights"]), edge_weights=t(kw["edge_weights"]),
                                                  corr_lambda=kw["corr_lambda"], arap_lambda=kw["arap_lambda"], lm_lambda=kw["lm_lambda"],
                                                  num_iterations=n)
            finally:
                torch.linalg.solve = real_solve
            assert len(solves) == n
            out["T%d" % n] = T[:, :3, :]
            if n == G.ITERS[-1] and warp:
                out["warp%d" % n] = ed.apply_deformation(t(inp["cloud"]), args[0], T, torch.from_numpy(inp["all_ai"]), t(inp["all_aw"]))
            if n == G.ITERS[-1]:
                for it in range(G.RECORD):
                    out["A%d" % it], out["b%d" % it], out["x%d" % it] = solves[it]
        torch.set_default_dtype(torch.float32)
        return {k: v.detach().double().numpy() for k, v in out.items()}

    res, res_A = {}, {}
    for name in G.SCENES:
        sc, inp = inputs(name)
        gap = R.screen(sc["cloud"], sc["nodes"], sc["K"])
        assert gap > 1e-5, "scene %s: sorted node distances within %.2e relative" % (name, gap)
        M = inp["nodes"].shape[0]
        for k, v in inp.items():
            res["%s_in_%s" % (name, k)] = v.astype(np.int32) if v.dtype == np.int64 else v
        worst = 0.0
        for form in G.FORMS:
            warp = name in G.WARP and form == "fn"
            r64, r32 = run(inp, form, torch.float64, warp), run(inp, form, torch.float32, warp)
            for k, v in r64.items():
                dst = res
                if k[0] == "A":
                    dst = res_A
                    if not G.has_A(name, form, M):
                        continue
                    if 6 * M > G.A_FULL:
                        v, r32[k] = G.tril_pack(v), G.tril_pack(r32[k])
                key = "%s_%s_%s" % (name, form, k)
                dst[key] = v
                dst[key + "_dev32"] = np.array([np.abs(r32[k] - v).max() if v.size else 0.0], np.float32)
                if k[0] == "T" and v.size:
                    worst = max(worst, float(np.abs(r32[k] - v).max()))
            r0 = float(np.abs(r64["b0"]).max())
        assert worst <= 1e-4, "scene %s rejected: float32 transforms deviate from float64 by %.2e" % (name, worst)
        print("scene %s: M %d (6 M = %d), N %d, K %d, E %d; relative distance gap %.2e; float32 transforms within %.2e of float64; |b| %.3e"
              % (name, M, 6 * M, inp["src"].shape[0], sc["K"], inp["edges"].shape[0], gap, worst, r0))
    res["provenance"] = np.array("vision3d/layers/nonrigid_icp.py non_rigid_icp_gauss_newton run on the CPU in float32 and float64 on float32 "
                                 "inputs; the graph from the reference's builder in float64 under a float64 brute-force kNN (pykeops absent)")
    for f, d in zip(G.FILES, (res, res_A)):
        out = os.path.join(GOLDEN, f)
        np.savez_compressed(out, **d)
        assert os.path.getsize(out) <= 1 << 20, "%s is %d bytes: above 1 MiB" % (f, os.path.getsize(out))
        print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1])
