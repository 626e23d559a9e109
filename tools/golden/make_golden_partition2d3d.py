"""Mint the fixture of the 2D-3D patch partition and ground-truth patch overlaps by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_partition2d3d.py REFERENCE_ROOT     # the directory holding Diff-Reg-2d3d/; writes tests/golden/partition2d3d.npz

The reference's own point_to_node_partition (vision3d/ops/point_cloud_partition.py:41-104), patchify, get_2d3d_node_correspondences and
multual_nn_correspondence (EXP/utils.py:28-56, 59-175, 234-252; EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1) are imported from
where they lie and chained as EXP/model.py:403-495 chains them (the glue of :412-416 -- node mask by pcd_min_node_size, padded gathers -- restated here),
on the scenes "a", "b", "c" of tests/partition2d3d_ref.make_scene.  Only reference OUTPUTS are stored, plus a checksum of the inputs.

Imports need the stubs of make_golden_train2d3d.py (MagicMock for open3d, pykeops, vision3d.ext, ...; a no-op Tensor.cuda).  ONE MORE SHIM, unavoidable
without pykeops: vision3d.ops.knn.keops_knn (the only KeOps call on this path, knn.py:10-27) is replaced by a dense
`(q[:, :, None] - s[:, None]).norm(dim=-1).topk(k, largest=False)` -- the same norm2 of differences that KeOps evaluates -- in chunks over the batch.
Everything else executed is the reference's code.  get_correspondences needs Open3D and is not minted: dr_radius_pairs_f32 is parity-unpinned against it.

The scenes are accepted only if the reference's outputs stay inside the caps of tests/partition2d3d_ref.py against the float64 restatement (the same
assertions tests/test_partition2d3d_oracle.py makes on the stored file).
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "partition2d3d.npz")
sys.path.insert(0, ROOT)


def dense_knn(q_points, s_points, k):
    import torch
    ds, ix = [], []
    for b0 in range(0, q_points.shape[0], 256):
        d = (q_points[b0:b0 + 256, :, None] - s_points[b0:b0 + 256, None]).norm(dim=-1).topk(k, dim=-1, largest=False)
        ds.append(d.values); ix.append(d.indices)
    return torch.cat(ds), torch.cat(ix)


def main(ref_root):
    import torch
    for m in ("vision3d.ext", "ipdb", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops"):
        sys.modules[m] = MagicMock()
    torch.Tensor.cuda = lambda self, *a, **k: self
    tree = os.path.join(ref_root, "Diff-Reg-2d3d")
    exp = os.path.join(tree, "experiments", "2d3dmatr.rgbdv2.stage4.level3.stage1")
    sys.path.insert(0, tree)
    sys.path.insert(0, exp)
    from vision3d.ops import point_to_node_partition
    sys.modules["vision3d.ops.knn"].keops_knn = dense_knn           # (vision3d.ops.knn as an attribute is the function; the module is in sys.modules)
    cwd = os.getcwd()
    os.chdir(exp)
    import utils as exp_utils
    os.chdir(cwd)
    from tests import partition2d3d_ref as R
    torch.set_num_threads(16)
    res = {}
    for name in ("a", "b", "c"):
        sc = R.make_scene(name)
        res[name + "_input_checksum"] = R.input_checksum(sc)
        p2n, sizes, masks, knn, kmask = point_to_node_partition(sc["pcd_points"], sc["nodes"], sc["limit"], gather_points=True, return_count=True)
        part = dict(point_to_node=p2n, node_sizes=sizes, node_masks=masks, node_knn_indices=knn, node_knn_masks=kmask)
        patches = exp_utils.patchify(sc["img_points"], sc["img_points_da"], sc["img_pixels"], sc["img_masks"], sc["img_masks_da"], sc["H"], sc["W"], sc["Hc"],
                                     sc["Wc"], stride=sc["stride"])
        # the reference's own partition and patches feed its overlap function, as in the model
        args = R.node_corr_inputs(sc, part, patches=patches)
        out = exp_utils.get_2d3d_node_correspondences(*R.reference_args(args))
        names = ("img_corr_indices", "pcd_corr_indices", "img_corr_overlaps", "pcd_corr_overlaps", "pcd_centers", "img_centers", "img_centers_da", "coarse_match_gt")
        got = dict(zip(names, out))
        # acceptance: the reference inside the caps against the float64 restatement
        ref_part = R.partition(sc["pcd_points"], sc["nodes"], sc["limit"], want_gaps=True)
        st_p = R.assert_partition_matches(part, ref_part, sc["pcd_points"].shape[0], sc["limit"], name)
        ref_oc = R.ref_node_corr(args, want_undecided=True)
        st_o = R.assert_overlaps_match(got, ref_oc, sc["nodes"].shape[0], name)
        st_m = R.assert_mutual_matches(got["coarse_match_gt"], got["pcd_centers"], got["img_centers"], R.R_MUTUAL, name)
        print("scene %s: largest node %d, width %d; undecided points %d (nodes touched %d, positions compared as sets %d); candidates %d, pairs %d "
              "(undecided %d); mutual pairs %d (undecided sources %d)" % (name, int(sizes.max()), knn.shape[1], st_p[0], st_p[1], st_p[2],
                                                                           ref_oc["cand_i"].shape[0], st_o[0], st_o[1], st_m[0], st_m[1]))
        for k, v in part.items():
            res["%s_%s" % (name, k)] = v.numpy().astype(np.int32) if v.dtype == torch.int64 else v.numpy()
        if name == "a":                                                 # "b" shares the image; "c" is small
            pn = ("knn_points", "knn_points_da", "knn_pixels", "knn_indices", "knn_masks", "knn_masks_da", "masks", "masks_da")
            for k, v in zip(pn, patches):
                if k in ("knn_indices", "knn_masks", "knn_masks_da", "masks", "masks_da"):
                    res["a_patch_" + k] = v.numpy().astype(np.int32) if v.dtype == torch.int64 else v.numpy()
                else:                                                   # gathered floats: the index pattern says it all; a checksum pins them
                    res["a_patch_" + k + "_sum"] = np.array([float(v.double().sum())])
        for k, v in got.items():
            v = torch.as_tensor(v)
            res["%s_%s" % (name, k)] = v.numpy().astype(np.int32) if v.dtype == torch.int64 else v.numpy()
    np.savez_compressed(OUT, **res)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(res), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
