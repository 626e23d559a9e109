"""Mint the fixture of the 2D-3D dataset item's ground truth by RUNNING THE REFERENCE's own functions (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_item2d3d.py REFERENCE_ROOT      # the directory holding Diff-Reg-2d3d/
    -> tests/golden/item2d3d.npz

vision3d.array_ops is imported as it lies, with vision3d.ext stubbed as the other minting tools do and np.long / np.float restored IN THIS PROCESS
ONLY (the reference's text predates their removal).  Its get_2d3d_correspondences_mutual and get_2d3d_correspondences_radius (two scipy cKDTrees
each) run on the cases of tests/item2d3d_ref.py; the radius pairs are stored sorted by (pixel, point), since their inner order is the KD-tree's.
The item cases run the arithmetic of SevenScenes2D3DHardPairDataset.__getitem__ (sevenscenes_hard.py:128-206) on in-memory arrays, statement by
statement with the reference's own apply_transform / compose_transforms / inverse_transform / get_transform_from_rotation_translation and its
two correspondence functions, with the draws of np.random fixed (tests/item2d3d_ref.make_item).

Screening, asserted here from float64 tables of the inputs alone (tests/item2d3d_ref.screen): every nearest / second-nearest gap, every
|d - radius_3d| and every distance of a render argument from an integer is at least 1e-9 relative, and no 2D squared distance equals
radius_2d^2.  A case that fails is drawn again with the next seed (the seed is recorded); none is skipped.  Under these conditions the result
depends neither on the rounding of the reference's BLAS nor on the order a KD-tree leaves equal distances in.
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "item2d3d.npz")

from tests import item2d3d_ref as R      # noqa: E402


def reference_ops(ref_root):
    np.long, np.float = np.int64, np.float64
    for m in ("vision3d.ext", "open3d", "cv2", "ipdb", "IPython"):
        sys.modules[m] = MagicMock()
    sys.path.insert(0, os.path.join(ref_root, "Diff-Reg-2d3d"))
    while True:
        try:
            import vision3d.array_ops as ops
            return ops
        except ModuleNotFoundError as e:
            sys.modules[e.name] = MagicMock()


def by_pixel_then_point(pix, idx, W):
    order = np.lexsort((idx, pix[:, 0] * W + pix[:, 1]))
    return pix[order].astype(np.int64).reshape(-1, 2), idx[order].astype(np.int64)


def reference_item(ops, raw, opt, draws):
    """sevenscenes_hard.py:128-206 on in-memory arrays"""
    d = {}
    depth, image = raw["depth"].copy(), raw["image"].copy()
    intrinsics, transform, points = raw["intrinsics"].copy(), raw["cloud_to_image"].copy(), raw["points"]
    if "sel_indices" in draws:
        points = points[draws["sel_indices"]]
    if opt["use_augmentation"]:
        aug_transform = draws["aug_transform"]
        center = points.mean(axis=0)
        subtract_center = ops.get_transform_from_rotation_translation(None, -center)
        add_center = ops.get_transform_from_rotation_translation(None, center)
        aug_transform = ops.compose_transforms(subtract_center, aug_transform, add_center)
        points = ops.apply_transform(points, aug_transform)
        inv_aug_transform = ops.inverse_transform(aug_transform)
        transform = ops.compose_transforms(inv_aug_transform, transform)
        points += (draws["noise"] - 0.5) * opt["augmentation_noise"]
    image -= image.mean()
    W = image.shape[1]
    r2, r3 = opt["matching_radius_2d"], opt["matching_radius_3d"]
    if opt["return_corr_indices"]:
        if opt["matching_method"] == "mutual_nearest":
            pix, idx = ops.get_2d3d_correspondences_mutual(depth, points, intrinsics, transform, r2, r3)
        else:
            pix, idx = by_pixel_then_point(*ops.get_2d3d_correspondences_radius(depth, points, intrinsics, transform, r2, r3), W)
        d["img_corr_pixels"], d["img_corr_indices"], d["pcd_corr_indices"] = pix, pix[:, 0] * W + pix[:, 1], idx
    if opt["return_overlap_indices"]:
        pix, idx = ops.get_2d3d_correspondences_radius(depth, points, intrinsics, transform, r2, r3)
        flat = pix[:, 0] * W + pix[:, 1]
        io, po = np.unique(flat), np.unique(idx)
        d["img_overlap_pixels"], d["img_overlap_indices"], d["pcd_overlap_indices"] = np.stack([io // W, io % W], axis=1), io, po
    d["intrinsics"] = intrinsics.astype(np.float32)
    d["transform"] = transform.astype(np.float32)
    d["image"] = image.astype(np.float32)
    d["points"] = points.astype(np.float32)
    return d


def main(ref_root):
    ops = reference_ops(ref_root)
    out = {}
    for k in range(len(R.CASES)):
        c, seed = R.draw_case(k)
        assert R.screen(c) is None
        H, W = c["depth"].shape
        depth = c["depth"].astype(np.float64)
        if c["points"].shape[0] and (R.image_points(c["depth"], c["K"])[0].shape[0]):
            mp, mi = ops.get_2d3d_correspondences_mutual(depth, c["points"], c["K"], c["T"], c["r2d"], c["r3d"])
            try:
                rp, ri = by_pixel_then_point(*ops.get_2d3d_correspondences_radius(depth, c["points"], c["K"], c["T"], c["r2d"], c["r3d"]), W)
            except IndexError:      # registration_utils.py:24-25 cannot slice an EMPTY list of pairs: the definition's answer is the empty list
                assert R.CASES[k][4] == "far" and len(R.corr_radius(c)[1]) == 0
                rp, ri = np.zeros((0, 2), np.int64), np.zeros((0,), np.int64)
        else:                       # no image point at all: cKDTree refuses an empty query set; the definition's answer is the empty list
            assert R.CASES[k][4] == "blank"
            mp, mi = np.zeros((0, 2), np.int64), np.zeros((0,), np.int64)
            rp, ri = mp, mi
        if R.CASES[k][4] == "far":
            assert len(mi) == 0 and len(ri) == 0
        for name in ("depth", "points", "K", "T"):
            out["c%d_%s" % (k, name)] = c[name]
        out["c%d_radii" % k] = np.array([c["r2d"], c["r3d"], c["limit"]])
        out["c%d_mutual_pixels" % k], out["c%d_mutual_indices" % k] = mp.astype(np.int64).reshape(-1, 2), mi.astype(np.int64)
        out["c%d_radius_pixels" % k], out["c%d_radius_indices" % k] = rp, ri
        out["c%d_seed" % k] = np.array([seed])
        print("case %2d %s seed %d: %d mutual pairs, %d radius pairs" % (k, R.CASES[k], seed, len(mi), len(ri)))
    for k in range(len(R.ITEMS)):
        raw, opt, draws, seed = R.draw_item(k)
        d = reference_item(ops, raw, opt, draws)
        for name, v in d.items():
            out["i%d_%s" % (k, name)] = v.astype(np.int64) if name in R.INT_KEYS else v
        out["i%d_seed" % k] = np.array([seed])
        print("item %d seed %d: %s" % (k, seed, {n: v.shape for n, v in d.items()}))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
