"""CPU: the float64 restatement of the 2D-3D patch partition / ground-truth overlaps (tests/partition2d3d_ref.py) against the fixture minted by running
the reference (tests/golden/partition2d3d.npz, tools/golden/make_golden_partition2d3d.py), under the decided / undecided rules stated there.  The caps are
conditions on the scenes: the reference's own float32 outputs must stay inside them, or the scene is no fixture."""
import os

import numpy as np
import pytest
import torch

from tests import partition2d3d_ref as R
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "partition2d3d.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _part(g, name):
    return {k: g["%s_%s" % (name, k)] for k in ("point_to_node", "node_sizes", "node_masks", "node_knn_indices", "node_knn_masks")}


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_inputs_are_the_minted_ones(golden, name):
    assert np.array_equal(R.input_checksum(R.make_scene(name)), golden[name + "_input_checksum"])


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_partition_restatement_vs_reference(golden, name):
    sc = R.make_scene(name)
    ref = R.partition(sc["pcd_points"], sc["nodes"], sc["limit"], want_gaps=True)
    und, touched, n_set = R.assert_partition_matches(_part(golden, name), ref, sc["pcd_points"].shape[0], sc["limit"], name)
    print("scene %s: undecided points %d, nodes they touch %d, positions compared as sets %d" % (name, und, touched, n_set))
    g = _part(golden, name)
    assert g["node_knn_indices"].shape[1] == min(int(g["node_sizes"].max()), sc["limit"])
    if name == "b":
        assert (g["node_sizes"] > sc["limit"]).any(), "scene b must exercise the cut at point_limit"
    if name == "c":
        assert (g["node_sizes"] == 0).any() and ((g["node_sizes"] > 0) & (g["node_sizes"] <= 5)).any(), "scene c must hold empty and tiny nodes"


def test_patchify_restatement_vs_reference(golden):
    sc = R.make_scene("a")
    p = R.patchify(sc["img_points"], sc["img_points_da"], sc["img_pixels"], sc["img_masks"], sc["img_masks_da"], sc["H"], sc["W"], sc["Hc"], sc["Wc"], sc["stride"])
    assert np.array_equal(p[3].numpy(), golden["a_patch_knn_indices"])
    assert np.array_equal(p[4].numpy(), golden["a_patch_knn_masks"]) and np.array_equal(p[5].numpy(), golden["a_patch_knn_masks_da"])
    assert np.array_equal(p[6].numpy(), golden["a_patch_masks"]) and np.array_equal(p[7].numpy(), golden["a_patch_masks_da"])
    for t, k in zip(p[:3], ("knn_points", "knn_points_da", "knn_pixels")):
        assert float(t.double().sum()) == float(golden["a_patch_%s_sum" % k][0])
    assert not golden["a_patch_masks"].all() and golden["a_patch_masks"].any(), "the zero-depth box must empty some image patches"


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_overlaps_restatement_vs_reference(golden, name):
    sc = R.make_scene(name)
    part = {k: torch.from_numpy(v.astype(np.int64) if v.dtype == np.int32 else v) for k, v in _part(golden, name).items()}
    args = R.node_corr_inputs(sc, part)                     # the reference's own partition feeds its overlaps, as at minting
    ref = R.ref_node_corr(args, want_undecided=True)
    got = {k: golden["%s_%s" % (name, k)] for k in ("img_corr_indices", "pcd_corr_indices", "img_corr_overlaps", "pcd_corr_overlaps", "pcd_centers",
                                                    "img_centers", "img_centers_da")}
    n, und = R.assert_overlaps_match(got, ref, sc["nodes"].shape[0], name)
    print("scene %s: %d candidates, %d pairs, %d undecided" % (name, ref["cand_i"].shape[0], n, und))
    assert n > 0
    if name == "c":
        assert not args["img_masks"].all(), "scene c must hold an all-masked image patch"
    # the float32 ratios are integer quotients: wherever decided they equal the restatement's bit for bit (asserted above); the mutual-NN list too
    m, und_m = R.assert_mutual_matches(golden[name + "_coarse_match_gt"], torch.from_numpy(golden[name + "_pcd_centers"]),
                                       torch.from_numpy(golden[name + "_img_centers"]), R.R_MUTUAL, name)
    assert m > 0


def test_radius_pairs_definition_is_self_consistent():
    sc = R.make_scene("c")
    pairs, d = R.radius_pairs(sc["nodes"], sc["pcd_points"][:200], sc["transform"], 0.2)
    assert pairs.shape[1] == 2 and pairs.shape[0] == int((d < 0.2).sum())
    R.assert_radius_pairs_match(pairs, sc["nodes"], sc["pcd_points"][:200], sc["transform"], 0.2)
    with pytest.raises(AssertionError):
        R.assert_radius_pairs_match(pairs[1:], sc["nodes"], sc["pcd_points"][:200], sc["transform"], 0.2)
