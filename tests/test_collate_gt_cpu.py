"""The ground-truth collate's numpy statement (tests/collate_gt_ref.py) against the fixture minted from the reference's own functions
(tests/golden/collate_gt.npz, tools/golden/make_golden_collate_gt.py), the fixture's screening conditions, and the public signatures.  CPU only."""
import inspect

import numpy as np
import pytest

from tests import collate_gt_ref as cg

MATCH_IDS = range(len(cg.MATCH_SCENES))
BLEND_IDS = range(len(cg.BLEND_SCENES))


def flow_bar(g, k):
    """the bar of every flow comparison: max(1e-9, 4 x the reference's own float32 deviation from float64 on that scene)"""
    return max(1e-9, 4.0 * float(g["b%d_dev" % k][0]))


@pytest.mark.parametrize("k", MATCH_IDS)
def test_match_statement_equals_the_reference(golden, k):
    g = golden("collate_gt")
    flow = g["m%d_flow" % k] if "m%d_flow" % k in g else None
    got = cg.coarse_gt_matches(g["m%d_src" % k], g["m%d_tgt" % k], g["m%d_rot" % k], g["m%d_trn" % k], cg.RADIUS, flow)
    want = g["m%d_matches" % k]
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    ns, nt, kind = cg.MATCH_SCENES[k]
    assert g["m%d_src" % k].shape == (ns, 3) and g["m%d_tgt" % k].shape == (nt, 3)
    assert (kind == "flow") == (flow is not None)
    if kind == "none":
        assert want.shape[1] == 0
    if kind == "all":
        assert np.array_equal(want[0], np.arange(ns))


@pytest.mark.parametrize("k", MATCH_IDS)
def test_match_scenes_pass_the_screening_and_are_reproducible(golden, k):
    g = golden("collate_gt")
    flow = g["m%d_flow" % k] if "m%d_flow" % k in g else None
    assert cg.screen_matches(g["m%d_src" % k], g["m%d_tgt" % k], g["m%d_rot" % k], g["m%d_trn" % k], cg.RADIUS, flow)
    sc = cg.match_scene(k, int(g["m%d_seed" % k][0]))
    for name in ("src", "tgt", "rot", "trn"):
        assert np.array_equal(sc[name], g["m%d_%s" % (k, name)])


@pytest.mark.parametrize("k", BLEND_IDS)
def test_blend_statement_equals_the_reference(golden, k):
    g = golden("collate_gt")
    q, r, f, want = g["b%d_query" % k], g["b%d_ref" % k], g["b%d_ref_flow" % k], g["b%d_out" % k]
    assert want.dtype == np.float32 and want.shape == q.shape
    exact = cg.blend_flow_knn3(q, r, f, np.float64)
    dev = np.abs(want.astype(np.float64) - exact).max()
    assert dev <= float(g["b%d_dev" % k][0]) * (1 + 1e-12)                      # the recorded deviation is the reference's from THIS statement
    got = cg.blend_flow_knn3(q, r, f, np.float32)
    assert got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - want).max() <= flow_bar(g, k)
    assert cg.screen_blend(q, r)
    nq, nr, coincident = cg.BLEND_SCENES[k]
    assert q.shape == (nq, 3) and r.shape == (nr, 3)
    assert int((cg.d2_matrix(q, r).min(1) == 0).sum()) == coincident           # the queries that sit on a reference point (1e-10 clamp)


def test_too_few_points_have_no_result():
    p = np.zeros((1, 3), np.float32)
    q = np.ones((5, 3), np.float32)
    assert cg.coarse_gt_matches(p, q, np.eye(3), np.zeros(3), 1.0) is None and cg.coarse_gt_matches(q, p, np.eye(3), np.zeros(3), 1.0) is None
    assert cg.blend_flow_knn3(q, q[:3], q[:3]) is None


def test_tie_scene_follows_the_lowest_index_rule():
    t = cg.TIE_MATCH
    for dtype in (np.float64, np.float32):
        m = cg.coarse_gt_matches(t["src"], t["tgt"], t["rot"], t["trn"], t["radius"], dtype=dtype)
        assert np.array_equal(m, np.array([[0], [0]]))
    b = cg.TIE_BLEND
    idx, val = cg.nearest(cg.d2_matrix(b["query"], b["ref"], np.float64), 3)
    assert np.array_equal(idx, np.array([[0, 1, 2], [0, 2, 6]])) and np.all(val == 1.0)     # five (four) references at d^2 = 1: the lowest three
    out = cg.blend_flow_knn3(b["query"], b["ref"], b["ref_flow"], np.float64)
    assert np.allclose(out, np.array([[1, 2, 4], [65, 0, 4]]) / 3.0, rtol=1e-15)


@pytest.mark.parametrize("k", range(len(cg.CALIB_DATASETS)))
def test_calibration_statement_equals_the_reference(golden, k):
    g = golden("collate_gt")
    hist_n = cg.hist_bins(cg.CALIB_CFG["deform_radius"])
    data = cg.calib_dataset(k)
    hists, limits, used = cg.calibrate_from_counts((cg.calib_counts(s, t) for s, t in data), cg.CALIB_CFG["num_layers"], hist_n,
                                                   samples_threshold=cg.CALIB_DATASETS[k][3])
    w = g["c%d_hists" % k]
    assert used == int(g["c%d_used" % k][0])
    assert np.array_equal(hists[:, :w.shape[1]], w) and not hists[:, w.shape[1]:].any()
    assert np.array_equal(limits, g["c%d_limits" % k])
    if k == 0:
        assert used < len(data)                 # stops early
    if k == 1:
        assert used == len(data)                # runs to its end


def test_fixture_holds_data_only_and_stays_small(golden):
    import os
    from tests.conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "collate_gt.npz")) < 1 << 20
    g = golden("collate_gt")
    assert all(g[k].dtype.kind in "fiu" for k in g.files)


def test_public_signatures():
    from diffreg_hip import collate
    s = inspect.signature(collate.collate_fn_device)
    assert list(s.parameters) == ["pairs", "config", "neighborhood_limits", "coarse_level", "training"]
    assert s.parameters["coarse_level"].default == -2 and s.parameters["training"].default is True
    s = inspect.signature(collate.calibrate_neighbors_device)
    assert list(s.parameters)[:4] == ["samples", "config", "keep_ratio", "samples_threshold"]
    assert s.parameters["keep_ratio"].default == 0.8 and s.parameters["samples_threshold"].default == 2000
    assert list(inspect.signature(collate.collate_fn_device_4dmatch).parameters)[:3] == ["pairs", "config", "neighborhood_limits"]


def test_library_exports_the_eleventh_set():
    from diffreg_hip import lib
    for name in ("dr_blend_flow_knn3_f32", "dr_coarse_gt_matches_f32", "dr_coarse_gt_matches_workspace_bytes"):
        assert name in lib.SIGNATURES and hasattr(lib.raw(), name)
    raw = lib.raw()
    assert raw.dr_coarse_gt_matches_workspace_bytes(0, 0) == 0
    assert raw.dr_coarse_gt_matches_workspace_bytes(65, 63) == 3 * 512 - 256 and raw.dr_coarse_gt_matches_workspace_bytes(64, 64) == 768
    # argument checks come before any launch: they answer without a device
    assert raw.dr_blend_flow_knn3_f32(-1, 0, 0, None, None, None, None, None, None, None, None) == -1
    assert raw.dr_blend_flow_knn3_f32(1, 4, 4, None, None, None, None, None, None, None, None) == -1
    assert raw.dr_coarse_gt_matches_f32(1, -2, 0, None, None, None, None, None, None, None, 0.1, None, None, None, None, None, 0, None) == -1
    assert raw.dr_coarse_gt_matches_f32(0, 0, 0, None, None, None, None, None, None, None, 0.1, None, None, None, None, None, 0, None) == 0


def test_pair_convention_is_positional_up_to_trn_and_a_dict_beyond():
    from diffreg_hip.collate import _pair_fields
    f = _pair_fields(("s", "t", "R", "T"))
    assert f["src_pcd"] == "s" and f["trn"] == "T" and f["gt_cov"] is None and f["s2t_flow"] is None
    assert _pair_fields(("s", "t"))["rot"] is None
    assert _pair_fields(dict(src_pcd="s", tgt_pcd="t", gt_cov=1))["gt_cov"] == 1
    with pytest.raises(ValueError):
        _pair_fields(("s", "t", "R", "T", "corr"))
    with pytest.raises(ValueError):
        _pair_fields(dict(src_pcd="s", tgt_pcd="t", flow=0))


def test_calibration_refuses_more_bins_than_the_count_kernel_keeps():
    from diffreg_hip.collate import calibrate_neighbors_device
    cfg = dict(cg.CALIB_CFG, architecture=list(cg._hash().KPFCN_ARCH), deform_radius=9.0)       # ceil(4/3 pi 10^3) = 4189 bins
    with pytest.raises(ValueError, match="4096"):
        calibrate_neighbors_device([], cfg)
