"""The 2D-3D item's numpy statement (tests/item2d3d_ref.py) against the fixture minted from the reference's own functions
(tests/golden/item2d3d.npz, tools/golden/make_golden_item2d3d.py), the fixture's size and screening, and the public signatures.  CPU only."""
import inspect
import os

import numpy as np
import pytest

from tests import item2d3d_ref as R

CASE_IDS = range(len(R.CASES))


def fixture_case(g, k):
    r2d, r3d, limit = g["c%d_radii" % k].tolist()
    return dict(depth=g["c%d_depth" % k], points=g["c%d_points" % k], K=g["c%d_K" % k], T=g["c%d_T" % k], r2d=r2d, r3d=r3d, limit=limit)


@pytest.mark.parametrize("k", CASE_IDS)
def test_statement_equals_the_reference(golden, k):
    g = golden("item2d3d")
    c = fixture_case(g, k)
    mp, mi = R.corr_mutual(c)
    assert mp.dtype == np.int64 and np.array_equal(mp, g["c%d_mutual_pixels" % k]) and np.array_equal(mi, g["c%d_mutual_indices" % k])
    rp, ri = R.corr_radius(c)
    assert np.array_equal(rp, g["c%d_radius_pixels" % k]) and np.array_equal(ri, g["c%d_radius_indices" % k])
    flat = rp[:, 0] * c["depth"].shape[1] + rp[:, 1]
    assert np.all((np.diff(flat) > 0) | ((np.diff(flat) == 0) & (np.diff(ri) > 0)))          # stored in ascending (pixel, point)
    kind = R.CASES[k][4]
    if kind in ("far", "blank"):
        assert len(mi) == 0 and len(ri) == 0
    else:
        assert len(mi) > 0 and len(ri) >= len(mi)


@pytest.mark.parametrize("k", CASE_IDS)
def test_cases_pass_the_screening_and_are_reproducible(golden, k):
    g = golden("item2d3d")
    c = fixture_case(g, k)
    assert R.screen(c) is None
    H, W, N, dt, kind, r2d, r3d = R.CASES[k]
    assert c["depth"].shape == (H, W) and c["depth"].dtype == np.float32 and c["points"].shape == (N, 3)
    assert c["points"].dtype == (np.float32 if dt == "f4" else np.float64) and (c["r2d"], c["r3d"]) == (r2d, r3d)
    again = R.make_case(k, int(g["c%d_seed" % k][0]))
    for name in ("depth", "points", "K", "T"):
        assert np.array_equal(again[name], c[name])
    if kind == "blank":
        assert not c["depth"].any()
    elif H * W >= 900:                                                                       # 35 or 67 pixels need not hold every kind
        d = c["depth"]
        assert 0.05 < (d == 0).mean() < 0.15 and (d > 6000).any() and ((d > 0) & (d < 200)).any()   # holes, beyond the limit, near the camera


def test_screening_sees_what_it_is_for():
    c = R.make_case(5, 1)
    ip, _ = R.image_points(c["depth"], c["K"])
    q = ip[:1] + np.array([[0.0, 0.0, c["r3d"]]])                                           # a point exactly radius_3d from a pixel
    c["points"] = ((q - c["T"][:3, 3]) @ c["T"][:3, :3])
    assert R.screen(c) is not None


@pytest.mark.parametrize("k", range(len(R.ITEMS)))
def test_item_statement_equals_the_reference(golden, k):
    g = golden("item2d3d")
    raw, opt, draws = R.make_item(k, int(g["i%d_seed" % k][0]))
    st = R.item_statement(raw, opt, draws)
    assert R.screen(st["_case"]) is None
    for name in R.INT_KEYS:
        assert (name in st) == ("i%d_%s" % (k, name) in g.files)
        if name in st:
            assert np.array_equal(st[name], g["i%d_%s" % (k, name)]), name
    for name in ("points", "transform", "image", "intrinsics"):
        want = g["i%d_%s" % (k, name)]
        assert want.dtype == np.float32 and np.all(np.abs(st[name].astype(np.float64) - want) <= np.spacing(np.abs(want))), name


def test_fixture_holds_data_only_and_stays_small(golden):
    from tests.conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "item2d3d.npz")) < 1 << 20
    g = golden("item2d3d")
    assert all(g[k].dtype.kind in "fiu" for k in g.files)


def test_public_signatures_are_the_references():
    from diffreg_hip import item2d3d as it
    want = ["depth_img", "pcd_points", "intrinsic", "transform", "matching_radius_2d", "matching_radius_3d", "depth_limit"]   # registration_utils.py:30-38
    for fn in (it.get_2d3d_correspondences_mutual, it.get_2d3d_correspondences_radius):
        s = inspect.signature(fn)
        assert list(s.parameters) == want and s.parameters["depth_limit"].default == 6.0
        assert all(p.default is inspect.Parameter.empty for n, p in s.parameters.items() if n != "depth_limit")
    s = inspect.signature(it.prepare_item)
    assert list(s.parameters)[0] == "raw" and all(p.kind is inspect.Parameter.KEYWORD_ONLY for n, p in s.parameters.items() if n != "raw")
    for name in ("max_points", "use_augmentation", "augmentation_noise", "return_corr_indices", "matching_method", "matching_radius_2d",
                 "matching_radius_3d", "return_overlap_indices", "crop", "generator", "aug_transform", "noise", "sel_indices"):
        assert name in s.parameters, name
    with pytest.raises(NotImplementedError):
        it.prepare_item({}, max_points=None, use_augmentation=False, augmentation_noise=0.005, return_corr_indices=False,
                        matching_method="mutual_nearest", matching_radius_2d=8.0, matching_radius_3d=0.0375, return_overlap_indices=False,
                        scale_augmentation=True)


def test_library_exports_the_thirteenth_set():
    from diffreg_hip import lib
    raw = lib.raw()
    names = ("dr_corr_2d3d_mutual_f64", "dr_corr_2d3d_mutual_workspace_bytes", "dr_corr_2d3d_radius_f64", "dr_corr_2d3d_radius_workspace_bytes",
             "dr_overlap_2d3d_f64", "dr_overlap_2d3d_workspace_bytes", "dr_column_mean_seq_f32")
    for name in names:
        assert name in lib.SIGNATURES and hasattr(raw, name)
    assert raw.dr_corr_2d3d_mutual_workspace_bytes(0, 0, 0) == 0
    # N = 64: 2048 + 1024 + 512 + 256; H W = 35: 256 pixel words; max = 64 offsets: 512; one chunk sum: 256
    assert raw.dr_corr_2d3d_mutual_workspace_bytes(7, 5, 64) == 2048 + 1024 + 512 + 256 + 256 + 512 + 256
    assert raw.dr_corr_2d3d_radius_workspace_bytes(7, 5, 64) == raw.dr_overlap_2d3d_workspace_bytes(7, 5, 64) == raw.dr_corr_2d3d_mutual_workspace_bytes(7, 5, 64)
    # argument checks come before any launch: they answer without a device
    none12 = (None, 1000.0, 6.0, None, None, 0, None, 8.0, 0.1)
    assert raw.dr_corr_2d3d_mutual_f64(-1, 1, 1, *none12, 0, None, None, None, None, 0, None) == -1
    assert raw.dr_corr_2d3d_radius_f64(4, 4, 4, *none12, 0, None, None, None, None, 0, None) == -1
    assert raw.dr_overlap_2d3d_f64(1 << 16, 1 << 16, 1, *none12, 0, 0, None, None, None, None, 0, None) != 0
    assert raw.dr_column_mean_seq_f32(0, None, None, None) == -1
