"""The 2D-3D dataset item on the device (diffreg_hip.item2d3d on csrc/item2d3d.hip) against the fixture minted from the reference's own functions
(tests/golden/item2d3d.npz, tools/golden/make_golden_item2d3d.py).  The pair lists are compared by exact equality: the fixture's screening
(tests/item2d3d_ref.screen) keeps every decision 1e-9 relative away from its threshold, far above float64 rounding.  Shapes: 24 x 40 (2 x 3 image
tiles), 7 x 5, 1 x 67; N = 1, 63, 64, 65, 300 and 513 (one LDS stage of the reverse check + 1); float32 and float64 clouds; points nearer than
radius_3d to the camera plane (the whole-image window), behind it, projecting outside the image, off every border and corner, pairs of points
that share a nearest pixel, an empty result, an image without a single point."""
import numpy as np
import pytest
import torch

from diffreg_hip import item2d3d as it          # without the feature every test of this file fails here
from diffreg_hip import lib
from tests import item2d3d_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = range(len(R.CASES))


def case_args(g, k):
    r2d, r3d, limit = g["c%d_radii" % k].tolist()
    t = lambda name: torch.from_numpy(g["c%d_%s" % (k, name)]).to(DEV)
    return (t("depth"), t("points"), t("K"), t("T"), r2d, r3d, limit)


@pytest.mark.parametrize("k", CASE_IDS)
def test_mutual_list_equals_the_reference(golden, k):
    g = golden("item2d3d")
    a = case_args(g, k)
    assert a[1].dtype == (torch.float32 if R.CASES[k][3] == "f4" else torch.float64)
    pix, idx = it.get_2d3d_correspondences_mutual(*a)
    assert pix.dtype == torch.int64 and idx.dtype == torch.int64 and pix.shape == (idx.shape[0], 2)
    assert np.array_equal(pix.cpu().numpy(), g["c%d_mutual_pixels" % k]) and np.array_equal(idx.cpu().numpy(), g["c%d_mutual_indices" % k])
    pix2, idx2 = it.get_2d3d_correspondences_mutual(*a)                     # two runs are bit-equal
    assert torch.equal(pix, pix2) and torch.equal(idx, idx2)


@pytest.mark.parametrize("k", CASE_IDS)
def test_radius_list_equals_the_reference(golden, k):
    g = golden("item2d3d")
    a = case_args(g, k)
    pix, idx = it.get_2d3d_correspondences_radius(*a)
    assert pix.dtype == torch.int64 and idx.dtype == torch.int64 and pix.shape == (idx.shape[0], 2)
    assert np.array_equal(pix.cpu().numpy(), g["c%d_radius_pixels" % k]) and np.array_equal(idx.cpu().numpy(), g["c%d_radius_indices" % k])
    pix2, idx2 = it.get_2d3d_correspondences_radius(*a)
    assert torch.equal(pix, pix2) and torch.equal(idx, idx2)


@pytest.mark.parametrize("k", CASE_IDS)
def test_overlap_lists_are_the_unique_of_the_reference_pairs(golden, k):
    g = golden("item2d3d")
    a = case_args(g, k)
    W = a[0].shape[1]
    io, po = it.get_2d3d_overlap_indices(*a)
    rp, ri = g["c%d_radius_pixels" % k], g["c%d_radius_indices" % k]
    assert np.array_equal(io.cpu().numpy(), np.unique(rp[:, 0] * W + rp[:, 1])) and np.array_equal(po.cpu().numpy(), np.unique(ri))


def test_the_edge_populations_are_in_the_fixture(golden):
    """the cases hold what their description promises (from the float64 statement): whole-image windows WITH partners, points behind the camera,
    projections outside the image, partners on all four borders and corners, and a pixel that is the nearest of two points"""
    g = golden("item2d3d")
    borders, shared, near_pairs, behind, outside = set(), 0, 0, 0, 0
    for k in CASE_IDS:
        c = dict(depth=g["c%d_depth" % k], points=g["c%d_points" % k], K=g["c%d_K" % k], T=g["c%d_T" % k])
        c["r2d"], c["r3d"], c["limit"] = g["c%d_radii" % k].tolist()
        H, W = c["depth"].shape
        q = R.transformed(c["points"], c["T"])
        behind += int((q[:, 2] <= -c["r3d"]).sum())
        rp, _ = R.render(q, c["K"])
        outside += int(((rp[:, 1] < 0) | (rp[:, 1] >= W)).sum())
        pix, idx = g["c%d_radius_pixels" % k], g["c%d_radius_indices" % k]
        near_pairs += int((q[idx, 2] <= c["r3d"]).sum())
        for h, w in g["c%d_mutual_pixels" % k]:
            borders |= {n for n, hit in (("top", h == 0), ("bottom", h == H - 1), ("left", w == 0), ("right", w == W - 1)) if hit}
            borders |= {"corner%d%d" % (h > 0, w > 0)} if (h in (0, H - 1) and w in (0, W - 1)) else set()
        px, d2, _, _ = R._tables(c)
        if d2.size:
            best = np.where(np.sqrt(d2.min(0)) < c["r3d"], d2.argmin(0), -1)
            best = best[best >= 0]
            shared += int(len(best) - len(np.unique(best)))
    assert behind > 0 and outside > 0 and near_pairs > 0 and shared > 0
    assert {"top", "bottom", "left", "right"} <= borders and len([b for b in borders if b.startswith("corner")]) >= 2, borders


def test_cap_below_the_number_found_raises_and_writes_nothing_behind_it(golden):
    g = golden("item2d3d")
    a = case_args(g, 0)
    for method, key in (("mutual_nearest", "mutual"), ("radius", "radius")):
        want_p, want_i = g["c0_%s_pixels" % key], g["c0_%s_indices" % key]
        cap = len(want_i) // 2
        # room for far more than cap behind the tensors handed in: the rows behind cap must keep their fill
        pix, idx, counts = lib.corr_2d3d(*a[:6], depth_limit=a[6], method=method, cap=cap)
        assert counts.tolist() == [cap, len(want_i)]
        assert np.array_equal(pix.cpu().numpy(), want_p[:cap]) and np.array_equal(idx.cpu().numpy(), want_i[:cap])
        with pytest.raises(RuntimeError, match="room for %d" % cap):
            it.correspondences(*a, method=method, cap=cap)
        # the raw entry with guarded buffers: rows behind cap stay untouched
        depth, pts, K, T = lib._item_inputs("test", a[0], a[1], a[2], a[3])
        pix = torch.full((len(want_i) + 8, 2), -7, dtype=torch.int64, device=DEV)
        idx = torch.full((len(want_i) + 8,), -7, dtype=torch.int64, device=DEV)
        counts = torch.zeros(2, dtype=torch.int32, device=DEV)
        fn, size_fn = ((lib.raw().dr_corr_2d3d_mutual_f64, lib.raw().dr_corr_2d3d_mutual_workspace_bytes) if key == "mutual" else
                       (lib.raw().dr_corr_2d3d_radius_f64, lib.raw().dr_corr_2d3d_radius_workspace_bytes))
        lib._item_call(fn, size_fn, depth, pts, K, T, 1000.0, a[6], a[4], a[5], [cap], [pix, idx], counts)
        assert counts.tolist() == [cap, len(want_i)]
        assert bool((pix[cap:] == -7).all()) and bool((idx[cap:] == -7).all()) and np.array_equal(idx[:cap].cpu().numpy(), want_i[:cap])


def test_empty_inputs(golden):
    g = golden("item2d3d")
    depth, pts, K, T, r2d, r3d, limit = case_args(g, 0)
    for d, p in ((depth, pts[:0]), (depth[:0], pts), (torch.zeros_like(depth), pts)):
        for fn in (it.get_2d3d_correspondences_mutual, it.get_2d3d_correspondences_radius):
            pix, idx = fn(d, p, K, T, r2d, r3d, limit)
            assert pix.shape == (0, 2) and idx.shape == (0,)
        io, po = it.get_2d3d_overlap_indices(d, p, K, T, r2d, r3d, limit)
        assert io.numel() == 0 and po.numel() == 0


def test_column_mean_is_numpys_row_after_row_sum():
    rng = np.random.RandomState(5)
    for n in (1, 2, 511, 512, 513, 3000):
        x = (rng.randn(n, 3) * 3 + np.array([1.5, -0.2, 4.0])).astype(np.float32)
        want = x.mean(axis=0)
        assert want.dtype == np.float32
        got = lib.column_mean_seq(torch.from_numpy(x).to(DEV)).cpu().numpy()
        assert np.array_equal(got, want), (n, got, want)


def ulp32(x):
    return np.spacing(np.abs(x.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize("k", range(len(R.ITEMS)))
def test_prepare_item_equals_the_reference(golden, k):
    g = golden("item2d3d")
    raw, opt, draws = R.make_item(k, int(g["i%d_seed" % k][0]))
    out = it.prepare_item(raw, device=DEV, **opt, **{n: torch.from_numpy(v).to(DEV) for n, v in draws.items()})
    for name in R.INT_KEYS:                                                  # every integer output is equal, and present exactly when the reference's is
        assert (name in out) == ("i%d_%s" % (k, name) in g.files), name
        if name in out:
            assert out[name].dtype == torch.int64 and np.array_equal(out[name].cpu().numpy(), g["i%d_%s" % (k, name)]), name
    for name in ("points", "transform"):                                     # the cast's own rounding: 1 float32 ulp of the reference's value
        got, want = out[name].cpu().numpy(), g["i%d_%s" % (k, name)]
        assert got.dtype == np.float32 and got.shape == want.shape
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print(name, "max error in ulp:", float((err / ulp32(want)).max()))
        assert np.all(err <= ulp32(want)), name
    # image: the reference's mean is a float64 pairwise sum over n = H W 3 terms of magnitude <= 1, off the exact mean by at most
    # (log2(n) + 16) 2^-53 (blocks of 128 summed eight-wide, pairwise above); ours likewise.  Both vanish under the float32 cast of
    # image - mean, whose own rounding is half an ulp; a value at a rounding boundary may fall to the other side: 1 float32 ulp in all.
    got, want = out["image"].cpu().numpy(), g["i%d_image" % k]
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("image max error in ulp:", float((err / ulp32(want)).max()))
    assert np.all(err <= ulp32(want))
    st = R.item_statement(raw, opt, draws)
    for name in ("intrinsics", "depth", "image_gray", "ori_image", "feats"):
        assert out[name].dtype == torch.float32 and np.array_equal(out[name].cpu().numpy(), st[name]), name
    assert out["image_h"] == raw["image"].shape[0] and out["image_w"] == raw["image"].shape[1] and out["scene_name"] == "scene"
    again = it.prepare_item(raw, device=DEV, **opt, **{n: torch.from_numpy(v).to(DEV) for n, v in draws.items()})
    for name, v in out.items():                                              # two runs are bit-equal
        assert torch.equal(v, again[name]) if torch.is_tensor(v) else v == again[name], name


def test_prepare_item_draws_from_a_generator_and_refuses_scale_augmentation(golden):
    g = golden("item2d3d")
    raw, opt, _ = R.make_item(0, int(g["i0_seed"][0]))
    outs = []
    for _ in range(2):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(11)
        outs.append(it.prepare_item(raw, device=DEV, generator=gen, **opt))
    assert outs[0]["points"].shape == (opt["max_points"], 3) and torch.equal(outs[0]["points"], outs[1]["points"])
    assert torch.equal(outs[0]["pcd_corr_indices"], outs[1]["pcd_corr_indices"])
    # the augmentation is rigid and the transform undoes it: the pairs' 3D distance stays inside the radius plus the noise
    o = outs[0]
    q = o["points"].double() @ o["transform"].double()[:3, :3].T + o["transform"].double()[:3, 3]
    z = o["depth"].double() / 1000.0
    K = o["intrinsics"].double()
    h, w = o["img_corr_pixels"][:, 0], o["img_corr_pixels"][:, 1]
    zz = z[h, w]
    p = torch.stack([(w - K[0, 2]) * zz / K[0, 0], ((h * o["image_w"] + w) / o["image_w"] - K[1, 2]) * zz / K[1, 1], zz], 1)
    assert o["pcd_corr_indices"].numel() > 0 and float((p - q[o["pcd_corr_indices"]]).norm(dim=1).max()) < opt["matching_radius_3d"] + 1e-5
    with pytest.raises(NotImplementedError):
        it.prepare_item(raw, device=DEV, scale_augmentation=True, **opt)
