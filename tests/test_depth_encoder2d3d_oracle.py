"""tests/depth_encoder2d3d_ref.py (the plain-torch restatement of Depth-Anything's ViT encoder) against the reference's own recorded outputs
(tests/golden/depth_encoder2d3d_*.npz, minted by tools/golden/make_golden_depth_encoder2d3d.py from the hub's DinoVisionTransformer).  CPU only.

In float64 the restatement is within 1e-9 (max |difference|) of every stored tensor; in float32 it is within 2 x the deviation the reference's own
float32 run had from its float64 run (recorded per tensor): DESIGN 5q's rule."""
import pytest
import torch

from tests import depth_encoder2d3d_ref as R


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def test_fixture_shape(fx):
    vit = R.fixture_vit(fx, torch.float32)
    assert sum(p.numel() for p in vit.parameters()) == 873344 - 128          # the hub class's count without its mask_token
    for i, (H, W) in enumerate(R.IMAGES):
        L = 1 + (H // 14) * (W // 14)
        assert fx["img%d.x" % i].shape == (1, 3, H, W) and fx["img%d.f64.x_prenorm" % i].shape == (1, L, 128)
        for n in R.TENSORS:
            assert fx["img%d.dev32.%s" % (i, n)] > 0


@pytest.mark.parametrize("img", range(len(R.IMAGES)))
def test_restatement_in_float64(fx, img):
    vit = R.fixture_vit(fx, torch.float64)
    x = torch.from_numpy(fx["img%d.x" % img]).double()
    got = R.run_all(vit, x)
    H, W = R.IMAGES[img]
    with torch.no_grad():
        pos = vit.interpolate_pos_encoding(torch.zeros(1, 1 + (H // 14) * (W // 14), 128, dtype=torch.float64), H, W)
    assert (pos - torch.from_numpy(fx["img%d.f64.pos" % img])).abs().max() <= 1e-9
    for n in R.TENSORS:
        ref = torch.from_numpy(fx["img%d.f64.%s" % (img, n)])
        assert got[n].shape == ref.shape, n
        e = (got[n] - ref).abs().max().item()
        assert e <= 1e-9, (n, e)


@pytest.mark.parametrize("img", range(len(R.IMAGES)))
def test_restatement_in_float32(fx, img):
    vit = R.fixture_vit(fx, torch.float32)
    got = R.run_all(vit, torch.from_numpy(fx["img%d.x" % img]))
    for n in R.TENSORS:
        ref, d = torch.from_numpy(fx["img%d.f64.%s" % (img, n)]), float(fx["img%d.dev32.%s" % (img, n)])
        e = (got[n].double() - ref).abs().max().item()
        assert e <= 2 * d, (n, e, d)


def test_regtokens_entry_is_empty(fx):
    vit = R.fixture_vit(fx, torch.float32)
    with torch.no_grad():
        out = vit.forward_features(torch.from_numpy(fx["img0.x"]))
    assert tuple(out["x_norm_regtokens"].shape) == (1, 0, 128) and out["masks"] is None
