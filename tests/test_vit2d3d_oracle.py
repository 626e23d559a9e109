"""CPU: the restatement of the DINOv2 ViT encoder (tests/vit2d3d_ref.py) against the reference's own recorded outputs (tests/golden/vit2d3d_*.npz,
minted by tools/golden/make_golden_vit2d3d.py).  In float64 it reproduces every float64 tensor of the fixture to 1e-9; in fp16 it stays within
twice the fixture's own fp16 deviation.  That licenses it as the float64 yardstick for the shapes the fixture lacks (tests/test_vit2d3d_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import vit2d3d_ref as R

TENSORS = ["x_norm_patchtokens", "x_norm_clstoken", "x_prenorm", "pos", "inter0", "inter0_cls", "inter1", "inter1_cls"]


@pytest.fixture(scope="module")
def fx():
    f = R.load_fixture()
    assert f, "tests/golden/vit2d3d_*.npz are missing"
    return f


def run(vit, x):
    with torch.no_grad():
        ff = vit.forward_features(x)
        il = vit.get_intermediate_layers(x, [0, 1], return_class_token=True, norm=True)
        H, W = x.shape[-2:]
        L = 1 + (H // 14) * (W // 14)
        pos = vit.interpolate_pos_encoding(torch.zeros(1, L, 128, dtype=x.dtype), H, W)
    out = {k: ff[k] for k in ("x_norm_patchtokens", "x_norm_clstoken", "x_prenorm")}
    out["pos"] = pos
    for k, (o, c) in enumerate(il):
        out["inter%d" % k], out["inter%d_cls" % k] = o, c
    return {k: v.double().numpy() for k, v in out.items()}


@pytest.mark.parametrize("i", range(len(R.IMAGES)))
def test_float64_restatement_reproduces_the_reference(fx, i):
    vit = R.fixture_vit(fx, torch.float64)
    got = run(vit, torch.from_numpy(fx["img%d.x" % i]).double())
    for k in TENSORS:
        ref = fx["img%d.f64.%s" % (i, k)]
        assert got[k].shape == ref.shape, k
        assert np.abs(got[k] - ref).max() <= 1e-9, (k, np.abs(got[k] - ref).max())


@pytest.mark.parametrize("i", range(len(R.IMAGES)))
def test_fp16_restatement_within_twice_the_reference_fp16_deviation(fx, i):
    vit = R.fixture_vit(fx, torch.float16)
    got = run(vit, torch.from_numpy(fx["img%d.x" % i]))
    for k in TENSORS:
        ref64, ref16 = fx["img%d.f64.%s" % (i, k)], fx["img%d.f16.%s" % (i, k)]
        own = np.abs(ref16 - ref64).max()
        assert np.abs(got[k] - ref64).max() <= 2 * own, (k, np.abs(got[k] - ref64).max(), own)


def test_fixture_exercises_what_it_claims(fx):
    assert [1 + (h // 14) * (w // 14) for h, w in R.IMAGES] == [16, 26, 131]
    # the square, same-size image takes the early return of interpolate_pos_encoding: its position rows ARE the trained grid
    assert np.array_equal(fx["img1.f64.pos"][0], fx["w.pos_embed"][0].astype(np.float64))
    assert not np.array_equal(fx["img0.f64.pos"][0, 1:], fx["w.pos_embed"][0, 1:16].astype(np.float64))
    for k, v in fx.items():
        if k.startswith("w."):
            assert v.dtype == np.float16, k
