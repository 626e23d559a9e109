"""CPU checks of the 3D / 4D dataset item: the float64 restatement (tests/item3d_ref.py) against the fixture minted from the reference's own
__getitem__ bodies (tests/golden/item3d.npz), and the screening that lets the GPU tests compare every pair of every list."""
import numpy as np
import pytest

from tests import item3d_ref as R

KINDS = [("3dmatch", k) for k in range(len(R.CASES_3D))] + [("4dmatch", k) for k in range(len(R.CASES_4D))]


def load(golden, kind, k):
    g = golden("item3d")
    pre = "%s_%d_" % (kind, k)
    c = {name[len(pre):]: g[name] for name in g.files if name.startswith(pre)}
    raw = dict(src=c["in_src"], tgt=c["in_tgt"], rot=c["in_rot"], trans=c["in_trans"])
    if kind == "4dmatch":
        raw["flow"] = c["in_flow"]
    draws = {name[5:]: c[name] for name in c if name.startswith("draw_")}
    cs = (R.CASES_3D if kind == "3dmatch" else R.CASES_4D)[k]
    return c, raw, draws, cs


@pytest.mark.parametrize("kind,k", KINDS)
def test_restatement_equals_the_reference(golden, kind, k):
    c, raw, draws, cs = load(golden, kind, k)
    noise = R.NOISE_3D if kind == "3dmatch" else R.NOISE_4D
    assert np.array_equal(R.scene(kind, k, int(c["seed"][0]))["src"], raw["src"])              # the scene is the recorded seed's
    out = R.prepare(kind, raw, draws, cs[2], cs[3], noise)
    for name in ("src", "tgt") + (("flow",) if kind == "4dmatch" else ()):
        ref = c["out_" + name]
        assert out[name].dtype == ref.dtype and out[name].shape == ref.shape, name
        # the same numpy operations on the same dtypes; a BLAS may sum a 3-term product in another order: a few float64 ulps at most
        assert np.abs(out[name].astype(np.float64) - ref.astype(np.float64)).max() <= 4 * np.spacing(np.abs(ref).max() + 1.0), name
    assert np.array_equal(out["rot"].astype(np.float32), c["out_rot"]) and np.array_equal(out["trans"].astype(np.float32), c["out_trans"])
    if cs[3]:
        assert (draws["coin"] > 0.5) == cs[4]                                                   # the branch the case asks for
        turned = "src" if cs[4] else "tgt"
        assert c["out_" + turned].dtype == np.float64 and c["out_" + ("tgt" if cs[4] else "src")].dtype == np.float32
    if kind == "3dmatch":
        pairs = R.radius_pairs(c["out_src"], c["out_tgt"], c["out_rot"], c["out_trans"], R.OVERLAP_RADIUS)
        assert np.array_equal(pairs, c["out_corr"])
    else:
        assert np.array_equal(c["out_corr"], c["in_corr"])
        if cs[5]:
            assert np.array_equal(c["out_metric_index"], c["in_metric_index"].squeeze())


@pytest.mark.parametrize("k", range(len(R.CASES_3D)))
def test_screening_leaves_no_pair_out(golden, k):
    """no distance within GAPR of the radius, for the reference's own float64 clouds and for their float32 roundings the device reads: the
    excluded share is 0"""
    c, _, _, _ = load(golden, "3dmatch", k)
    for cast in (np.float64, np.float32):
        src, tgt = c["out_src"].astype(cast), c["out_tgt"].astype(cast)
        assert R.near_radius(src, tgt, c["out_rot"], c["out_trans"], R.OVERLAP_RADIUS) == 0
        assert np.array_equal(R.radius_pairs(src, tgt, c["out_rot"], c["out_trans"], R.OVERLAP_RADIUS), c["out_corr"])


def test_unselected_flow_is_in_the_fixture(golden):
    c, raw, draws, cs = load(golden, "4dmatch", 3)
    assert c["out_src"].shape == (100, 3) and c["out_flow"].shape == (300, 3) and np.array_equal(c["out_flow"], raw["flow"])


def test_euler_restatement():
    for seed in range(5):
        a = np.random.default_rng(seed).random(3) * 2 * np.pi
        M = R.euler_zyx(a)
        assert np.abs(M @ M.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(M) - 1) < 1e-14
    # extrinsic z, then y, then x
    assert np.allclose(R.euler_zyx([np.pi / 2, 0, 0]) @ [1, 0, 0], [0, 1, 0]) and np.allclose(R.euler_zyx([0, 0, np.pi / 2]) @ [0, 1, 0], [0, 0, 1])
    from diffreg_hip.item3d import euler_zyx_matrix
    import torch
    a = np.random.default_rng(9).random((4, 3)) * 2 * np.pi
    got = euler_zyx_matrix(torch.from_numpy(a)).numpy()
    assert max(np.abs(got[i] - R.euler_zyx(a[i])).max() for i in range(4)) < 1e-15
