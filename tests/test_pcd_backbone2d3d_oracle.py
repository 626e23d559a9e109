"""CPU: the float64 restatement of the 2D-3D point backbone (tests/pcd_backbone2d3d_ref.py) against the fixture minted by running the reference's own
PointBackbone (tools/golden/make_golden_pcd_backbone2d3d.py): the pyramid checksums, the float64 loss, all 110 parameter gradients and the output
column sums to 1e-9 of each tensor's maximum, the stored (quantised) output rows to half a quantisation step + 1e-9, and every KPConv call's
neighbour counts exactly."""
import numpy as np
import pytest
import torch

from tests import pcd_backbone2d3d_ref as R

SCENES = ("a", "c")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("pcd_backbone2d3d")


@pytest.fixture(scope="module")
def runs(golden):
    res = {}
    for name in SCENES:
        pyr = R.make_pyramid(name)
        m = R.PointBackbone().double()
        m.load_state_dict({**m.state_dict(), **R.make_weights(m)})
        m = m.double()
        d = {k: [t.double() if t.is_floating_point() else t for t in v] for k, v in R.to_torch(pyr).items()}
        counts = []
        outs = m(torch.ones(d["points"][0].shape[0], 1, dtype=torch.float64), d, counts)
        loss = R.loss_of(outs, R.loss_weights(outs))
        loss.backward()
        res[name] = dict(pyr=pyr, outs=[o.detach() for o in outs], loss=float(loss.detach()), counts=counts,
                         grads={n: R.sub_grad(p.grad).numpy() for n, p in m.named_parameters()}, out=golden("pcd_backbone2d3d_%s_out" % name))
    return res


@pytest.mark.parametrize("name", SCENES)
def test_pyramid_is_the_minted_one(fx, runs, name):
    pyr = runs[name]["pyr"]
    assert np.array_equal(R.pyramid_checksum(pyr), fx[name + "_pyramid_checksum"])
    assert max(a.shape[1] for k in ("neighbors", "subsampling", "upsampling") for a in pyr[k]) <= 64
    if name == "c":
        n1 = pyr["points"][1].shape[0]
        assert (pyr["upsampling"][0] == n1).all(1).any(), "scene c must hold an all-shadow interpolation row"
        assert ((pyr["neighbors"][0] < pyr["points"][0].shape[0]).sum(1) == 1).any(), "scene c must hold a one-entry neighbour list"


@pytest.mark.parametrize("name", SCENES)
def test_restatement_float64_vs_reference(fx, runs, name):
    r = runs[name]
    assert abs(r["loss"] - float(fx[name + "_loss64"][0])) <= 1e-9 * abs(float(fx[name + "_loss64"][0]))
    n = 0
    for k in fx.files:
        if k.startswith(name + "_g64_"):
            pname = k[len(name + "_g64_"):]
            ref, got = fx[k], r["grads"][pname]
            assert got.shape == ref.shape, pname
            assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max(), pname
            n += 1
    assert n == 110
    for i, o in enumerate(r["outs"]):
        assert tuple(fx["%s_out%d_shape" % (name, i)]) == tuple(o.shape)
        cs = fx["%s_out%d_colsum64" % (name, i)]
        assert np.abs(o.sum(0).numpy() - cs).max() <= 1e-9 * np.abs(cs).max(), i
        step = r["out"]["out%d_step" % i]
        ref = R.dequantise(r["out"]["out%d_q" % i], step)
        got = o[::R.OUT_ROWS[name]].numpy()
        assert np.abs(got - ref).max() <= 0.5 * float(step[0]) + 1e-9 * np.abs(got).max(), i
    for ci, c in enumerate(r["counts"]):
        assert np.array_equal(c.numpy(), fx["%s_counts_%02d" % (name, ci)].astype(np.int64)), ci
