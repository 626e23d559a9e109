"""CPU: the restatement in tests/finenoise2d3d_ref.py against the fixture minted from the reference itself (tests/golden/finenoise2d3d.npz,
tools/golden/make_golden_finenoise2d3d.py), and the fixture rules on the scenes (cap on undecided cases: 0)."""
import os

import numpy as np
import pytest
import torch

from tests import finenoise2d3d_ref as F
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "finenoise2d3d.npz"))
DT = {"32": torch.float32, "64": torch.float64}
TOL = {"32": 2e-5, "64": 1e-10}       # float32: summation order of the same float32 ops; float64: the same arithmetic


def close(a, b, tol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.size:
        assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-30), (what, np.abs(a - b).max(), np.abs(b).max())


@pytest.mark.parametrize("name", list(F.FINE_CASES))
def test_fine_scene_obeys_the_fixture_rules(name):
    sc = F.make_fine_scene(**F.FINE_CASES[name])
    px, idx = F.select(sc)
    assert F.fixture_rules(sc, px, idx) == []
    if name == "sub":
        assert sc["pcd_corr_indices"].shape[0] > F.FINE_CFG["max_correspondences"] and px.shape[0] == 256
    if name == "dup":
        assert px.shape[0] < 256 and len(set(idx.tolist())) < idx.shape[0]


@pytest.mark.parametrize("tag", ["32", "64"])
@pytest.mark.parametrize("name", list(F.FINE_CASES))
def test_fine_restatement_matches_the_reference(name, tag):
    sc = F.make_fine_scene(**F.FINE_CASES[name])
    px, idx = F.select(sc)
    loss, recall, gi, gp = F.fine_loss_and_grads(sc, px, idx, DT[tag])
    ref_loss = float(G["fine_%s_loss%s" % (name, tag)])
    if name == "empty":
        assert np.isnan(ref_loss) and bool(torch.isnan(loss)) and float(gi.abs().max()) == 0.0
    else:
        assert abs(float(loss) - ref_loss) <= TOL[tag] * abs(ref_loss)
    assert float(recall) == pytest.approx(float(G["fine_%s_recall%s" % (name, tag)]), abs=1e-6)
    rows = px[:, 0] * sc["image_w"] + px[:, 1]
    close(gi[rows][:, ::F.GRAD_COL_STRIDE], G["fine_%s_gimg%s" % (name, tag)], TOL[tag] * 10, "img")
    close(gp[idx][:, ::F.GRAD_COL_STRIDE], G["fine_%s_gpcd%s" % (name, tag)], TOL[tag] * 10, "pcd")


@pytest.mark.parametrize("name", list(F.WARP_CASES))
def test_ladder_fit_matches_the_reference(name):
    c = F.make_warp_case(**F.WARP_CASES[name])
    out = F.soft_procrustes(c["matrix_gt"], c["s_pcd"], c["t_pcd"], c["src_mask"], c["tgt_mask"], F.WARP_HP["sample_rate"], F.WARP_HP["max_cond"])
    for k, v in zip(("R", "t", "R_forwd", "t_forwd"), out):
        close(v, G["ladder_%s_%s32" % (name, k)], 1e-5, k)
    assert bool(out[5][0]) == bool(G["ladder_%s_mask32" % name][0])
    close(out[4], G["ladder_%s_condition32" % name], 1e-3, "condition")


@pytest.mark.parametrize("name", list(F.WARP_CASES))
def test_warp_restatement_matches_the_reference(name):
    c = F.make_warp_case(**F.WARP_CASES[name])
    r32, r64 = F.warp_and_grads(c, torch.float32), F.warp_and_grads(c, torch.float64)
    ok, s64 = F.topk_rule(r64["conf"], c["src_mask"], c["tgt_mask"], F.WARP_HP["sample_rate"])
    assert ok and s64 == F.topk_rule(r32["conf"], c["src_mask"], c["tgt_mask"], F.WARP_HP["sample_rate"])[1]
    assert bool(r32["mask"][0]) == bool(G["warp_%s_mask32" % name][0]) == bool(G["warp_%s_mask64" % name][0]) == (name == "fit")
    for k in ("R", "t", "R_forwd", "t_forwd", "warped"):
        close(r32[k], G["warp_%s_%s32" % (name, k)], 1e-4, k)
        close(r64[k], G["warp_%s_%s64" % (name, k)], 1e-4, k)          # (the reference's float64 run fits in float32: its own casts)
    close(r32["condition"], G["warp_%s_condition32" % name], 1e-3, "condition")
    close(r32["g_bin"], G["warp_%s_gbin32" % name], 1e-3, "g_bin")
    close(r64["g_bin"], G["warp_%s_gbin64" % name], 1e-3, "g_bin")
    close(r64["g_scores"], G["warp_%s_gscores64" % name], 1e-3, "g_scores")
    if name == "gated":
        assert float(r64["g_bin"]) == 0.0 and float(r64["g_scores"].abs().max()) == 0.0
        assert torch.equal(r32["warped"], c["s_pcd"])
    else:
        assert abs(float(G["warp_fit_gbin64"])) > 1e-3                    # the term `noising=True` restores is not small here


@pytest.mark.parametrize("t", [0, 417, 999])
def test_q_sample_restatement_is_bit_equal(t):
    g = torch.from_numpy(F._gauss((1, 24, 40), 21)).float()
    x0 = (torch.from_numpy(F._hash01(np.arange(24 * 40), 22).reshape(1, 24, 40)) > 0.9).float()
    out = F.q_sample(x0, torch.tensor([t]), g, 1000)
    assert out.dtype == torch.float64 and np.array_equal(out.numpy(), G["qsample_t%d" % t])


def test_cached_q_sample_is_bit_equal_on_the_cpu():
    from diffreg_hip import autograd2d3d
    g = torch.from_numpy(F._gauss((1, 24, 40), 21)).float()
    x0 = (torch.from_numpy(F._hash01(np.arange(24 * 40), 22).reshape(1, 24, 40)) > 0.9).float()
    for t in (0, 417, 999, 417):
        out = autograd2d3d.q_sample(x_start=x0, t=torch.tensor([t]), noise=g, timesteps=1000)
        assert out.dtype == torch.float64 and np.array_equal(out.numpy(), G["qsample_t%d" % t])
