"""The edges of the layer schedule (loop_common.h: layer_schedule) that the six-layer tests never reach, on both engines and both GEMM paths:
n_layers = 1 (layer 0 only: the buffer of the once-per-call half is the result), 2 (the cross layer that reads the cached operands is the last
one) and 3 (the walk ends on a self layer).  The forced plane path and the f32 path are two evaluations of the same network: each is held to
1e-4 of the reference by the suite's contract, so they agree within 2e-4 (DESIGN.md section 4 measured <= 8e-6 at six layers)."""
import pytest
import torch

from diffreg_hip import synth
from tests.helpers import T, pair, weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, MC, TOL = 2, 200.0, 2e-4


def _check(outs):
    (a, sa), (b, sb) = outs
    for out, status in outs:
        status.check()                                              # the call's own status word
        for k in ("conf_matrix_pred", "x0", "R_forwd", "t_forwd"):
            assert torch.isfinite(out[k]).all() and out[k].abs().max().item() > 0, k
        assert (out["cond"] <= MC).all(), out["cond"]               # the warp was active in every step
    for k in ("conf_matrix_pred", "R_forwd", "t_forwd"):
        err = (a[k] - b[k]).abs().max().item()
        print(k, err)
        assert err < TOL, (k, err)
    err = (a["x0"][-1] - b["x0"][-1]).abs().max().item()
    print("x0[-1]", err)
    assert err < TOL, err


@pytest.mark.parametrize("n_layers", [1, 2, 3])
def test_3dmatch_plane_path_is_the_f32_path_at_short_schedules(n_layers):
    from diffreg_hip.engine import DenoiseEngine
    variant, N, M = "3dmatch", 96, 160
    v = synth.VARIANTS[variant]
    ps = [pair(variant, N, M, s)[1] for s in (33, 34)]
    cat = lambda k: torch.cat([q[k] for q in ps]).to(DEV)
    outs = []
    for planes in (True, False):
        eng = DenoiseEngine(weights(variant, "soft"), variant=variant, C=v["C"], H=v["H"], voxel=v["voxel"], origin=v["origin"], steps=STEPS,
                            sk_iters=v["skh_iters"], sample_rate=v["sample_rate"], max_condition_num=MC, n_layers=n_layers, device=DEV, planes=planes)
        out = eng.run(cat("f_s"), cat("f_t"), cat("p_s"), cat("p_t"), cat("x_T"), trace=True)
        outs.append((out, out["_status"]))
    _check(outs)


@pytest.mark.parametrize("n_layers", [1, 2, 3])
def test_2d3d_plane_path_is_the_f32_path_at_short_schedules(n_layers):
    from diffreg_hip.engine import DenoiseEngine2D3D
    N, M = 96, 160
    Wn = synth.make_weights_2d3d(seed=9, head_gain=16.0)
    W = {k: T(a) for k, a in Wn.items()}
    pr = synth.make_pair_2d3d(N, M, 31, weights=Wn)
    d = lambda k: T(pr[k])[None].to(DEV)
    outs = []
    for planes in (True, False):
        eng = DenoiseEngine2D3D(W, steps=STEPS, max_condition_num=MC, n_layers=n_layers, device=DEV, planes=planes)
        out = eng.run(d("img_feats"), d("img_dino"), d("img_pixels"), d("pcd_feats"), d("s_pcd"), d("t_pcd_da"), d("x_T"), trace=True)
        outs.append((out, out["_status"]))
    _check(outs)
