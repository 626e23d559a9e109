"""The once-per-call projections of the plane path (loop.hip: fill_step_invariants) against the per-step projections they replace.

Layer 0's q | k | v of the src rows are projected once per call up to the rotary step (the input is the caller's feat0; only the src position
code moves) and a row-wise kernel applies the step's code and writes the q / k images; the q image of layer 1's second cross call (tgt rows) is
written once.  The claim is bit-identity, not a tolerance: the same accumulators, the rotary arithmetic as the GEMM epilogues round it, the same bound
and split.  The diagnostics knob DR_LOOP_HOIST=0 runs the loop with the per-step projections."""
import os

import pytest
import torch

from diffreg_hip import synth
from tests.helpers import pair, weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANT, STEPS = "3dmatch", 3                 # C = 432, H = 4: the geometry whose head dim 108 is padded to 112


def _engine(mc, variant=VARIANT):
    from diffreg_hip.engine import DenoiseEngine
    v = synth.VARIANTS[variant]
    return DenoiseEngine(weights(variant, "soft"), variant=variant, C=v["C"], H=v["H"], voxel=v["voxel"], origin=v["origin"], steps=STEPS,
                         sk_iters=v["skh_iters"], sample_rate=v["sample_rate"], max_condition_num=mc, n_layers=v["n_layers"], device=DEV, planes=True)


def _both_arms(monkeypatch, run):
    """run() with the per-step projections (knob off), then with the once-per-call ones (the default)"""
    from diffreg_hip import lib
    lib.ensure_init()
    lib.raw().dr_debug_enable_env(1)
    try:
        monkeypatch.setenv("DR_LOOP_HOIST", "0")
        off = run()
        monkeypatch.delenv("DR_LOOP_HOIST")
        on = run()
    finally:
        lib.raw().dr_debug_enable_env(1 if os.environ.get("DR_DIAGNOSTICS") == "1" else 0)      # (back to what lib.ensure_init had set)
    return off, on


# (P, N, M, seeds, max_condition_num): whole-workgroup groups with N != M (the inline group bound) and, by the CPU oracle, a warp that is refused
# in step 0 (condition numbers 42.2 / 14.1 > 10) and active in steps 1 and 2 (8.1, 9.7 / 7.4, 8.7): the src code stays, then moves | rows that are
# no multiple of 128 (launch_group_max, a partial last row block, a tgt side that starts inside a row block), warp active throughout | one pair
@pytest.mark.parametrize("P,N,M,seeds,mc", [(2, 128, 256, (31, 32), 10.0), (2, 96, 160, (33, 34), 200.0), (1, 128, 128, (35,), 200.0)])
def test_loop_is_bitwise_the_loop_with_per_step_projections(monkeypatch, P, N, M, seeds, mc):
    ps = [pair(VARIANT, N, M, s)[1] for s in seeds]
    cat = lambda k: torch.cat([q[k] for q in ps]).to(DEV)
    eng = _engine(mc)

    def run():
        from diffreg_hip import lib
        lib.prof_collect()                    # (drop what earlier calls recorded)
        lib.prof_enable(True)
        try:
            out = eng.run(cat("f_s"), cat("f_t"), cat("p_s"), cat("p_t"), cat("x_T"), trace=True, graph=False)
            prof = lib.prof_collect()
        finally:
            lib.prof_enable(False)
        ml = eng.match_list(out)              # (checks the call's status word too)
        got = {k: out[k].clone() for k in ("conf_matrix_pred", "x_final", "R_forwd", "t_forwd", "x0", "cond")}
        got["matches"] = [m.clone() for m in ml]
        got["launches"] = {k: v[0] for k, v in prof.items()}
        return got
    off, on = _both_arms(monkeypatch, run)
    # the two arms did run different launches: one row-wise rotary kernel per step (family position_code) in place of layer 0's projection launch;
    # once per call two launches for layer 0 and one for layer 1's q
    assert on["launches"]["position_code"] == off["launches"]["position_code"] + STEPS, (on["launches"], off["launches"])
    assert on["launches"]["gemm_split"] == off["launches"]["gemm_split"] - STEPS + 3, (on["launches"], off["launches"])
    for k in ("conf_matrix_pred", "x_final", "R_forwd", "t_forwd", "x0"):
        assert torch.equal(off[k], on[k]), k
    assert len(off["matches"]) == P and all(torch.equal(a, b) for a, b in zip(off["matches"], on["matches"]))
    assert torch.isfinite(on["conf_matrix_pred"]).all() and on["conf_matrix_pred"].abs().max().item() > 0
    if mc < 100:
        assert (on["cond"] > mc).any() and (on["cond"] <= mc).any(), on["cond"]       # refused in one step, active in another
    else:
        assert (on["cond"] <= mc).all(), on["cond"]


def test_wide_wave_geometry_is_bitwise_the_loop_with_per_step_projections(monkeypatch):
    """4DMatch (C = 528, heads padded 132 -> 144): the projections run on the wide-wave kernel, whose rotary rounds its odd elements in another
    order than the 448-column kernel's -- the row-wise kernel follows the kernel it stands in for"""
    import numpy as np
    N, M, seeds = 128, 256, (31, 32)
    ps = [pair("4dmatch", N, M, s)[1] for s in seeds]
    cat = lambda k: torch.cat([q[k] for q in ps]).to(DEV)
    noise = torch.from_numpy(np.stack([synth.step_noise(N, M, sd, STEPS) for sd in seeds], 1)).to(DEV)
    eng = _engine(40.0, "4dmatch")

    def run():
        out = eng.run(cat("f_s"), cat("f_t"), cat("p_s"), cat("p_t"), cat("x_T"), noise=noise, trace=True, graph=False)
        out["_status"].check()
        return {k: out[k].clone() for k in ("conf_matrix_pred", "x_final", "R_forwd", "t_forwd", "x0")}
    off, on = _both_arms(monkeypatch, run)
    for k in off:
        assert torch.equal(off[k], on[k]), k
    assert torch.isfinite(on["conf_matrix_pred"]).all()


def test_ragged_call_is_bitwise_the_call_with_per_step_projections(monkeypatch):
    """pairs of different sizes padded to (128, 256) with DR_LOOP_RAGGED on the plane path: masked rows and columns"""
    sizes = [(128, 256), (96, 160)]
    ps = [pair(VARIANT, n, m, 41 + i)[1] for i, (n, m) in enumerate(sizes)]
    items = [dict(src_feats=q["f_s"][0].to(DEV), tgt_feats=q["f_t"][0].to(DEV), s_pcd=q["p_s"][0].to(DEV), t_pcd=q["p_t"][0].to(DEV),
                  x_T=q["x_T"][0].to(DEV)) for q in ps]
    eng = _engine(200.0)

    def run():
        got = eng.run_ragged(items)
        return [{k: g[k].clone() for k in ("conf_matrix_pred", "R_final", "t_final", "match_pred")} for g in got]
    off, on = _both_arms(monkeypatch, run)
    for a, b in zip(off, on):
        for k in a:
            assert torch.equal(a[k], b[k]), k
        assert torch.isfinite(b["conf_matrix_pred"]).all()


@pytest.mark.parametrize("C,wide", [(432, False), (528, True)])
def test_rotary_image_kernel_writes_the_gemm_epilogues_bytes(C, wide):
    """dr_rotary_planes_f32 alone: from the rows a PL_F32 launch without rotary wrote, the q / k images and bounds equal, byte for byte, what the
    PL_PLANES launch with rotary writes for the same inputs.  130 rows: one full 128-row block and a partial one; rows of zeros, of denormal
    scale, of 1e-30 and of 1e4 beside ordinary ones."""
    from diffreg_hip import lib
    rows = 130
    torch.manual_seed(C)
    x = torch.randn(rows, C, device=DEV) * (torch.rand(rows, 1, device=DEV) * 5 + 0.01)
    x[0] = 0
    x[1] *= 1e-39
    x[2] *= 1e-30
    x[3] *= 1e4
    x[129] *= 1e-3
    img, bnd = lib.planes_from_f32(x)
    W = torch.randn(2 * C, C, device=DEV) / C ** 0.5
    ang = torch.rand(rows, C // 2, device=DEV) * 6.28
    cosT, sinT = ang.cos().contiguous(), ang.sin().contiguous()
    csT = torch.stack([cosT, sinT], -1).contiguous()
    nbytes = lib.raw().dr_plane_image_bytes(rows, C)
    # the reference: one PL_PLANES launch per block (each block its own image and bound array, as q | k | v in the loop)
    ref_img = torch.zeros(2, nbytes, dtype=torch.uint8, device=DEV)
    ref_bnd = torch.zeros(2, rows, device=DEV)
    for b in range(2):
        pk = lib.pack_weight_planes(W[b * C:(b + 1) * C], 1, C, wide=wide)
        lib.linear_planes(rows, C, 1, img, bnd, C, pk, lib.PL_PLANES, cos_t=cosT, sin_t=sinT, rot_mask=1, rot_C=C, out_image=ref_img[b],
                          out_image_k=C, out_bound=ref_bnd[b], wide=wide)
    # the two halves: projection up to the rotary step, then the kernel under test
    pk2 = lib.pack_weight_planes(W, 2, C, wide=wide)
    pre = torch.full((rows, 2 * C), float("nan"), device=DEV)
    lib.linear_planes(rows, C, 2, img, bnd, C, pk2, lib.PL_F32, out=pre, ldo=2 * C, blk_stride=C, wide=wide)
    got_img = torch.zeros(2, nbytes, dtype=torch.uint8, device=DEV)
    got_bnd = torch.zeros(2, rows, device=DEV)
    lib.rotary_planes(pre, C, C, 2, csT, 3, C, bnd, pk2, C, got_img, nbytes, got_bnd, rows, wide=wide)
    torch.cuda.synchronize()
    assert torch.isfinite(pre).all()
    assert torch.equal(got_bnd.view(torch.int32), ref_bnd.view(torch.int32))
    assert torch.equal(got_img, ref_img)
    assert ref_img[:, : nbytes // 2].any() and ref_bnd[0, 0].item() == 0.0 and ref_bnd[0, 5].item() > 0      # (the reference did write; the zero row's bound is 0)
