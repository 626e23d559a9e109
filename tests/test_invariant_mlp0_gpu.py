"""The x half of mlp0 kept across denoise steps (loop.hip: PlHoist::x0_store / x0_use; pgemm.h: acc_store / acc_load) against the loop that
contracts it in every step.

mlp0 contracts [x | message] and x comes first.  In two per-step layer calls x stays during a loop call -- layer 0 on the src rows (x = the caller's
features) and layer 1's second cross call (x = the tgt rows of the once-per-call layer-0 output) -- so the accumulators at the segment boundary
are the same in every step: the first evaluation of a call stores them, the later ones start from them.  The claim is bit-identity, not a
tolerance, with the same launches in both arms.  The diagnostics knob DR_LOOP_HOIST_MLP0=0 runs the loop without the slabs."""
import os

import numpy as np
import pytest
import torch

from diffreg_hip import synth
from tests.helpers import pair, weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VARIANT, STEPS = "3dmatch", 3                 # C = 432: two column blocks of the 448-column geometry, 27 k-chunks per segment (odd: a virtual chunk)
FIELDS = ("conf_matrix_pred", "x_final", "R_forwd", "t_forwd", "x0", "cond")
# kernel form of the plane GEMMs -> (the knobs that force it, its number in dr_debug_pgemm_acc_forms)
FORMS = {"m16": ({"DR_PG_HALF": "0"}, 1), "rows128": ({"DR_PG_HALF": "0", "DR_PG_M16": "0"}, 2), "rows64": ({"DR_PG_HALF": "2"}, 3)}


def _engine(mc, variant=VARIANT):
    from diffreg_hip.engine import DenoiseEngine
    v = synth.VARIANTS[variant]
    return DenoiseEngine(weights(variant, "soft"), variant=variant, C=v["C"], H=v["H"], voxel=v["voxel"], origin=v["origin"], steps=STEPS,
                         sk_iters=v["skh_iters"], sample_rate=v["sample_rate"], max_condition_num=mc, n_layers=v["n_layers"], device=DEV, planes=True)


def _both_arms(monkeypatch, run, knobs=()):
    """run() with mlp0's x half contracted in every step (knob off), then with the slabs (the default); both under `knobs`.
    Each arm returns (what run() returned, the forms that stored / loaded accumulators during it)."""
    from diffreg_hip import lib
    lib.ensure_init()
    lib.raw().dr_debug_enable_env(1)
    try:
        for k, v in dict(knobs).items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("DR_LOOP_HOIST_MLP0", "0")
        lib.raw().dr_debug_pgemm_acc_forms(1)
        off = run()
        off_forms = lib.raw().dr_debug_pgemm_acc_forms(1)
        monkeypatch.delenv("DR_LOOP_HOIST_MLP0")
        on = run()
        on_forms = lib.raw().dr_debug_pgemm_acc_forms(1)
    finally:
        for k in dict(knobs):
            monkeypatch.delenv(k, raising=False)
        lib.raw().dr_debug_enable_env(1 if os.environ.get("DR_DIAGNOSTICS") == "1" else 0)      # (back to what lib.ensure_init had set)
    return (off, off_forms), (on, on_forms)


def _inputs(variant, P, N, M, seeds):
    ps = [pair(variant, N, M, s)[1] for s in seeds]
    return lambda k: torch.cat([q[k] for q in ps]).to(DEV)


def _profiled(eng, call):
    from diffreg_hip import lib
    lib.prof_collect()                        # (drop what earlier calls recorded)
    lib.prof_enable(True)
    try:
        out = call()
        prof = lib.prof_collect()
    finally:
        lib.prof_enable(False)
    ml = eng.match_list(out)                  # (checks the call's status word too)
    got = {k: out[k].clone() for k in FIELDS}
    got["matches"] = [m.clone() for m in ml]
    got["launches"] = {k: v[0] for k, v in prof.items()}
    return got


def _assert_same(off, on, P):
    assert on["launches"] == off["launches"], (on["launches"], off["launches"])        # the slabs cost no launch
    for k in FIELDS:
        assert torch.equal(off[k], on[k]), k
    assert len(off["matches"]) == P and all(torch.equal(a, b) for a, b in zip(off["matches"], on["matches"]))
    assert torch.isfinite(on["conf_matrix_pred"]).all() and on["conf_matrix_pred"].abs().max().item() > 0


# (P, N, M, seeds, max_condition_num), the shapes of test_invariant_projections_gpu.py: whole row blocks with N != M and, by the CPU oracle, a warp
# that is refused in step 0 and active in steps 1 and 2 | a partial last row block on both sides | one pair
SHAPES = [(2, 128, 256, (31, 32), 10.0), (2, 96, 160, (33, 34), 200.0), (1, 128, 128, (35,), 200.0)]


@pytest.mark.parametrize("form", ["m16", "rows64"])
@pytest.mark.parametrize("P,N,M,seeds,mc", SHAPES)
def test_loop_is_bitwise_the_loop_that_contracts_x_every_step(monkeypatch, P, N, M, seeds, mc, form):
    cat = _inputs(VARIANT, P, N, M, seeds)
    eng = _engine(mc)
    run = lambda: _profiled(eng, lambda: eng.run(cat("f_s"), cat("f_t"), cat("p_s"), cat("p_t"), cat("x_T"), trace=True, graph=False))
    knobs, f = FORMS[form]
    (off, off_forms), (on, on_forms) = _both_arms(monkeypatch, run, knobs)
    # the intended form ran, stored (step 0) and loaded (steps 1, 2) -- and no other; the knob-off arm touched no slab
    assert off_forms == 0 and on_forms == (1 << (f - 1)) | (1 << (4 + f - 1)), (off_forms, on_forms)
    _assert_same(off, on, P)
    if mc < 100:
        assert (on["cond"] > mc).any() and (on["cond"] <= mc).any(), on["cond"]       # refused in one step, active in another
    else:
        assert (on["cond"] <= mc).all(), on["cond"]


def test_generic_128_row_form_is_bitwise_too(monkeypatch):
    """the 128-row workgroups on the generic (32x32x16) main loop, which the 16x16x32 loop replaces by default: the partial-block shape"""
    P, N, M, seeds, mc = SHAPES[1]
    cat = _inputs(VARIANT, P, N, M, seeds)
    eng = _engine(mc)
    run = lambda: _profiled(eng, lambda: eng.run(cat("f_s"), cat("f_t"), cat("p_s"), cat("p_t"), cat("x_T"), trace=True, graph=False))
    knobs, f = FORMS["rows128"]
    (off, off_forms), (on, on_forms) = _both_arms(monkeypatch, run, knobs)
    assert off_forms == 0 and on_forms == (1 << (f - 1)) | (1 << (4 + f - 1)), (off_forms, on_forms)
    _assert_same(off, on, P)


def test_wide_wave_geometry_falls_back_and_stays_bitwise(monkeypatch):
    """4DMatch (C = 528): mlp0 runs on the wide-wave kernel, which keeps no accumulators between launches -- the loop keeps its launches as
    they were, no error status is set"""
    N, M, seeds = 128, 256, (31, 32)
    cat = _inputs("4dmatch", 2, N, M, seeds)
    noise = torch.from_numpy(np.stack([synth.step_noise(N, M, sd, STEPS) for sd in seeds], 1)).to(DEV)
    eng = _engine(40.0, "4dmatch")

    def run():
        out = eng.run(cat("f_s"), cat("f_t"), cat("p_s"), cat("p_t"), cat("x_T"), noise=noise, trace=True, graph=False)
        out["_status"].check()
        return {k: out[k].clone() for k in FIELDS}
    (off, off_forms), (on, on_forms) = _both_arms(monkeypatch, run)
    assert off_forms == 0 and on_forms == 0
    for k in off:
        assert torch.equal(off[k], on[k]), k
    assert torch.isfinite(on["conf_matrix_pred"]).all()


def test_graph_replays_equal_the_eager_call():
    """two replays of one captured call: every replay's step 0 stores the slabs again, so a replay does not depend on what the one before left"""
    P, N, M, seeds, mc = SHAPES[0]
    cat = _inputs(VARIANT, P, N, M, seeds)
    eng = _engine(mc)
    args = lambda: (cat("f_s"), cat("f_t"), cat("p_s"), cat("p_t"), cat("x_T"))
    eager = eng.run(*args(), trace=True, graph=False)
    eager["_status"].check()
    for _ in range(2):                        # (the shape has been seen: the first of these captures and replays, the second replays)
        # the slabs and every other buffer of the workspace hold the previous run's values when a replay starts
        got = eng.run(*args(), trace=True, graph=True)
        got["_status"].check()
        for k in FIELDS:
            assert torch.equal(eager[k], got[k]), k
        assert torch.equal(eager["matches_padded"], got["matches_padded"]) and torch.equal(eager["match_count"], got["match_count"])


def test_teacher_forced_call_is_bitwise_the_same_in_both_arms(monkeypatch):
    """force_x / force_R replace the state and the pose of every step; the features the slabs are built from are not theirs to replace"""
    P, N, M, seeds, mc = SHAPES[1]
    cat = _inputs(VARIANT, P, N, M, seeds)
    eng = _engine(mc)
    gen = torch.Generator().manual_seed(77)
    fx = torch.randn(STEPS, P, N, M, generator=gen, dtype=torch.float64)
    Rq, _ = torch.linalg.qr(torch.eye(3) + 0.2 * torch.randn(STEPS, P, 3, 3, generator=gen))
    Rq = Rq * torch.sign(torch.linalg.det(Rq))[..., None, None]
    force = dict(x=fx, R=Rq.float(), t=0.1 * torch.randn(STEPS, P, 3, 1, generator=gen))
    run = lambda: _profiled(eng, lambda: eng.run(cat("f_s"), cat("f_t"), cat("p_s"), cat("p_t"), cat("x_T"), trace=True, graph=False, force=force))
    (off, off_forms), (on, on_forms) = _both_arms(monkeypatch, run)
    assert off_forms == 0 and on_forms != 0
    _assert_same(off, on, P)


def test_trace_feature_outputs_keep_the_last_layers_fp32_rows(monkeypatch):
    """the loop drops the fp32 copy of the last layer's result unless the trace asks for the head's feature outputs, which are projected from it"""
    P, N, M, seeds, mc = SHAPES[2]
    cat = _inputs(VARIANT, P, N, M, seeds)
    eng = _engine(mc)
    names = ("src_feats", "tgt_feats", "src_feats_nopos", "tgt_feats_nopos", "conf_matrix_pred")

    def run():
        out = eng.run(cat("f_s"), cat("f_t"), cat("p_s"), cat("p_t"), cat("x_T"), graph=False, side_outputs=True)
        out["_status"].check()
        return {k: out[k].clone() for k in names}
    (off, _), (on, _) = _both_arms(monkeypatch, run)
    plain = eng.run(cat("f_s"), cat("f_t"), cat("p_s"), cat("p_t"), cat("x_T"), graph=False)       # (no trace: the fp32 rows are not written)
    for k in names:
        assert torch.equal(off[k], on[k]), k
        assert torch.isfinite(on[k]).all() and on[k].abs().max().item() > 0, k
    assert torch.equal(plain["conf_matrix_pred"], on["conf_matrix_pred"])
