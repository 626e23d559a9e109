"""CPU checks of tests/nonrigid_gn_ref.py, the block-wise float64 restatement of vision3d's non_rigid_icp_gauss_newton that the GPU tests and the
timing tool lean on: it has to reproduce what the reference itself computed in float64 (tests/golden/nonrigid_gn.npz, nonrigid_gn_A.npz) at 1e-9."""
import os

import numpy as np
import pytest

from tests import nonrigid_gn_ref as G
from tests.conftest import GOLDEN

TOL = 1e-9
CASES = [(s, f) for s in G.SCENES for f in G.FORMS]


@pytest.fixture(scope="module")
def gold():
    return G.load(GOLDEN)


@pytest.fixture(scope="module")
def runs(gold):
    """every scene and form once: (rot, trn) after each recorded iteration count and the trace of the first iterations"""
    out = {}
    for s, f in CASES:
        inp = G.scene_inputs(gold, s)
        kw = G.form_args(inp, f)
        state, done, T = None, 0, {}
        trace = []
        for n in G.ITERS:
            rot, trn, tr = G.gauss_newton(inp["nodes"], inp["src"], inp["tgt"], inp["ai"], inp["aw"], inp["edges"], num_iterations=n - done,
                                          record=max(G.RECORD - done, 0), state=state, **kw)
            trace += tr
            state, done = (rot, trn), n
            T[n] = G.to34(rot, trn)
        out[(s, f)] = (T, trace)
    return out


def test_fixture_covers_every_scene_and_form(gold):
    for s, f in CASES:
        for n in G.ITERS:
            assert "%s_%s_T%d" % (s, f, n) in gold
        for it in range(G.RECORD):
            assert "%s_%s_b%d" % (s, f, it) in gold and "%s_%s_x%d" % (s, f, it) in gold
    sizes = {s: 6 * gold["%s_in_nodes" % s].shape[0] for s in G.SCENES}
    assert sizes["f"] == 60 and sizes["h"] == 66 and sizes["g"] == 3 * G.BLOCK and sizes["i"] == 2 * G.BLOCK + 22
    for f in G.FILES:
        assert os.path.getsize(os.path.join(GOLDEN, f)) <= 1 << 20
    for s in G.WARP:
        assert "%s_fn_warp5" % s in gold


@pytest.mark.parametrize("scene,form", CASES)
def test_restatement_reproduces_the_reference(gold, runs, scene, form):
    T, trace = runs[(scene, form)]
    key = "%s_%s_" % (scene, form)
    checked_A = 0
    for it in range(G.RECORD):
        for name in ("b", "x"):
            err = float(np.abs(trace[it][name] - gold[key + "%s%d" % (name, it)]).max())
            assert err <= TOL, (name, it, err)
        if key + "A%d" % it in gold:
            ref = gold[key + "A%d" % it]
            got = trace[it]["A"] if ref.ndim == 2 else G.tril_pack(trace[it]["A"])
            assert float(np.abs(got - ref).max()) <= TOL
            assert float(np.abs(trace[it]["A"] - trace[it]["A"].T).max()) <= 1e-12
            checked_A += 1
    M = gold["%s_in_nodes" % scene].shape[0]
    assert checked_A == (G.RECORD if G.has_A(scene, form, M) else 0)
    for n in G.ITERS:
        err = float(np.abs(T[n] - gold[key + "T%d" % n]).max())
        assert err <= TOL, (n, err)


def test_a_repeated_anchor_keeps_the_later_column(gold):
    """the rule the device documents for a row that names one node twice: the later column's block, once"""
    inp = G.scene_inputs(gold, "c")
    ai, aw = inp["ai"].copy(), inp["aw"].copy()
    ai[7, 0] = ai[7, 2]
    M = inp["nodes"].shape[0]
    eye, zero = np.tile(np.eye(3), (M, 1, 1)), np.zeros((M, 3))
    got = G.dense(*G.normal_blocks(eye, zero, inp["nodes"], inp["src"], inp["tgt"], ai, aw, inp["edges"]))[0]
    ai2, aw2 = ai.copy(), aw.copy()
    ai2[7, 0] = -1                                          # the same row with the earlier column absent from the Jacobian
    want = G.dense(*G.normal_blocks(eye, zero, inp["nodes"], inp["src"], inp["tgt"], ai2, aw, inp["edges"]))[0]
    # the residual still warps through both columns, so only A (which does not hold the residual) is compared
    assert np.array_equal(got, want)


def test_exp_so3_zero_is_identity():
    assert np.array_equal(G.exp_so3(np.zeros(3)), np.eye(3))
    Rm = G.exp_so3(np.array([0.3, -0.2, 0.5]))
    assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-15
