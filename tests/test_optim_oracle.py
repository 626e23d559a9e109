"""The checker's side of the device optimizer, on the CPU: tests/optim_ref.py -- the float64 statements the GPU tests hold
diffreg_hip.optim to -- against torch.optim.{SGD, Adam, AdamW} on float64 CPU tensors, and the twelfth set of ABI entries in the header, in the
ctypes table and in the built library."""
import os
import re

import numpy as np
import pytest
import torch

from tests import optim_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(), (3,), (5, 7), (129,), (0,)]
ENTRIES = ("dr_grads_finite_multi_f32", "dr_sgd_step_multi_f32", "dr_adam_step_multi_f32", "dr_optim_finish")


def _inputs(seed, steps=3):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g, dtype=torch.float64) for s in SHAPES]
    grads = [[0.3 * torch.randn(s, generator=g, dtype=torch.float64) for s in SHAPES] for _ in range(steps)]
    return params, grads


def _hold(ref, opt, tparams, state_names):
    """both sides are float64 statements of one formula: 1e-12 of each tensor's maximum"""
    for i, p in enumerate(tparams):
        pairs = [(ref.p[i], p.detach().numpy())]
        for name, mine in zip(state_names, (ref.s0[i], ref.s1[i])):
            theirs = opt.state[p].get(name) if p in opt.state else None
            assert (mine is None) == (theirs is None), (i, name)
            if mine is not None:
                pairs.append((mine, theirs.numpy()))
        for mine, theirs in pairs:
            if theirs.size:
                assert np.abs(mine - theirs).max() <= 1e-12 * max(np.abs(theirs).max(), 1e-300), i


@pytest.mark.parametrize("case", list(oref.SGD_CASES))
def test_sgd_statement_is_torchs(case):
    opts = oref.SGD_CASES[case]
    params, grads = _inputs(3)
    tparams = [p.clone().requires_grad_(True) for p in params]
    opt = torch.optim.SGD(tparams, **opts)
    ref = oref.RefOptimizer("SGD", [p.numpy() for p in params], **opts)
    for gs in grads:
        for p, g in zip(tparams, gs):
            p.grad = g.clone()
        opt.step()
        ref.step([g.numpy() for g in gs])
        _hold(ref, opt, tparams, ("momentum_buffer",))


@pytest.mark.parametrize("case", list(oref.ADAM_CASES))
def test_adam_statement_is_torchs(case):
    cls, opts = oref.ADAM_CASES[case]
    params, grads = _inputs(4)
    tparams = [p.clone().requires_grad_(True) for p in params]
    opt = getattr(torch.optim, cls)(tparams, **opts)
    ref = oref.RefOptimizer(cls, [p.numpy() for p in params], **opts)
    for t, gs in enumerate(grads):
        for p, g in zip(tparams, gs):
            p.grad = g.clone()
        opt.step()
        ref.step([g.numpy() for g in gs])
        _hold(ref, opt, tparams, ("exp_avg", "exp_avg_sq"))
        assert all(float(opt.state[p]["step"]) == t + 1 == ref.t for p in tparams)


def test_a_tensor_without_gradient_is_passed_over():
    params, grads = _inputs(5, steps=1)
    ref = oref.RefOptimizer("Adam", [p.numpy() for p in params], lr=1e-3)
    gs = [g.numpy() for g in grads[0]]
    gs[2] = None
    ref.step(gs)
    assert np.array_equal(ref.p[2], params[2].numpy()) and ref.s0[2] is None and ref.s1[2] is None
    assert not np.array_equal(ref.p[1], params[1].numpy())


def test_gate_statement_is_the_references_rule():
    clean = [np.ones(4), np.zeros(()), np.full(3, 3.0e38, np.float32)]
    assert oref.grads_valid(clean) and oref.grads_valid([])
    for bad in (np.nan, np.inf, -np.inf):
        g = [a.copy() for a in clean]
        g[1] = np.array(bad)
        assert not oref.grads_valid(g)
        # the reference's loop, verbatim on torch tensors
        assert any(bool(torch.any(torch.isnan(torch.from_numpy(np.atleast_1d(a))))) or bool(torch.any(torch.isinf(torch.from_numpy(np.atleast_1d(a)))))
                   for a in g)


def test_twelfth_set_is_declared_bound_and_exported():
    import ctypes

    from diffreg_hip import lib
    header = open(os.path.join(ROOT, "include", "diffreg_hip.h")).read()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in lib.SIGNATURES, name
        assert hasattr(so, name), name
    for struct in ("dr_optim_tensor", "dr_sgd_options", "dr_adam_options"):
        assert re.search(r"\} %s;" % struct, header), struct
    assert re.search(r"#define DR_ABI_VERSION 700\b", header) and lib.ABI_VERSION == 700 and lib.raw().dr_version() == 700
    # the ctypes structs have the header's layout: five 8-byte words; four / five doubles and three ints
    assert ctypes.sizeof(lib.OptimTensor) == 40 and ctypes.sizeof(lib.SgdOptions) == 48 and ctypes.sizeof(lib.AdamOptions) == 56


def test_entries_refuse_bad_arguments_before_any_launch():
    """argument checks that return before the first launch run without a device"""
    import ctypes

    from diffreg_hip import lib
    raw = lib.raw()
    word = ctypes.c_void_p(16)
    assert raw.dr_grads_finite_multi_f32(None, 1, word, None) == -1                 # a count without an array
    assert raw.dr_grads_finite_multi_f32(None, 0, None, None) == -1                 # no status word
    assert raw.dr_grads_finite_multi_f32(None, 0, word, None) == 0                  # an empty set launches nothing
    t = (lib.OptimTensor * 2)(lib.OptimTensor(16, 18, 0, 0, 4), lib.OptimTensor(0, 0, 0, 0, 0))
    assert raw.dr_grads_finite_multi_f32(t, 2, word, None) == -1                    # a gradient off the 4-byte grid
    empty = (lib.OptimTensor * 1)(lib.OptimTensor(0, 0, 0, 0, 0))
    o = lib.SgdOptions(0.1, 0.0, 0.9, 0.0, 0, 0, 0)
    assert raw.dr_sgd_step_multi_f32(empty, 1, ctypes.byref(o), word, word, None) == 0        # numel == 0 is skipped, pointers unseen
    need = (lib.OptimTensor * 1)(lib.OptimTensor(16, 32, 0, 0, 4))
    assert raw.dr_sgd_step_multi_f32(need, 1, ctypes.byref(o), word, word, None) == -1        # momentum without a buffer
    bad = lib.SgdOptions(0.1, 0.0, 0.0, 0.0, 1, 0, 0)
    assert raw.dr_sgd_step_multi_f32(empty, 1, ctypes.byref(bad), word, word, None) == -1     # nesterov without momentum (torch's ValueError)
    a = lib.AdamOptions(1e-3, 0.9, 1.0, 1e-8, 0.0, 0, 0, 0)
    assert raw.dr_adam_step_multi_f32(empty, 1, ctypes.byref(a), word, word, None) == -1      # beta2 outside [0, 1)
    assert raw.dr_optim_finish(None, word, None, None, 0, None) == -1
