"""The device optimizer (diffreg_hip.optim, csrc/optim.hip) against tests/optim_ref.py in float64 and torch's own float32 optimizers
on the same device.  Needs a GPU.

Every parameter, gradient and (from the second step on) state tensor is a view into a buffer between two guard bands (tests/helpers.guarded),
some starting 1, 2 or 3 floats behind a 16-byte boundary, with the offsets of one tensor's arrays equal for some tensors and different for others.
The sizes sit at the edges of the block -> (tensor, chunk, slot) map of csrc/optim_index.h, whose constants are read from the header.

The bar per tensor (case 1 and 4): max(one float32 ulp of the tensor's largest magnitude, 4 x the deviation of torch's own float32 optimizer on
the same device from the float64 statement).  Every test prints the largest error / bar ratio it met.
"""
import copy
import os
import re
import warnings

import numpy as np
import pytest
import torch

from diffreg_hip import optim as dopt
from tests import optim_ref as oref
from tests.helpers import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "diff-reg_amd", "csrc", "optim_index.h")).read()
_K = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, _HDR).group(1))
CHUNK, CAP = _K("OPT_BLOCK") * _K("OPT_VEC") * _K("OPT_UNROLL"), _K("OPT_CAP")

# (numel, 0-d?, offsets in floats of param, grad, state0, state1 behind a 16-byte boundary)
EDGES = [(0, False, (0, 0, 0, 0)), (1, True, (0, 0, 0, 0)), (3, False, (1, 1, 1, 1)), (4, False, (2, 2, 2, 2)), (5, False, (3, 3, 3, 3)),
         (CHUNK - 1, False, (1, 2, 3, 0)), (CHUNK, False, (0, 0, 0, 0)), (CHUNK + 1, False, (2, 2, 1, 2)), (2 * CHUNK + 3, False, (3, 3, 3, 3)),
         (CHUNK + 1, False, (1, 1, 1, 1)), (1, True, (3, 1, 2, 0))]
NO_GRAD = len(EDGES)                      # one more tensor, of 9 elements, never gets a gradient
BLOCK2 = [(7, False, ((i % 4,) * 4 if i % 3 else (i % 4, (i + 1) % 4, (i + 2) % 4, i % 4))) for i in range(CAP + 1)]


class TensorSet:
    """parameters with gradient views, all between guard bands; values drawn from `seed` on the host"""

    def __init__(self, spec, seed, with_no_grad=True):
        self.spec = list(spec)
        self.checks = []
        gen = torch.Generator().manual_seed(seed)
        self.gen = gen
        self.p0 = [torch.randn(n, generator=gen) for n, _, _ in self.spec]
        self.params = [self.view(n, scalar, off[0], v) for (n, scalar, off), v in zip(self.spec, self.p0)]
        for p, (n, scalar, off) in zip(self.params, self.spec):
            p.grad = self.view(n, scalar, off[1])
        self.no_grad = None
        if with_no_grad:
            self.no_grad = self.view(9, False, 1, torch.randn(9, generator=gen))
            self.no_grad0 = self.no_grad.clone()

    def view(self, n, scalar, off, values=None):
        buf, chk = guarded((n + off,), torch.float32, DEV, fill=0.0)
        self.checks.append(chk)
        v = buf[off:off + n]
        if scalar:
            v = v.reshape(())
        if values is not None:
            v.copy_(values.reshape(v.shape))
        return v

    def all_params(self):
        return self.params + ([self.no_grad] if self.no_grad is not None else [])

    def draw(self):
        """one step's gradients, on the host"""
        return [0.3 * torch.randn(n, generator=self.gen) for n, _, _ in self.spec]

    def set_grads(self, grads):
        for p, g in zip(self.params, grads):
            p.grad.copy_(g.reshape(p.shape))

    def misalign_states(self, opt):
        """move every state tensor into a guarded view at the offsets of the spec (the optimizer looks its states up at every step)"""
        for p, (n, scalar, off) in zip(self.params, self.spec):
            st = opt.state.get(p, {})
            for name, o in (("momentum_buffer", off[2]), ("exp_avg", off[2]), ("exp_avg_sq", off[3])):
                if st.get(name) is not None:
                    st[name] = self.view(n, scalar, o, st[name])

    def check_guards(self):
        for chk in self.checks:
            chk()


def _states(opt, p):
    st = opt.state.get(p, {}) if p in opt.state else {}
    names = ("momentum_buffer",) if isinstance(opt, torch.optim.SGD) else ("exp_avg", "exp_avg_sq")
    return [st.get(n) for n in names]


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _make(kind, params, opts, **kw):
    return getattr(torch.optim, kind)(params, **opts, **kw)


DIFFER = [0, 0]          # elements that are not bit-equal to torch's float32 result / elements compared (printed, not asserted)


def _hold(ts, opt, topt, tparams, ref):
    """every parameter and state of `opt` against the float64 statement, at the bar of the module docstring -> the largest error / bar"""
    worst = 0.0
    for i, (p, tp) in enumerate(zip(ts.params, tparams)):
        if p.numel() == 0:
            continue
        triples = [(p, tp, ref.p[i])] + list(zip(_states(opt, p), _states(topt, tp), (ref.s0[i], ref.s1[i])))
        for mine, theirs, want in triples:
            assert (mine is None) == (theirs is None) == (want is None), i
            if mine is None:
                continue
            want = want.reshape(-1)
            ulp = float(np.spacing(np.float32(np.abs(want).max())))
            bar = max(ulp, 4.0 * float(np.abs(_np64(theirs).reshape(-1) - want).max()))
            err = float(np.abs(_np64(mine).reshape(-1) - want).max())
            worst = max(worst, err / bar)
            DIFFER[0] += int((mine.reshape(-1) != theirs.reshape(-1)).sum())
            DIFFER[1] += mine.numel()
            assert err <= bar, (i, p.numel(), err, bar)
    return worst


def _case(name):
    if name in oref.SGD_CASES:
        return "SGD", oref.SGD_CASES[name]
    return oref.ADAM_CASES[name]


CASES = list(oref.SGD_CASES) + list(oref.ADAM_CASES)


@pytest.mark.parametrize("which", ["edges", "second_block"])
@pytest.mark.parametrize("case", CASES)
def test_three_steps_hold_the_float64_statement(case, which):
    kind, opts = _case(case)
    ts = TensorSet(EDGES if which == "edges" else BLOCK2, seed=11)
    opt = _make(kind, ts.all_params(), opts)
    acc = dopt.accelerate(opt, gate=True, zero_grads=False)
    tparams = [p0.to(DEV).reshape(p.shape).clone() for p0, p in zip(ts.p0, ts.params)]
    topt = _make(kind, tparams, opts, foreach=False)
    ref = oref.RefOptimizer(kind, [p0.numpy() for p0 in ts.p0], **opts)
    worst = 0.0
    for step in range(3):
        grads = ts.draw()
        ts.set_grads(grads)
        for tp, g in zip(tparams, grads):
            tp.grad = g.to(DEV).reshape(tp.shape).clone()
        opt.step()
        topt.step()
        ref.step([g.numpy() for g in grads])
        worst = max(worst, _hold(ts, opt, topt, tparams, ref))
        if step == 0:
            ts.misalign_states(opt)
    ts.check_guards()
    assert torch.equal(ts.no_grad, ts.no_grad0) and len(opt.state.get(ts.no_grad, {})) == 0       # no gradient: bit-unchanged and stateless
    assert dopt.steps_taken(opt) == 3 and dopt.skipped_steps(opt) == 0
    acc.remove()
    print("optim error / bar: case %s set %s largest ratio %.4f; %d of %d elements so far differ from torch's float32 bits" % ((case, which, worst) + tuple(DIFFER)))


def _snapshot(ts, opt):
    return [[t.clone() if t is not None else None for t in [p] + _states(opt, p)] for p in ts.params]


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for r, s in zip(a, b) for x, y in zip(r, s))


def _reference_rule(params):
    """validate_gradient, restated: no isnan and no isinf over all gradients"""
    return not any(bool(torch.isnan(p.grad).any()) or bool(torch.isinf(p.grad).any()) for p in params if p.grad is not None)


POISON = {"nan_last_element_of_last_tensor": (len(EDGES) + CAP, -1, float("nan")),
          "posinf_in_the_0d_tensor": (1, 0, float("inf")),
          "neginf_in_ragged_tail_of_misaligned": (8, -1, float("-inf")),       # 2 CHUNK + 3 elements, 3 floats behind the boundary
          "nan_in_second_argument_block": (len(EDGES) + CAP - 5, 3, float("nan"))}


@pytest.mark.parametrize("poison", list(POISON))
@pytest.mark.parametrize("case", ["shipped", "adam_wd"])
def test_gate_holds_the_step_back_and_history_goes_on(case, poison):
    kind, opts = _case(case)
    a, b = TensorSet(EDGES + BLOCK2, seed=23), TensorSet(EDGES + BLOCK2, seed=23)
    oa, ob = _make(kind, a.all_params(), opts), _make(kind, b.all_params(), opts)
    dopt.accelerate(oa, gate=True, zero_grads=True)
    dopt.accelerate(ob, gate=True, zero_grads=True)
    g1, g2, g3 = a.draw(), a.draw(), a.draw()
    for ts, o in ((a, oa), (b, ob)):
        ts.set_grads(g1)
        assert bool(dopt.gradients_valid(ts.all_params())) and _reference_rule(ts.params)
        o.step()
        ts.misalign_states(o)
    before = _snapshot(a, oa)
    taken, skipped = dopt.steps_taken(oa), dopt.skipped_steps(oa)
    # the poisoned step: `a` alone
    idx, elem, value = POISON[poison]
    a.set_grads(g2)
    a.params[idx].grad.view(-1)[elem] = value
    valid = dopt.gradients_valid(a.all_params())
    assert valid.dtype == torch.bool and valid.dim() == 0 and valid.is_cuda
    assert not bool(valid) and not _reference_rule(a.params)
    oa.step()
    oa.zero_grad()
    assert _same(_snapshot(a, oa), before)
    assert dopt.steps_taken(oa) == taken and dopt.skipped_steps(oa) == skipped + 1
    assert int(dopt.status_word(oa).item()) == 0
    assert all(bool((p.grad == 0).all()) for p in a.params)
    # the next finite step equals the step of the history that never saw the poisoned one
    for ts, o in ((a, oa), (b, ob)):
        ts.set_grads(g3)
        assert bool(dopt.gradients_valid(ts.all_params()))
        o.step()
    assert _same(_snapshot(a, oa), _snapshot(b, ob))
    assert all(bool((p.grad == 0).all()) for p in b.params)
    assert dopt.steps_taken(oa) == dopt.steps_taken(ob) == taken + 1 and dopt.skipped_steps(ob) == 0
    assert torch.equal(a.no_grad, a.no_grad0)
    a.check_guards()
    b.check_guards()


@pytest.mark.parametrize("case", ["shipped", "adam_wd"])
def test_captured_sequence_equals_eager_steps_and_runs_are_bit_equal(case):
    kind, opts = _case(case)
    sets = [TensorSet(EDGES + BLOCK2, seed=31) for _ in range(3)]
    opts_ = [_make(kind, ts.all_params(), opts) for ts in sets]
    for o in opts_:
        dopt.accelerate(o, gate=True, zero_grads=False)
    g1, g2 = sets[0].draw(), sets[0].draw()
    for ts, o in zip(sets, opts_):
        ts.set_grads(g1)
        o.step()                                     # creates the states, outside the capture
        ts.set_grads(g2)
    for ts, o in zip(sets[:2], opts_[:2]):           # two eager runs
        o.step()
        o.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                    # one stream: finite sweep(s), update(s), finish
        opts_[2].step()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    snaps = [_snapshot(ts, o) for ts, o in zip(sets, opts_)]
    assert _same(snaps[0], snaps[1])
    assert _same(snaps[0], snaps[2])
    assert [dopt.steps_taken(o) for o in opts_] == [3, 3, 3]
    if kind != "SGD":
        assert all(float(opts_[2].state[p]["step"]) == 3.0 for p in sets[2].params if p.numel())
    for ts in sets:
        ts.check_guards()


def _trajectory(kind, opts, ts, grads, lrs=None):
    """torch's float32 optimizer and the float64 statement over `grads` from the set's initial values -> (topt, tparams, ref)"""
    tparams = [p0.to(DEV).reshape(p.shape).clone() for p0, p in zip(ts.p0, ts.params)]
    topt = _make(kind, tparams, opts, foreach=False)
    ref = oref.RefOptimizer(kind, [p0.numpy() for p0 in ts.p0], **opts)
    for k, gs in enumerate(grads):
        for tp, g in zip(tparams, gs):
            tp.grad = g.to(DEV).reshape(tp.shape).clone()
        if lrs is not None:
            topt.param_groups[0]["lr"] = lrs[k]
        topt.step()
        ref.step([g.numpy() for g in gs], lr=None if lrs is None else lrs[k])
    return topt, tparams, ref


@pytest.mark.parametrize("case", ["shipped", "adam_wd"])
def test_state_dict_interchanges_with_the_plain_class(case):
    kind, opts = _case(case)
    ts = TensorSet(EDGES, seed=41, with_no_grad=False)
    grads = [ts.draw() for _ in range(3)]
    topt, tparams, ref = _trajectory(kind, opts, ts, grads)
    # accelerated for two steps -> plain torch for the third
    opt = _make(kind, ts.params, opts)
    acc = dopt.accelerate(opt)
    for gs in grads[:2]:
        ts.set_grads(gs)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    acc.remove()
    plain = _make(kind, ts.params, opts, foreach=False)
    plain.load_state_dict(sd)
    ts.set_grads(grads[2])
    plain.step()
    worst = _hold(ts, plain, topt, tparams, ref)
    # plain torch for two steps -> accelerated for the third, bound before (SGD) or after (Adam) the state is loaded
    ts2 = TensorSet(EDGES, seed=41, with_no_grad=False)
    plain2 = _make(kind, ts2.params, opts, foreach=False)
    for gs in grads[:2]:
        ts2.set_grads(gs)
        plain2.step()
    sd2 = copy.deepcopy(plain2.state_dict())
    opt2 = _make(kind, ts2.params, opts)
    if kind == "SGD":
        dopt.accelerate(opt2)
        opt2.load_state_dict(sd2)
    else:
        opt2.load_state_dict(sd2)
        dopt.accelerate(opt2)
        assert dopt.steps_taken(opt2) == 2
    ts2.set_grads(grads[2])
    opt2.step()
    worst = max(worst, _hold(ts2, opt2, topt, tparams, ref))
    ts.check_guards()
    ts2.check_guards()
    print("optim error / bar: interchange %s largest ratio %.4f" % (case, worst))


def test_a_scheduler_attached_before_accelerate_sets_the_kernels_lr():
    kind, opts = "SGD", dict(lr=0.1, momentum=0.9)
    ts = TensorSet(EDGES, seed=43, with_no_grad=False)
    grads = [ts.draw() for _ in range(3)]
    lrs = [0.1, 0.05, 0.025]
    topt, tparams, ref = _trajectory(kind, opts, ts, grads, lrs)
    opt = _make(kind, ts.params, opts)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.5)
    dopt.accelerate(opt)
    for k, gs in enumerate(grads):
        assert abs(opt.param_groups[0]["lr"] - lrs[k]) < 1e-15
        ts.set_grads(gs)
        opt.step()
        with warnings.catch_warnings():              # the scheduler finds its mark on the re-bound step and sees that it was called
            warnings.simplefilter("error")
            sched.step()
    worst = _hold(ts, opt, topt, tparams, ref)
    # the halved rates were used: the constant-rate trajectory is far outside the bar
    const = oref.RefOptimizer(kind, [p0.numpy() for p0 in ts.p0], **opts)
    for gs in grads:
        const.step([g.numpy() for g in gs])
    assert np.abs(const.p[6] - ref.p[6]).max() > 1e-3
    ts.check_guards()
    print("optim error / bar: scheduler largest ratio %.4f" % worst)


def test_version_bump_reaches_the_engine_and_remove_restores():
    from models.pipeline import Pipeline
    from tests.test_models_api_gpu import StubBackbone, ref_like_config
    model = Pipeline(ref_like_config("3dmatch", 20, 200.0), backbone=StubBackbone()).to(DEV).train()
    named = [(k, p) for k, p in model.named_parameters() if k.startswith("denoising_transformer.") or k.startswith("denoising_coarse_matching.")]
    assert named
    params = [p for _, p in named]
    opt = torch.optim.SGD(params, lr=0.015, momentum=0.93, weight_decay=1e-6)
    acc = dopt.accelerate(opt, gate=True, zero_grads=True)
    handed, held_back = params[:-1], params[-1]
    for p in handed:
        p.grad = torch.full_like(p, 1e-3)
    before = [p.detach().clone() for p in params]
    versions = [p._version for p in params]
    engine_version = model._weights_version()
    opt.step()
    opt.zero_grad()
    torch.cuda.synchronize()
    assert all(p._version > v for p, v in zip(handed, versions[:-1]))
    assert model._weights_version() != engine_version
    assert all(not torch.equal(p, q) for p, q in zip(handed, before[:-1]) if p.numel())
    assert torch.equal(held_back, before[-1]) and held_back.grad is None
    assert all(bool((p.grad == 0).all()) for p in handed)
    assert "step" in opt.__dict__
    acc.remove()
    assert "step" not in opt.__dict__ and "zero_grad" not in opt.__dict__ and opt.step.__func__ is type(opt).step
    with pytest.raises(ValueError):
        dopt.steps_taken(opt)


def _unbound(opt):
    return all(k not in opt.__dict__ for k in ("step", "zero_grad", "load_state_dict", "_diffreg_accelerated")) \
        and opt.step.__func__ is type(opt).step


def test_refusals_leave_nothing_bound_and_nothing_written():
    ok = torch.randn(33, device=DEV)
    ok.grad = torch.randn(33, device=DEV)
    # a float16 parameter
    half = torch.randn(8, device=DEV).half()
    half.grad = torch.ones_like(half)
    # a non-contiguous parameter
    strided = torch.randn(4, 6, device=DEV).t()
    strided.grad = torch.ones_like(strided)
    assert not strided.is_contiguous()
    for bad, make in ((half, lambda ps: torch.optim.SGD(ps, lr=0.1)), (strided, lambda ps: torch.optim.Adam(ps, lr=0.1)),
                      (None, lambda ps: torch.optim.Adam(ps, lr=0.1, amsgrad=True)), (None, lambda ps: torch.optim.AdamW(ps, lr=0.1, amsgrad=True)),
                      (None, lambda ps: torch.optim.Adam(ps, lr=0.1, capturable=True)), (None, lambda ps: torch.optim.RMSprop(ps, lr=0.1))):
        ps = [ok] + ([bad] if bad is not None else [])
        keep = [p.clone() for p in ps]
        opt = make(ps)
        with pytest.raises(NotImplementedError):
            dopt.accelerate(opt)
        assert _unbound(opt)
        assert all(torch.equal(p, k) for p, k in zip(ps, keep))
    # a closure: refused at the call, before any launch
    keep = ok.clone()
    opt = torch.optim.SGD([ok], lr=0.1, momentum=0.9)
    acc = dopt.accelerate(opt)
    with pytest.raises(NotImplementedError):
        opt.step(lambda: 0.0)
    torch.cuda.synchronize()
    assert torch.equal(ok, keep) and dopt.steps_taken(opt) == 0 and len(opt.state.get(ok, {})) == 0
    # a second optimizer binds and steps while the first stays bound
    ok.grad = None
    other = torch.randn(5, device=DEV)
    opt2 = torch.optim.SGD([other], lr=0.1)
    acc2 = dopt.accelerate(opt2)
    other.grad = torch.ones(5, device=DEV)
    opt2.step()
    torch.cuda.synchronize()
    assert dopt.steps_taken(opt2) == 1
    acc.remove()
    acc2.remove()
    assert _unbound(opt) and _unbound(opt2)


def test_a_strided_gradient_is_made_contiguous_and_still_zeroed():
    p = torch.randn(6, 4, device=DEV)
    p.grad = torch.randn(4, 6, device=DEV).t()
    assert not p.grad.is_contiguous()
    want, _ = oref.sgd_step(_np64(p), _np64(p.grad), None, lr=0.1)
    opt = torch.optim.SGD([p], lr=0.1)
    acc = dopt.accelerate(opt, zero_grads=True)
    opt.step()
    torch.cuda.synchronize()
    assert np.abs(_np64(p) - want).max() <= float(np.spacing(np.float32(np.abs(want).max())))
    assert bool((p.grad == 0).all())
    acc.remove()
