"""The closing leg of a training iteration on the device: gradient gate + SGD / Adam / AdamW update.

The reference's trainers end an iteration with a per-tensor isnan / isinf loop that reads the host twice per parameter tensor
(`validate_gradient`, 3D/lib/utils.py:96-106, called at lib/trainer.py:195-201; `check_gradients`, vision3d/engine/base_trainer.py:311-325), then
`optimizer.step()` and `zero_grad()`.  `accelerate` re-binds `step` on the optimizer INSTANCE to four kinds of launches of libdiffreg_hip.so --
the finite sweep over every group (dr_grads_finite_multi_f32), one gated update per group (dr_sgd_step_multi_f32 / dr_adam_step_multi_f32) and
dr_optim_finish -- with no host read anywhere, and returns the undo:

    acc = optim.accelerate(optimizer, gate=True, zero_grads=True)     # NotImplementedError for what it refuses, nothing left bound
    loss.backward(); optimizer.step(); optimizer.zero_grad()          # the trainer's lines, minus `if validate_gradient(model):`
    optim.skipped_steps(optimizer), optim.steps_taken(optimizer)      # one host read each, for the epoch log
    acc.remove()

The state stays in torch's own layout in `optimizer.state` (`momentum_buffer`; `exp_avg`, `exp_avg_sq`, `step`), so state_dict() /
load_state_dict() interchange with the unaccelerated class, and a scheduler that holds the optimizer keeps working (lr is read from the group at
every step).  Adam's `step` entries are 0-d float32 views of ONE device array that dr_optim_finish rewrites from the one device counter of the
optimizer; binding (or loading) existing state reads them once on the host and requires them to be equal.

What differs from torch, all of it where the host cannot know whether the device took a step:
  * a parameter that gets its first gradient at a later step joins with the optimizer's counter, not with a counter of its own (Adam's bias
    correction), and SGD's first-step rule `buf = g` is taken from the counter: a late joiner starts from a zero buffer, which is the same value
    unless dampening != 0;
  * state tensors are created (zero) at the first step that hands a parameter over, also when that step is gated off;
  * `_version` of every handed-over parameter is bumped at every step(), also when it is gated off;
  * steps_taken() of an SGD counts from the binding (torch keeps no step count for SGD); step hooks registered on the optimizer are not run.
"""
import array
import ctypes

import torch

from . import lib

_WORD, _STEP, _SKIPPED = 0, 1, 2


def _refuse(msg):
    raise NotImplementedError("diffreg_hip.optim: " + msg)


def _descriptors(rows):
    """rows of (param, grad, state0, state1, numel) as addresses -> (buffer of dr_optim_tensor, its address, count)"""
    flat = array.array("Q")
    for r in rows:
        flat.extend(r)
    return flat, ctypes.c_void_p(flat.buffer_info()[0]), len(rows)


def _check_tensor(t, what):
    if t.is_sparse or t.layout != torch.strided:
        _refuse("%s is sparse" % what)
    if not t.is_cuda:
        _refuse("%s is not on a ROCm device; there is no CPU path" % what)
    if t.dtype != torch.float32:
        _refuse("%s is %s; the kernels take float32 only" % (what, t.dtype))


def _grad_of(p):
    """the float32 contiguous gradient to hand over (a non-contiguous one is made contiguous first) -> (tensor, is_copy)"""
    g = p.grad
    _check_tensor(g, "a gradient")
    if g.is_contiguous():
        return g, False
    return g.contiguous(), True


class AcceleratedOptimizer:
    """what accelerate() returns: remove() restores the instance"""

    def __init__(self, optimizer, gate, zero_grads):
        kind = type(optimizer)
        if isinstance(optimizer, torch.optim.SGD):
            self.kind = "sgd"
        elif isinstance(optimizer, torch.optim.Adam):            # AdamW is a subclass of Adam (decoupled_weight_decay)
            self.kind = "adam"
        elif isinstance(optimizer, torch.optim.AdamW):
            self.kind = "adam"
        else:
            _refuse("%s is not torch.optim.SGD, Adam or AdamW" % kind.__name__)
        self.optimizer, self.gate, self.zero_grads = optimizer, bool(gate), bool(zero_grads)
        self._params = [p for g in optimizer.param_groups for p in g["params"]]
        if not self._params:
            _refuse("the optimizer has no parameters")
        for group in optimizer.param_groups:
            self._check_group(group)
        dev = self._params[0].device
        for p in self._params:
            _check_tensor(p, "a parameter")
            if not p.is_contiguous():
                _refuse("a parameter is not contiguous")
            if p.device != dev:
                _refuse("the parameters lie on more than one device")
            if p.grad is not None:
                _check_tensor(p.grad, "a gradient")
        self.device = dev
        self._index = {id(p): i for i, p in enumerate(self._params)}
        self._ctrl = torch.zeros(4, dtype=torch.int32, device=dev)              # status word, step counter, skipped counter
        self._mirror = torch.zeros(len(self._params) if self.kind == "adam" else 0, dtype=torch.float32, device=dev)
        self._zeroed = False
        self._adopt_state()
        # bound last: a refusal above leaves the instance as it was
        self._saved = {k: optimizer.__dict__[k] for k in ("step", "zero_grad", "load_state_dict") if k in optimizer.__dict__}
        self._load_state_dict = optimizer.load_state_dict
        self._zero_grad = optimizer.zero_grad
        def step(closure=None):
            return self.step(closure)
        if hasattr(optimizer.step, "_wrapped_by_lr_sched"):      # a scheduler bound before us marked torch's step; it looks for its mark
            step._wrapped_by_lr_sched = True
        optimizer.step = step
        optimizer.load_state_dict = self.load_state_dict
        if self.zero_grads:
            optimizer.zero_grad = self.zero_grad
        optimizer._diffreg_accelerated = self

    # ---- binding ---------------------------------------------------------------------------------------------------------------------
    def _check_group(self, group):
        if group.get("amsgrad"):
            _refuse("amsgrad is not provided")
        if group.get("capturable") or group.get("differentiable"):
            _refuse("capturable / differentiable optimizers are not supported (the accelerated step is capturable as it is)")
        for k in ("lr", "weight_decay", "momentum", "dampening", "eps"):
            if torch.is_tensor(group.get(k)):
                _refuse("a tensor %s would need a host read per step; pass a float" % k)
        if any(torch.is_tensor(b) for b in group.get("betas", ())):
            _refuse("tensor betas would need a host read per step; pass floats")

    def _state_tensor(self, t, p, name):
        if not (torch.is_tensor(t) and t.is_cuda and t.device == p.device and t.dtype == torch.float32 and t.is_contiguous()
                and t.shape == p.shape):
            _refuse("the existing state %s of a parameter is not a contiguous float32 tensor of its shape on its device" % name)

    def _adopt_state(self):
        """existing optimizer.state -> the device counter.  One host read of Adam's step entries, which must be equal."""
        st_of = self.optimizer.state
        if self.kind == "sgd":
            have = False
            for p in self._params:
                buf = st_of.get(p, {}).get("momentum_buffer")
                if buf is not None:
                    self._state_tensor(buf, p, "momentum_buffer")
                    have = True
            self._ctrl[_STEP] = 1 if have else 0            # SGD's first-step rule needs zero / non-zero only
            return
        held = [p for p in self._params if "step" in st_of.get(p, {})]
        steps = set()
        if held:
            for p in held:
                self._state_tensor(st_of[p].get("exp_avg"), p, "exp_avg")
                self._state_tensor(st_of[p].get("exp_avg_sq"), p, "exp_avg_sq")
            vals = [st_of[p]["step"] for p in held]
            if all(torch.is_tensor(v) and v.is_cuda for v in vals):
                steps = set(torch.stack([v.reshape(()).float() for v in vals]).cpu().tolist())
            else:
                steps = set(float(v) for v in vals)
            if len(steps) != 1:
                _refuse("the parameters' Adam step counts differ (%s); one device counter serves the optimizer" % sorted(steps))
        n = int(steps.pop()) if steps else 0
        self._ctrl[_STEP] = n
        self._mirror.fill_(float(n))
        for p in held:
            st_of[p]["step"] = self._mirror[self._index[id(p)]]

    def remove(self):
        opt = self.optimizer
        if getattr(opt, "_diffreg_accelerated", None) is not self:
            return
        for k in ("step", "zero_grad", "load_state_dict"):
            if k in self._saved:
                opt.__dict__[k] = self._saved[k]
            else:
                opt.__dict__.pop(k, None)
        del opt._diffreg_accelerated

    # ---- the re-bound methods ----------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        self._load_state_dict(state_dict)
        self._params = [p for g in self.optimizer.param_groups for p in g["params"]]
        for group in self.optimizer.param_groups:
            self._check_group(group)
        self._adopt_state()

    def zero_grad(self, set_to_none=True):
        """the first zero_grad() after an accelerated step() is the pass the update kernels already made (the gradients stay allocated and are
        zero: zero_grad(set_to_none=False)); any other call is torch's"""
        if self._zeroed:
            self._zeroed = False
            return
        self._zero_grad(set_to_none=set_to_none)

    def _rows(self, group):
        """the group's parameters that have a gradient -> (descriptor rows, parameters, gradient copies to zero by hand)"""
        st_of = self.optimizer.state
        rows, params, copies = [], [], []
        sgd = self.kind == "sgd"
        momentum = group["momentum"] != 0 if sgd else False
        for p in group["params"]:
            if p.grad is None:
                continue
            i = self._index.get(id(p))
            if i is None:
                _refuse("a parameter was added after accelerate(); remove() and accelerate again")
            g, copied = _grad_of(p)
            if copied:
                copies.append((p, g))
            s0 = s1 = 0
            if sgd:
                if momentum:
                    st = st_of[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    s0 = buf.data_ptr()
            else:
                st = st_of[p]
                if "step" not in st:
                    st["step"] = self._mirror[i]
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                s0, s1 = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            rows.append((p.data_ptr(), g.data_ptr(), s0, s1, p.numel()))
            params.append(p)
        return rows, params, copies

    def step(self, closure=None):
        if closure is not None:
            _refuse("step(closure) would re-evaluate the model between the launches; call the closure yourself")
        opt = self.optimizer
        with torch.no_grad(), torch.cuda.device(self.device):
            work = [(group,) + self._rows(group) for group in opt.param_groups]      # every refusal happens before the first launch
            raw = lib.raw()
            stream = lib.stream_of(self._ctrl)
            base = self._ctrl.data_ptr()
            word, step, skipped = (ctypes.c_void_p(base + 4 * k) for k in (_WORD, _STEP, _SKIPPED))
            lib.ensure_init()
            sets = [_descriptors(rows) for _, rows, _, _ in work]
            if self.gate:
                for _, addr, n in sets:
                    if n:
                        lib.check(raw.dr_grads_finite_multi_f32(addr, n, word, stream))
            handed = []
            for (group, rows, params, copies), (_, addr, n) in zip(work, sets):
                if not n:
                    continue
                if self.kind == "sgd":
                    o = lib.SgdOptions(group["lr"], group["weight_decay"], group["momentum"], group["dampening"], int(group["nesterov"]),
                                       int(group["maximize"]), int(self.zero_grads))
                    lib.check(raw.dr_sgd_step_multi_f32(addr, n, ctypes.byref(o), word, step, stream))
                else:
                    b1, b2 = group["betas"]
                    o = lib.AdamOptions(group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                        int(bool(group.get("decoupled_weight_decay", False))), int(group["maximize"]), int(self.zero_grads))
                    lib.check(raw.dr_adam_step_multi_f32(addr, n, ctypes.byref(o), word, step, stream))
                handed += params
                if self.zero_grads:
                    for p, _ in copies:                      # the kernel zeroed the contiguous copy, not the strided original
                        p.grad.zero_()
            lib.check(raw.dr_optim_finish(word, step, skipped, lib.ptr(self._mirror) if self._mirror.numel() else None,
                                          self._mirror.numel(), stream))
            if handed:
                # the kernels write through raw pointers: without this the caches keyed on _version (Pipeline._weights_version) go stale
                torch.autograd.graph.increment_version(handed)
        self._zeroed = self.zero_grads
        opt._opt_called = True                               # what torch's own step wrapper tells a scheduler


def accelerate(optimizer, gate=True, zero_grads=False):
    """Re-bind `optimizer.step` (and `zero_grad` when zero_grads=True) on the instance to the library's launches; -> the object whose remove()
    restores it.  gate=True: a step whose gradients hold a NaN or an Inf anywhere in any group writes nothing and is counted by skipped_steps().
    zero_grads=True: the update pass also zeroes the gradients, and the zero_grad() that follows a step() does nothing more.
    NotImplementedError, with nothing bound: an optimizer other than SGD / Adam / AdamW, amsgrad, capturable / differentiable, a sparse gradient,
    a parameter that is not a contiguous float32 tensor on one ROCm device, tensor hyper-parameters, Adam step counts that differ; at step(): a
    closure, a gradient that is not float32."""
    if getattr(optimizer, "_diffreg_accelerated", None) is not None:
        _refuse("the optimizer is accelerated already; remove() first")
    return AcceleratedOptimizer(optimizer, gate, zero_grads)


def _acc(optimizer):
    acc = getattr(optimizer, "_diffreg_accelerated", None)
    if acc is None:
        raise ValueError("diffreg_hip.optim: the optimizer is not accelerated")
    return acc


def skipped_steps(optimizer):
    """steps the gate held back since accelerate() (one host read)"""
    return int(_acc(optimizer)._ctrl[_SKIPPED].item())


def steps_taken(optimizer):
    """the device step counter (one host read): Adam's step count; for SGD the steps since accelerate() (+ 1 when it was bound with momentum
    buffers present)"""
    return int(_acc(optimizer)._ctrl[_STEP].item())


def status_word(optimizer):
    """the gate's device status word as a 1-element int32 view (bits DR_GRAD_NAN 1, DR_GRAD_POS_INF 2, DR_GRAD_NEG_INF 4): zero between steps"""
    return _acc(optimizer)._ctrl[_WORD:_WORD + 1]


def gradients_valid(model_or_params):
    """validate_gradient(model) (3D/lib/utils.py:96-106) as a 0-d bool DEVICE tensor, with no host read: True when no gradient of the module's /
    the iterable's parameters holds a NaN or an Inf.  Parameters without a gradient are passed over, as the reference passes them over."""
    params = model_or_params.parameters() if isinstance(model_or_params, torch.nn.Module) else model_or_params
    grads = [_grad_of(p)[0] for p in params if p.grad is not None]
    if not grads:
        raise ValueError("diffreg_hip.optim.gradients_valid: no parameter has a gradient (the device to answer on is unknown)")
    dev = grads[0].device
    if any(g.device != dev for g in grads):
        _refuse("the gradients lie on more than one device")
    with torch.cuda.device(dev):
        word = torch.zeros(1, dtype=torch.int32, device=dev)
        lib.ensure_init()
        _, addr, n = keep = _descriptors([(0, g.data_ptr(), 0, 0, g.numel()) for g in grads])
        lib.check(lib.raw().dr_grads_finite_multi_f32(addr, n, lib.ptr(word), lib.stream_of(word)))
        del keep
        return (word == 0).reshape(())
