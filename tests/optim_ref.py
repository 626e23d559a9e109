"""float64 statements of the optimizer updates and of the gradient gate that diffreg_hip.optim runs on the device, written from
torch's documentation of torch.optim.SGD, Adam and AdamW -- numpy, one tensor at a time, nothing in place.

    sgd_step    g <- -g (maximize);  g <- g + lambda theta;  b <- g at the first step, else mu b + (1 - tau) g;
                g <- g + mu b (nesterov) | b;  theta <- theta - gamma g
    adam_step   g <- -g (maximize);  Adam: g <- g + lambda theta | AdamW: theta <- theta - gamma lambda theta;
                m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;  theta <- theta - gamma (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps)
    grads_valid the reference's rule (3D/lib/utils.py:96-106): no NaN and no Inf in any gradient
"""
import numpy as np


def sgd_step(p, g, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False):
    """-> (p, buf); buf is None before the first step and stays None when momentum == 0"""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    if maximize:
        g = -g
    if weight_decay != 0:
        g = g + weight_decay * p
    if momentum != 0:
        buf = g.copy() if buf is None else momentum * np.asarray(buf, np.float64) + (1.0 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    return p - lr * g, buf


def adam_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, maximize=False):
    """t: the number of this step, from 1 -> (p, m, v); m and v are None before the first step"""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    m = np.zeros_like(p) if m is None else np.asarray(m, np.float64)
    v = np.zeros_like(p) if v is None else np.asarray(v, np.float64)
    b1, b2 = betas
    if maximize:
        g = -g
    if weight_decay != 0:
        if decoupled:
            p = p - lr * weight_decay * p
        else:
            g = g + weight_decay * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    m_hat = m / (1.0 - b1 ** t)
    v_hat = v / (1.0 - b2 ** t)
    return p - lr * m_hat / (np.sqrt(v_hat) + eps), m, v


def grads_valid(grads):
    return not any(bool(np.isnan(g).any()) or bool(np.isinf(g).any()) for g in grads)


# the option combinations the tests run, as keyword arguments of torch.optim.<class>
SGD_CASES = {
    "plain": dict(lr=0.015),
    "shipped": dict(lr=0.015, momentum=0.93, weight_decay=1e-6),           # the 3D yaml: main.py:90-96
    "dampening": dict(lr=0.015, momentum=0.93, dampening=0.1),
    "nesterov": dict(lr=0.015, momentum=0.93, nesterov=True, weight_decay=1e-6),
    "maximize": dict(lr=0.015, momentum=0.93, weight_decay=1e-6, maximize=True),
}
ADAM_CASES = {
    "adam": ("Adam", dict(lr=1e-3)),
    "adam_wd": ("Adam", dict(lr=1e-3, weight_decay=1e-2)),
    "adamw": ("AdamW", dict(lr=1e-3, weight_decay=1e-2, betas=(0.8, 0.99), eps=1e-6)),
    "adam_maximize": ("Adam", dict(lr=1e-3, weight_decay=1e-4, maximize=True)),
}


class RefOptimizer:
    """the float64 trajectory of a list of tensors under one of the cases above; entries of `grads` may be None (the tensor is passed over)"""

    def __init__(self, kind, params, **opts):
        self.kind, self.opts = kind, dict(opts)
        self.p = [np.asarray(p, np.float64) for p in params]
        self.s0 = [None] * len(self.p)
        self.s1 = [None] * len(self.p)
        self.t = 0

    def step(self, grads, lr=None):
        o = dict(self.opts)
        if lr is not None:
            o["lr"] = lr
        self.t += 1
        for i, g in enumerate(grads):
            if g is None:
                continue
            if self.kind == "SGD":
                self.p[i], self.s0[i] = sgd_step(self.p[i], g, self.s0[i], **o)
            else:
                self.p[i], self.s0[i], self.s1[i] = adam_step(self.p[i], g, self.s0[i], self.s1[i], self.t, decoupled=self.kind == "AdamW", **o)
