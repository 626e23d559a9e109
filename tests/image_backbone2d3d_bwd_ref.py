"""Shared by the image backbone's backward tests and the tool that mints their fixture (tools/golden/make_golden_image_backbone2d3d_bwd.py):
the cotangents of the loss  sum_i <out_i, cot_i>, the order of the gradient tensors, and the loader of the fixture, which is stored in parts
(tests/golden/image_backbone2d3d_bwd.npz holds the index, the recorded deviations and the small tensors; image_backbone2d3d_bwd_<n>.npz the rest,
so that no file exceeds the repository's size limit for a committed file)."""
import glob
import os

import numpy as np
import torch

from tests import image_backbone2d3d_ref as R

BWD_CASES = ("b", "c")
PART_BYTES = 900 * 1024


def cotangents(case, shapes, device="cpu"):
    """one float32 unit-normal cotangent per output, drawn in output order from a generator seeded seed + 2000"""
    g = torch.Generator(device=device)
    g.manual_seed(case["seed"] + 2000)
    return [torch.randn(tuple(s), generator=g, device=device, dtype=torch.float32) for s in shapes]


def grad_names(module):
    """the gradient tensors of a case, in the fixture's order: every parameter, then the two inputs"""
    return [n for n, _ in module.named_parameters()] + ["x", "dino_feat"]


def run_backward(module, x, dino, case):
    """loss = sum_i <out_i, cot_i>; backward; -> (outputs, {name: gradient}) in the module's dtype"""
    dt = next(module.parameters()).dtype
    x = x.detach().to(dt).requires_grad_(True)
    dino = dino.detach().to(dt).requires_grad_(True)
    module.zero_grad(set_to_none=True)
    outs = module(x, dino)
    cots = cotangents(case, [o.shape for o in outs], device="cpu")
    loss = sum((o * c.to(device=o.device, dtype=dt)).sum() for o, c in zip(outs, cots))
    loss.backward()
    grads = {n: p.grad.detach() for n, p in module.named_parameters()}
    grads["x"], grads["dino_feat"] = x.grad.detach(), dino.grad.detach()
    return outs, grads


def load(golden_dir):
    """the fixture as one dict: '<case>/<name>' -> float64 gradient, '<case>_dev32' [n], '<case>_floor' [1], '<case>_names'"""
    res = {}
    paths = [os.path.join(golden_dir, "image_backbone2d3d_bwd.npz")] + sorted(glob.glob(os.path.join(golden_dir, "image_backbone2d3d_bwd_[0-9]*.npz")))
    for p in paths:
        with np.load(p) as z:
            for k in z.files:
                assert k not in res, k
                res[k] = z[k]
    return res
