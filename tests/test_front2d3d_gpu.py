"""The geometry head and the feature-layout glue of MATR2D3D.forward on the device (csrc/front2d3d.hip; diffreg_hip/front2d3d.py).  Needs a GPU.

Bars.  Error measure everywhere: max over the elements of |a - ref64| / max(1, |ref64|) (front2d3d_ref.rel_dev).
 * back_project (both modes), render: against the reference's own float64 outputs (tests/golden/front2d3d.npz); the device may be off by at most
   max(1e-9, 4 x the deviation of the reference's own float32 run on the same case); masks equal everywhere (the fixture keeps every z 1e-3 away
   from 0 and from the limit: tests/test_front2d3d_oracle.py).
 * create_meshgrid: bit-equal to its definition (cartesian_prod of arange / linspace).  The reference's calls .cuda() and has no golden.
 * resize_tokens, rows_normalized: against torch.nn.functional in float64 on the device; at most 4 x the deviation of torch's own float32 run from
   that float64 run -- no floor: where torch's float32 is exact (identity resample, 1 x 1 target, C = 1) the device is exact too.  For the
   normalise backward the all-zero row (gradient g / 1e-12) is measured apart from the other rows, so that it cannot hide them.
 * two runs bit-equal; the sparse backward equals the dense backward fed the scattered gradient to one float32 ulp per element (both round a
   double once; their double sums differ in order only)."""
import itertools
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import front2d3d_ref as F
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = np.load(os.path.join(ROOT, "tests", "golden", "front2d3d.npz"))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def held(what, dev, r32, r64, floor=1e-9):
    e, d = F.rel_dev(dev, r64), F.rel_dev(r32, r64)
    allowed = max(floor, 4 * d)
    print("%s: device %.3e from float64, reference float32 %.3e (bar %.3e)" % (what, e, d, allowed))
    assert e <= allowed, (what, e, d, allowed)


def held_torch(what, dev, t32, t64):
    """the layout bar: 4 x torch's own float32 deviation, no floor"""
    held(what, dev.double().cpu().numpy(), t32.double().cpu().numpy(), t64.cpu().numpy(), floor=0.0)


# ---- back_project ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(F.BACK_PROJECT_CASES))
def test_back_project_against_the_reference(name):
    from diffreg_hip import front2d3d as fr, lib
    kw = F.BACK_PROJECT_CASES[name]
    depth, K = t(G[name + "_in_depth"]), t(G[name + "_in_intrinsics"])
    a, b = float(G[name + "_in_a"]), float(G[name + "_in_b"])
    if kw["mode"] == 0:
        pts, mask = fr.back_project(depth, K, scaling_factor=a, depth_limit=F.DEPTH_LIMIT, transposed=True, return_mask=True)
    else:                                                           # the model's factors are device tensors
        pts, mask = fr.back_project_depth(depth, K, scaling_factor_a=torch.tensor(a, device=DEV), scaling_factor_b=torch.tensor([b], device=DEV),
                                          depth_limit=F.DEPTH_LIMIT, transposed=True, return_mask=True)
    H, W = kw["H"], kw["W"]
    assert tuple(pts.shape) == (1, H, W, 3) and pts.dtype == torch.float32 and tuple(mask.shape) == (1, H, W) and mask.dtype == torch.bool
    assert np.array_equal(mask.reshape(-1).cpu().numpy(), G[name + "_mask64"])
    held(name, pts.reshape(-1, 3).cpu().numpy(), G[name + "_points32"], G[name + "_points64"])
    # the other return forms are views of the same numbers
    chw = fr.back_project(depth, K, a, F.DEPTH_LIMIT) if kw["mode"] == 0 else fr.back_project_depth(depth, K, a, b, F.DEPTH_LIMIT)
    assert tuple(chw.shape) == (1, 3, H, W) and torch.equal(chw.permute(0, 2, 3, 1), pts)
    # numbers on the host instead of device tensors; the pixel output is create_meshgrid(H, W).float(); no limit keeps the far depths
    p2, m2, pix = lib.back_project_points(depth[0], K[0], mode=kw["mode"], a=a, b=b, depth_limit=F.DEPTH_LIMIT, pixels=True)
    assert torch.equal(p2, pts.reshape(-1, 3)) and torch.equal(m2.bool(), mask.reshape(-1))
    assert torch.equal(pix, torch.cartesian_prod(torch.arange(H), torch.arange(W)).float().to(DEV))
    ref, rm = F.back_project(G[name + "_in_depth"][0], G[name + "_in_intrinsics"][0], kw["mode"], a, b, None, np.float64)
    p3, m3, _ = lib.back_project_points(depth[0], K[0], mode=kw["mode"], a=a, b=b)
    assert np.array_equal(m3.bool().cpu().numpy(), rm) and F.rel_dev(p3.cpu().numpy(), ref) <= 1e-6


def test_back_project_unaligned_and_batched_forms():
    """a depth image at an address that is no multiple of 16 takes the scalar kernel; B = 2 takes the module's torch statement: same numbers"""
    from diffreg_hip import front2d3d as fr
    name = "bp0_33x65"
    depth, K = t(G[name + "_in_depth"]), t(G[name + "_in_intrinsics"])
    want = fr.back_project(depth, K, depth_limit=F.DEPTH_LIMIT, transposed=True)
    buf = torch.zeros(depth.numel() + 1, device=DEV)
    buf[1:] = depth.reshape(-1)
    off = buf[1:].view(1, 33, 65)
    assert off.data_ptr() % 16 == 4
    assert torch.equal(fr.back_project(off, K, depth_limit=F.DEPTH_LIMIT, transposed=True), want)
    both, masks = fr.back_project(torch.cat([depth, depth]), torch.cat([K, K]), depth_limit=F.DEPTH_LIMIT, transposed=True, return_mask=True)
    assert tuple(both.shape) == (2, 33, 65, 3) and masks.dtype == torch.bool
    assert F.rel_dev(both[1].cpu().numpy(), want[0].cpu().numpy()) <= 1e-6


# ---- render ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(F.RENDER_CASES))
def test_render_against_the_reference(name):
    from diffreg_hip import front2d3d as fr
    pts, K = t(G[name + "_in_points"]), t(G[name + "_in_intrinsics"])
    T = t(G[name + "_in_extrinsics"]) if name + "_in_extrinsics" in G.files else None
    pix, z = fr.render(pts, K, extrinsics=T, rounding=False, return_depth=True)
    assert tuple(pix.shape) == (pts.shape[0], 2) and pix.dtype == torch.float32 and tuple(z.shape) == (pts.shape[0],)
    held(name + " pixels", pix.cpu().numpy(), G[name + "_pixels32"], G[name + "_pixels64"])
    held(name + " depth", z.cpu().numpy(), G[name + "_depth32"], G[name + "_depth64"])
    assert torch.equal(fr.render(pts, K, extrinsics=T, rounding=False), pix)
    # a batch dimension of 1 is the same call; rounding=True is the module's torch statement of the same definition
    b = fr.render(pts[None], K[None], extrinsics=None if T is None else T[None], rounding=False)
    assert tuple(b.shape) == (1, pts.shape[0], 2) and torch.equal(b[0], pix)
    r = fr.render(pts, K, extrinsics=T)
    assert r.dtype == torch.int64 and tuple(r.shape) == tuple(pix.shape)


# ---- create_meshgrid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", F.MESHGRID_SIZES)
@pytest.mark.parametrize("normalized,flatten", list(itertools.product((False, True), (False, True))))
def test_create_meshgrid_is_its_definition(hw, normalized, flatten):
    from diffreg_hip import front2d3d as fr
    h, w = hw
    got = fr.create_meshgrid(h, w, normalized=normalized, flatten=flatten)
    if normalized:
        want = torch.cartesian_prod(torch.linspace(0.0, 1.0, steps=h), torch.linspace(0.0, 1.0, steps=w))
    else:
        want = torch.cartesian_prod(torch.arange(h), torch.arange(w))
        assert np.array_equal(want.view(h, w, 2).numpy(), F.create_meshgrid(h, w))
    want = want if flatten else want.view(h, w, 2)
    assert got.is_cuda and got.dtype == (torch.float32 if normalized else torch.int64) and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want)


# ---- resize_tokens -----------------------------------------------------------------------------------------------------------------------------
RESIZE_CASES = [(3, 4, 6, 3, 5), (130, 7, 9, 34, 45), (5, 6, 6, 6, 6), (2, 5, 4, 1, 1)]


@pytest.mark.parametrize("C,Hs,Ws,Hd,Wd", RESIZE_CASES)
def test_resize_tokens_against_interpolate(C, Hs, Ws, Hd, Wd):
    from diffreg_hip import front2d3d as fr
    gen = torch.Generator().manual_seed(C * 1000 + Hd)
    x = torch.randn(1, C, Hs, Ws, generator=gen).to(DEV)
    g = torch.randn(Hd * Wd, C, generator=gen).to(DEV)

    def torch_side(dt):
        xi = x.to(dt).clone().requires_grad_(True)
        y = TF.interpolate(xi, size=(Hd, Wd), mode="bilinear", align_corners=True).squeeze(0).view(-1, Hd * Wd).transpose(0, 1)
        y.backward(g.to(dt))
        return y.detach(), xi.grad

    y64, gx64 = torch_side(torch.float64)
    y32, gx32 = torch_side(torch.float32)
    runs = []
    for _ in range(2):
        xd = x.clone().requires_grad_(True)
        y = fr.resize_tokens(xd, (Hd, Wd))
        y.backward(g)
        runs.append((y.detach(), xd.grad))
    y, gx = runs[0]
    assert tuple(y.shape) == (Hd * Wd, C) and y.is_contiguous() and tuple(gx.shape) == (1, C, Hs, Ws)
    held_torch("resize forward", y, y32, y64)
    held_torch("resize backward", gx, gx32, gx64)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])       # bit-equal twice over


# ---- rows_normalized ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,P", list(itertools.product((1, 128, 130, 256), (1, 63, 65, 4097))))
def test_rows_normalized_against_normalize(C, P):
    from diffreg_hip import front2d3d as fr, lib
    gen = torch.Generator().manual_seed(C * 10000 + P)
    x = torch.randn(C, P, generator=gen)
    zero = P // 2
    x[:, zero] = 0.0                                                     # one all-zero row: the eps clamp
    x = x.to(DEV)
    g = (torch.randint(-128, 129, (P, C), generator=gen).float() / 64).to(DEV)
    K = min(2 * P + 3, 50)
    rows = torch.randint(0, P, (K,), generator=gen)
    rows[0], rows[K - 1] = zero, rows[1]                                 # the zero row is touched; at least one repeat
    rows = rows.to(DEV)
    gk = (torch.randint(-128, 129, (K, C), generator=gen).float() / 64).to(DEV)

    def torch_side(dt):
        xi = x.to(dt).clone().requires_grad_(True)
        y = TF.normalize(xi.view(C, -1).transpose(0, 1).contiguous(), p=2, dim=1)
        (gd,) = torch.autograd.grad((y * g.to(dt)).sum(), xi, retain_graph=True)
        (gs,) = torch.autograd.grad((y[rows] * gk.to(dt)).sum(), xi)
        return y.detach(), gd, gs

    y64, gd64, gs64 = torch_side(torch.float64)
    y32, gd32, gs32 = torch_side(torch.float32)
    xd = x.view(1, C, 1, P).clone().requires_grad_(True)                 # (1, C, H, W)
    y = fr.rows_normalized(xd)
    (gd,) = torch.autograd.grad((y * g).sum(), xd)
    full, picked = fr.rows_normalized(xd, rows=rows)
    (gs,) = torch.autograd.grad((picked * gk).sum(), xd)
    assert tuple(y.shape) == (P, C) and y.is_contiguous() and tuple(gd.shape) == tuple(xd.shape) == tuple(gs.shape)
    assert torch.equal(full, y.detach()) and not full.requires_grad and torch.equal(picked.detach(), y.detach()[rows])
    assert torch.equal(y[zero], torch.zeros(C, device=DEV))
    gd, gs = gd.view(C, P), gs.view(C, P)
    held_torch("normalize forward", y.detach(), y32, y64)
    rest = torch.arange(P, device=DEV) != zero
    for what, dev, r32, r64 in (("dense", gd, gd32, gd64), ("sparse", gs, gs32, gs64)):
        held_torch("normalize %s backward, zero row" % what, dev[:, zero], r32[:, zero], r64[:, zero])
        held_torch("normalize %s backward, other rows" % what, dev[:, rest], r32[:, rest], r64[:, rest])
    # sparse == dense fed the scattered gradient (sums of multiples of 1 / 64 are exact in float32), to one ulp per element
    scattered = torch.zeros(P, C, device=DEV).index_add_(0, rows, gk)
    dense = lib.rows_normalize_chw_backward(x, scattered).cpu().numpy()
    sparse = lib.rows_normalize_chw_backward(x, gk, rows=rows)
    assert torch.equal(sparse, gs)
    assert np.all(np.abs(sparse.cpu().numpy() - dense) <= np.spacing(np.abs(dense)))
    untouched = torch.ones(P, dtype=torch.bool, device=DEV)
    untouched[rows] = False
    assert not sparse[:, untouched].any()
    assert torch.equal(lib.rows_normalize_chw_backward(x, gk, rows=rows), sparse) and torch.equal(lib.rows_normalize_chw(x), y.detach())


def test_rows_normalized_refuses_what_it_cannot_do():
    from diffreg_hip import front2d3d as fr, lib
    with pytest.raises(RuntimeError, match="not supported"):
        fr.rows_normalized(torch.zeros(1, 257, 2, 3, device=DEV))
    with pytest.raises(ValueError):
        fr.rows_normalized(torch.zeros(2, 4, 2, 3, device=DEV))
    with pytest.raises(RuntimeError):
        lib.rows_normalize_chw(torch.zeros(4, 6))                        # no CPU path
    # a row outside [0, P) is skipped -- the others are written -- and reported, not dropped silently
    x = torch.randn(4, 6, device=DEV)
    lib.device_status()
    out = lib.rows_normalize_chw_backward(x, torch.ones(2, 4, device=DEV), rows=torch.tensor([6, 2]))
    with pytest.raises(RuntimeError, match="invalid argument"):
        lib.device_status()
    assert out[:, 2].abs().sum() > 0 and not out[:, [0, 1, 3, 4, 5]].any()
    lib.device_status()                                                  # consumed


# ---- overlay -----------------------------------------------------------------------------------------------------------------------------------
def _stub_model():
    mod = types.ModuleType("front2d3d_stub_model")
    sys.modules[mod.__name__] = mod
    mod.back_project, mod.render, mod.create_meshgrid = (lambda *a, **k: "bp"), (lambda *a, **k: "rd"), (lambda *a, **k: "mg")

    class Sub:
        def forward(self, *a, **k):
            return None

    class Model:
        training = False

        def __init__(self):
            self.denoising_transformer, self.denoising_coarse_matching = Sub(), Sub()

        def get_warped_from_noising_matching3D3D(self, *a):
            return None

        def back_project_depth(self, *a, **k):
            return "bpd"

    Model.__module__ = mod.__name__
    return mod, Model()


def test_overlay_front_flag_binds_and_restores():
    from diffreg_hip import front2d3d as fr
    from diffreg_hip.overlay2d3d import accelerate
    mod, model = _stub_model()
    try:
        orig = {k: getattr(mod, k) for k in ("back_project", "render", "create_meshgrid")}
        ov = accelerate(model)                                           # without the flag nothing of the four is touched
        assert all(getattr(mod, k) is v for k, v in orig.items()) and "back_project_depth" not in model.__dict__
        ov.remove()
        ov = accelerate(model, front=True)
        assert mod.back_project is fr.back_project and mod.render is fr.render and mod.create_meshgrid is fr.create_meshgrid
        assert model.back_project_depth is fr.back_project_depth
        ov.remove()
        assert all(getattr(mod, k) is v for k, v in orig.items())
        assert "back_project_depth" not in model.__dict__ and model.back_project_depth() == "bpd"
    finally:
        sys.modules.pop(mod.__name__, None)
