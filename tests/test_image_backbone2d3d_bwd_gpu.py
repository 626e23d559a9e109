"""The 2D-3D image backbone's backward on the device (csrc/conv2d.hip, csrc/conv_index.h, csrc/resize_index.h;
diffreg_hip/image_backbone2d3d.py).  Needs a GPU.

Bars.  Error measure everywhere: per tensor, max|a - ref64| / max|ref64| (image_backbone2d3d_ref.rel_dev).
 * conv gradients: against autograd through torch.nn.functional.conv2d in float64 on the device; grad_x, grad_w and grad_bias each at most 4 x
   the deviation of torch's own float32 gradient from the float64 one (held_torch, no floor).  Two runs bit-equal; outputs prefilled with NaN are
   written everywhere; NULL grad_w / grad_bias; padded leading dimensions and base pointers 4 bytes off a 16-byte boundary bit-equal to the
   contiguous call with the guard cells untouched; out-of-domain arguments return their code without a launch.
 * resize_rows_backward: against autograd of F.interpolate in float64 under held_torch, bit-equal to dr_resize_tokens_backward_f32 transposed.
 * whole backbone, fixture cases b and c: every gradient tensor within 4 x max(its recorded dev32, the case's recorded floor = the median dev32)
   of the reference's float64 gradient.  The floor is the median because a whole-network gradient passes through about fifty kernels and a
   tensor where the reference's float32 run happened to be lucky is no standard; the rule was fixed before any device number existed.
 * real widths: against the restatement's .double() autograd on the device, 4 x max(torch's float32 deviation, the median of those) per tensor."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import image_backbone2d3d_bwd_ref as B
from tests import image_backbone2d3d_ref as R
from tests.conftest import ROOT
from tests.test_image_backbone2d3d_bwd_oracle import EXTRA_CONV_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL_CONV = dict(R.CONV_CASES, **EXTRA_CONV_CASES)


def held_torch(what, dev, t32, t64):
    e, d = R.rel_dev(dev, t64), R.rel_dev(t32, t64)
    print("%s: device %.3e from float64, torch float32 %.3e (bar %.3e)" % (what, e, d, 4 * d))
    assert e <= 4 * d, (what, e, d, 4 * d)


def rows(t):
    """[1, C, H, W] -> [H W, C]"""
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).contiguous()


def nchw(r, size):
    return r.view(size[0], size[1], r.shape[1]).permute(2, 0, 1).contiguous()[None]


_CONV_CACHE = {}


def conv_case(name):
    """inputs and torch's float32 / float64 gradients of one geometry, computed once and shared"""
    if name not in _CONV_CACHE:
        k, s, p, d, cin, cout, H, W = ALL_CONV[name]
        g = torch.Generator(device=DEV)
        g.manual_seed(300 + sorted(ALL_CONV).index(name))
        x = torch.randn(1, cin, H, W, generator=g, device=DEV)
        w = torch.randn(cout, cin, k, k, generator=g, device=DEV) * (1.0 / (cin * k * k)) ** 0.5
        b = torch.randn(cout, generator=g, device=DEV) * 0.1
        Ho, Wo = (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1
        go = torch.randn(1, cout, Ho, Wo, generator=g, device=DEV)
        grads = {}
        for dt in (torch.float32, torch.float64):
            xx, ww, bb = (t.detach().to(dt).clone().requires_grad_(True) for t in (x, w, b))
            (TF.conv2d(xx, ww, bb, stride=s, padding=p, dilation=d) * go.to(dt)).sum().backward()
            grads[dt] = (xx.grad, ww.grad, bb.grad)
        _CONV_CACHE[name] = ((k, s, p, d), x, w, go, grads)
    return _CONV_CACHE[name]


def device_grads(name, need_weight=True, need_bias=True):
    from diffreg_hip import lib
    (k, s, p, d), x, w, go, _ = conv_case(name)
    size = tuple(x.shape[2:])
    gx = torch.full((size[0] * size[1], x.shape[1]), float("nan"), device=DEV)
    lib.conv2d_rows_backward_data(rows(go), size, lib.pack_conv_weight_t(w), k, s, p, d, out=gx)
    gw, gb = lib.conv2d_rows_backward_weight(rows(x), size, rows(go), k, s, p, d, need_weight=need_weight, need_bias=need_bias)
    return gx, gw, gb


# ---- the conv gradients ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ALL_CONV))
def test_conv_gradients_against_torch(name):
    (k, s, p, d), x, w, go, grads = conv_case(name)
    size = tuple(x.shape[2:])
    gx, gw, gb = device_grads(name)
    assert not torch.isnan(gx).any() and not torch.isnan(gw).any() and not torch.isnan(gb).any()       # every element written
    (x32, w32, b32), (x64, w64, b64) = grads[torch.float32], grads[torch.float64]
    held_torch("conv %s grad_x" % name, nchw(gx, size), x32, x64)
    held_torch("conv %s grad_w" % name, gw, w32, w64)
    held_torch("conv %s grad_bias" % name, gb, b32, b64)
    if name == "uncovered":                                           # the last input row is reached by no tap: exactly zero, and written
        assert bool((x64[0, :, -1, :] == 0).all()) and bool((nchw(gx, size)[0, :, -1, :] == 0).all())
    gx2, gw2, gb2 = device_grads(name)
    assert torch.equal(gx, gx2) and torch.equal(gw, gw2) and torch.equal(gb, gb2), "two runs differ"


@pytest.mark.parametrize("name", ["stride2", "stem_c3", "slabs"])
def test_conv_weight_gradient_accepts_null_outputs(name):
    gx, gw, gb = device_grads(name)
    _, gw1, gb1 = device_grads(name, need_bias=False)
    _, gw2, gb2 = device_grads(name, need_weight=False)
    assert gb1 is None and gw2 is None and torch.equal(gw1, gw) and torch.equal(gb2, gb)


@pytest.mark.parametrize("name", ["stride2", "stem_c3", "ragged", "cout_10", "slabs"])
def test_conv_gradients_with_leading_dimensions_and_unaligned_pointers(name):
    """every leading dimension padded and every base pointer 4 bytes off a 16-byte boundary (the scalar-load arms): bit-equal to the contiguous
    call, the cells around the views untouched"""
    from diffreg_hip import lib
    (k, s, p, d), x, w, go, _ = conv_case(name)
    size, cin, cout = tuple(x.shape[2:]), x.shape[1], w.shape[0]
    gx, gw, gb = device_grads(name)
    r = lib.raw()
    n_in, n_out = size[0] * size[1], go.shape[2] * go.shape[3]

    def view(n, c, pad, fill):
        buf = torch.full((n * (c + pad) + 1,), fill, device=DEV)
        return buf, buf[1:].view(n, c + pad)[:, :c]
    xb, xv = view(n_in, cin, 3, 7.0)
    xv.copy_(rows(x))
    gb_, gv = view(n_out, cout, 5, 7.0)
    gv.copy_(rows(go))
    ob, ov = view(n_in, cin, 2, -3.0)
    wtb = torch.zeros(cin * k * k * cout + 1, device=DEV)
    wt = wtb[1:].view(cin, k * k * cout)
    wt.copy_(lib.pack_conv_weight_t(w))
    assert xv.data_ptr() % 16 == 4 and gv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4 and wt.data_ptr() % 16 == 4
    assert r.dr_conv2d_rows_backward_data_f32(size[0], size[1], cin, cout, k, s, p, d, gv.data_ptr(), cout + 5, wt.data_ptr(), None, 0, ov.data_ptr(),
                                              cin + 2, None) == 0
    assert torch.equal(ov.contiguous(), gx), "the strided, unaligned data gradient differs from the contiguous one"
    assert float(ob[0]) == -3.0 and bool((ob[1:].view(n_in, cin + 2)[:, cin:] == -3.0).all())
    gwb, gbb = torch.full((cout * k * k * cin + 2,), -3.0, device=DEV), torch.full((cout + 2,), -3.0, device=DEV)
    wsb = r.dr_conv2d_rows_backward_weight_workspace_bytes(size[0], size[1], cin, cout, k, s, p, d)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    assert r.dr_conv2d_rows_backward_weight_f32(size[0], size[1], cin, cout, k, s, p, d, xv.data_ptr(), cin + 3, gv.data_ptr(), cout + 5,
                                                gwb.data_ptr() + 4, gbb.data_ptr() + 4, ws.data_ptr(), wsb, None) == 0
    got_w = gwb[1:-1].view(cout, k, k, cin).permute(0, 3, 1, 2)
    assert torch.equal(got_w, gw) and torch.equal(gbb[1:-1], gb), "the strided, unaligned weight gradient differs from the contiguous one"
    assert float(gwb[0]) == -3.0 == float(gwb[-1]) and float(gbb[0]) == -3.0 == float(gbb[-1])
    assert bool((xb[1:].view(n_in, cin + 3)[:, cin:] == 7.0).all()) and bool((gb_[1:].view(n_out, cout + 5)[:, cout:] == 7.0).all())


def test_data_gradient_addend():
    from diffreg_hip import lib
    (k, s, p, d), x, w, go, _ = conv_case("stride2")
    size = tuple(x.shape[2:])
    gx, _, _ = device_grads("stride2")
    add = torch.randn_like(gx)
    got = lib.conv2d_rows_backward_data(rows(go), size, lib.pack_conv_weight_t(w), k, s, p, d, addend=add)
    assert torch.equal(got, gx + add)


def test_out_of_domain_returns_its_code_without_a_launch():
    from diffreg_hip import lib
    r = lib.raw()
    g, wt, o = torch.zeros(25, 4, device=DEV), torch.zeros(4, 36, device=DEV), torch.full((25, 4), 5.0, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    dg = lambda *geom, gp=g.data_ptr(), ldg=4: r.dr_conv2d_rows_backward_data_f32(*geom, gp, ldg, wt.data_ptr(), None, 0, o.data_ptr(), 4, None)
    assert dg(5, 5, 4, 4, 3, 1, 0, 3) == -1 and dg(5, 5, 4, 4, 3, 0, 1, 1) == -1 and dg(5, 5, 4, 4, 3, 1, 1, 1, ldg=3) == -1
    assert dg(5, 5, 4, 4, 3, 1, 1, 1, gp=g.data_ptr() + 2) == -1 and dg(5, 5, 4, 4, 32, 1, 16, 1) == -3
    wg = lambda *geom, ldx=4, wsb=1 << 16: r.dr_conv2d_rows_backward_weight_f32(*geom, g.data_ptr(), ldx, g.data_ptr(), 4, o.data_ptr(), o.data_ptr(),
                                                                                ws.data_ptr(), wsb, None)
    assert wg(5, 5, 4, 4, 3, 1, 0, 3) == -1 and wg(5, 5, 4, 4, 3, 1, 1, 1, ldx=3) == -1 and wg(5, 5, 4, 4, 3, 1, 1, 1, wsb=64) == -1
    assert wg(5, 5, 4, 4, 32, 1, 16, 1) == -3
    assert r.dr_resize_rows_backward_f32(4, 0, 5, 5, 5, g.data_ptr(), 4, o.data_ptr(), 4, None) == -1
    assert r.dr_resize_rows_backward_f32(4, 5, 5, 5, 5, g.data_ptr(), 3, o.data_ptr(), 4, None) == -1
    torch.cuda.synchronize()
    assert bool((o == 5.0).all())                                    # nothing was launched


# ---- resize_rows_backward --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.RESIZE_CASES) + ["down_21x27"])
def test_resize_rows_backward_against_torch_and_resize_tokens_backward(name):
    from diffreg_hip import lib
    src, dst = dict(R.RESIZE_CASES, down_21x27=((21, 27), (6, 7)))[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(9)
    C = 37
    x = torch.randn(1, C, *src, generator=g, device=DEV)
    go = torch.randn(1, C, *dst, generator=g, device=DEV)
    ref = {}
    for dt in (torch.float32, torch.float64):
        xx = x.detach().to(dt).clone().requires_grad_(True)
        (TF.interpolate(xx, size=dst, mode="bilinear", align_corners=True) * go.to(dt)).sum().backward()
        ref[dt] = xx.grad
    got = torch.full((src[0] * src[1], C), float("nan"), device=DEV)
    lib.resize_rows_backward(rows(go), src, dst, out=got)
    assert not torch.isnan(got).any()
    held_torch("resize_rows_backward %s" % name, nchw(got, src), ref[torch.float32], ref[torch.float64])
    tok = lib.resize_tokens_backward(rows(go), (C,) + tuple(src), dst)                 # [C, Hs, Ws]
    assert torch.equal(got, tok.reshape(C, -1).t().contiguous()), "differs from dr_resize_tokens_backward_f32 transposed"
    assert torch.equal(got, lib.resize_rows_backward(rows(go), src, dst))


# ---- the whole backbone ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return B.load(os.path.join(ROOT, "tests", "golden"))


@pytest.mark.parametrize("name", B.BWD_CASES)
def test_backbone_gradients_against_the_reference(name, fixture):
    from diffreg_hip.image_backbone2d3d import bind
    case = R.CASES[name]
    m = R.build(case, device=DEV)
    x, dino = (t.to(DEV) for t in R.make_inputs(case))
    dev = bind(m, grad=True)
    with torch.no_grad():
        plain = dev.forward(x, dino)
    outs, grads = B.run_backward(m, x, dino, case)
    for a, b in zip(outs, plain):
        assert a.requires_grad and torch.equal(a.detach(), b), "the grad-recording arm's forward differs from the no_grad arm's"
    names, floor = [str(n) for n in fixture[name + "_names"]], float(fixture[name + "_floor"][0])
    failed = []
    for n, d in zip(names, fixture[name + "_dev32"]):
        ref = fixture["%s/%s" % (name, n)]
        assert tuple(grads[n].shape) == ref.shape, n
        e, bar = R.rel_dev(grads[n].cpu(), ref), 4 * max(float(d), floor)
        print("backbone %s %s: device %.3e from the reference's float64, the reference's float32 %.3e (bar %.3e)" % (name, n, e, float(d), bar))
        if not e <= bar:
            failed.append((n, e, float(d), bar))
    assert not failed, failed


def test_backbone_gradients_real_widths():
    from diffreg_hip.image_backbone2d3d import bind
    case = R.REAL
    m = R.ImageBackbone(1, case["out"], case["base"]).to(DEV).eval()
    m.load_state_dict(R.make_weights(m, case["seed"], device=DEV))
    x, dino = R.make_inputs(case, device=DEV)
    _, g32 = B.run_backward(m, x, dino, case)
    g32 = {k: v.clone() for k, v in g32.items()}
    _, g64 = B.run_backward(m.double(), x, dino, case)
    g64 = {k: v.clone() for k, v in g64.items()}
    m.float()
    bind(m, grad=True)
    _, gd = B.run_backward(m, x, dino, case)
    names = B.grad_names(m)
    devs = {n: R.rel_dev(g32[n], g64[n]) for n in names}
    med = float(np.median(list(devs.values())))
    failed = []
    for n in names:
        e, bar = R.rel_dev(gd[n], g64[n]), 4 * max(devs[n], med)
        print("real widths %s %s: device %.3e from float64, torch float32 %.3e (bar %.3e)" % (n, tuple(g64[n].shape), e, devs[n], bar))
        if not e <= bar:
            failed.append((n, e, devs[n], bar))
    assert not failed, failed


def test_accelerate_with_gradients_trains_on_the_device():
    from diffreg_hip.overlay2d3d import accelerate
    case = R.CASES["b"]
    ib = R.build(case, device=DEV)
    stub = torch.nn.Module()
    stub.img_backbone = ib
    stub.denoising_transformer, stub.denoising_coarse_matching = torch.nn.Identity(), torch.nn.Identity()
    stub.get_warped_from_noising_matching3D3D = types.MethodType(lambda self, *a: None, stub)
    x, dino = R.make_inputs(case, device=DEV)
    calls = [0]                                                       # the module's own forward runs its sub-modules; the device path never does
    ib.encoder1.register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
    ov = accelerate(stub, image_backbone_grad=True)
    assert "forward" in ib.__dict__ and ov.image_backbone and ov.image_backbone_grad
    ib.train()
    with torch.enable_grad():
        outs = ib(x, dino)
        sum(o.sum() for o in outs).backward()
    assert calls[0] == 0, "the bound forward ran the module's own code"
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in ib.parameters())
    with torch.no_grad():                                             # an in-place SGD step: the packed weights must be rebuilt
        for p in ib.parameters():
            p.add_(p.grad, alpha=-1e-3)
    with torch.enable_grad():
        got = ib(x, dino)
    assert calls[0] == 0
    ov.remove()
    assert "forward" not in ib.__dict__ and "_dr_overlay" not in stub.__dict__
    with torch.no_grad():
        own = ib(x, dino)
    assert calls[0] == 1
    for a, b in zip(got, own):
        e = R.rel_dev(a.detach(), b)
        print("after the update: device forward %.3e from the module's own forward on the new weights" % e)
        assert tuple(a.shape) == tuple(b.shape) and e < 1e-5
    ib.eval()
    ib.decoder1_2[0].act = torch.nn.ReLU()                            # refused when binding, never at call time
    with pytest.raises(NotImplementedError):
        accelerate(stub, image_backbone_grad=True)
