"""The 2D-3D image backbone's inference forward on the device (csrc/conv2d.hip, csrc/conv_index.h; diffreg_hip/image_backbone2d3d.py).  Needs a GPU.

Bars.  Error measure everywhere: per tensor, max|a - ref64| / max|ref64| (image_backbone2d3d_ref.rel_dev).
 * conv primitive: against torch.nn.functional.conv2d in float64 on the device; at most 4 x the deviation of torch's own float32 run from that
   float64 run (the rule of test_front2d3d_gpu.py::held_torch, no floor).  Without bias, with addend, with padded leading dimensions and a base
   pointer offset by 4 bytes (the scalar-load arm); two runs bit-equal; out-of-domain arguments return their code without a launch.
 * resize_rows: against F.interpolate(bilinear, align_corners=True) in float64 under the same rule, with and without addend, and bit-equal to
   dr_resize_tokens_f32 on the same numbers.
 * whole backbone, fixture cases a / b / c: each of the four outputs within max(floor, 4 x the reference's recorded float32 deviation) of the
   reference's float64 output (tests/golden/image_backbone2d3d.npz; floor = the smallest recorded deviation, written by the minting run).
 * real widths (128 base channels, 48 x 64 image): against the restatement run as .double() on the device, 4 x torch's float32 deviation per output."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import image_backbone2d3d_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = np.load(os.path.join(ROOT, "tests", "golden", "image_backbone2d3d.npz"))


def held_torch(what, dev, t32, t64):
    e, d = R.rel_dev(dev, t64), R.rel_dev(t32, t64)
    print("%s: device %.3e from float64, torch float32 %.3e (bar %.3e)" % (what, e, d, 4 * d))
    assert e <= 4 * d, (what, e, d, 4 * d)


def rows(t):
    """[1, C, H, W] -> [H W, C]"""
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).contiguous()


def nchw(r, size):
    return r.view(size[0], size[1], r.shape[1]).permute(2, 0, 1).contiguous()[None]


def conv_case(name, seed=0):
    k, s, p, d, cin, cout, H, W = R.CONV_CASES[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(100 + seed)
    x = torch.randn(1, cin, H, W, generator=g, device=DEV)
    w = torch.randn(cout, cin, k, k, generator=g, device=DEV) * (1.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=g, device=DEV) * 0.1
    return (k, s, p, d), x, w, b


# ---- the conv primitive --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CONV_CASES))
def test_conv_against_torch(name):
    from diffreg_hip import lib
    (k, s, p, d), x, w, b = conv_case(name)
    t64 = TF.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p, dilation=d)
    t32 = TF.conv2d(x, w, b, stride=s, padding=p, dilation=d)
    out, size = lib.conv2d_rows(rows(x), x.shape[2:], lib.pack_conv_weight(w), k, b, s, p, d)
    assert size == tuple(t64.shape[2:])
    held_torch("conv " + name, nchw(out, size), t32, t64)
    again, _ = lib.conv2d_rows(rows(x), x.shape[2:], lib.pack_conv_weight(w), k, b, s, p, d)
    assert torch.equal(out, again)


@pytest.mark.parametrize("name", ["stride2", "stem_c3", "ragged"])
def test_conv_without_bias_with_addend_and_leading_dimensions(name):
    from diffreg_hip import lib
    (k, s, p, d), x, w, b = conv_case(name, seed=1)
    cin, cout = x.shape[1], w.shape[0]
    wp = lib.pack_conv_weight(w)
    # no bias
    t64, t32 = (TF.conv2d(x.to(dt), w.to(dt), None, stride=s, padding=p, dilation=d) for dt in (torch.float64, torch.float32))
    out, size = lib.conv2d_rows(rows(x), x.shape[2:], wp, k, None, s, p, d)
    held_torch("conv %s, no bias" % name, nchw(out, size), t32, t64)
    # addend
    add = torch.randn(size[0] * size[1], cout, device=DEV)
    t64 = TF.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p, dilation=d) + nchw(add, size).double()
    t32 = TF.conv2d(x, w, b, stride=s, padding=p, dilation=d) + nchw(add, size)
    out, _ = lib.conv2d_rows(rows(x), x.shape[2:], wp, k, b, s, p, d, addend=add)
    held_torch("conv %s, addend" % name, nchw(out, size), t32, t64)
    # ldx, lda, ldo > C and every base pointer 4 bytes off a 16-byte boundary: views into larger buffers (the scalar-load arm; the cells around
    # the views must stay untouched)
    n_in, n_out = x.shape[2] * x.shape[3], size[0] * size[1]
    xb = torch.full((n_in * (cin + 3) + 1,), 7.0, device=DEV)
    xv = xb[1:].view(n_in, cin + 3)[:, :cin]
    xv.copy_(rows(x))
    ab = torch.zeros(n_out * (cout + 5) + 1, device=DEV)
    av = ab[1:].view(n_out, cout + 5)[:, :cout]
    av.copy_(add)
    ob = torch.full((n_out * (cout + 2) + 1,), -3.0, device=DEV)
    ov = ob[1:].view(n_out, cout + 2)[:, :cout]
    assert xv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4
    lib.conv2d_rows(xv, x.shape[2:], wp, k, b, s, p, d, addend=av, out=ov)
    assert torch.equal(ov.contiguous(), out), "the strided, unaligned call differs from the contiguous one"
    assert float(ob[0]) == -3.0 and bool((ob[1:].view(n_out, cout + 2)[:, cout:] == -3.0).all())


def test_conv_out_of_domain_returns_its_code():
    from diffreg_hip import lib
    r = lib.raw()
    x, w, o = torch.zeros(25, 4, device=DEV), torch.zeros(4, 36, device=DEV), torch.full((25, 4), 5.0, device=DEV)
    call = lambda *geom, xp=x.data_ptr(), ldx=4: r.dr_conv2d_rows_f32(*geom, xp, ldx, w.data_ptr(), None, None, 0, o.data_ptr(), 4, None)
    assert call(5, 5, 4, 4, 3, 1, 0, 3) == -1 and call(5, 5, 4, 4, 3, 0, 1, 1) == -1 and call(5, 5, 4, 4, 3, 1, 1, 1, ldx=3) == -1
    assert call(5, 5, 4, 4, 3, 1, 1, 1, xp=x.data_ptr() + 2) == -1 and call(5, 5, 4, 4, 32, 1, 16, 1) == -3
    assert r.dr_resize_rows_f32(4, 0, 5, 5, 5, x.data_ptr(), 4, None, 0, o.data_ptr(), 4, None) == -1
    torch.cuda.synchronize()
    assert bool((o == 5.0).all())                                    # nothing was launched


# ---- resize_rows -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.RESIZE_CASES))
@pytest.mark.parametrize("with_addend", [False, True])
def test_resize_rows_against_torch_and_resize_tokens(name, with_addend):
    from diffreg_hip import lib
    src, dst = R.RESIZE_CASES[name]
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    C = 37
    x = torch.randn(1, C, *src, generator=g, device=DEV)
    add = torch.randn(dst[0] * dst[1], C, generator=g, device=DEV) if with_addend else None
    t64 = TF.interpolate(x.double(), size=dst, mode="bilinear", align_corners=True)
    t32 = TF.interpolate(x, size=dst, mode="bilinear", align_corners=True)
    if with_addend:
        t64, t32 = t64 + nchw(add, dst).double(), t32 + nchw(add, dst)
    out = lib.resize_rows(rows(x), src, dst, addend=add)
    held_torch("resize_rows %s%s" % (name, ", addend" if with_addend else ""), nchw(out, dst), t32, t64)
    tok = lib.resize_tokens(x[0], dst)
    assert torch.equal(out, tok + add if with_addend else tok)
    assert torch.equal(out, lib.resize_rows(rows(x), src, dst, addend=add))


# ---- the whole backbone -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_backbone_against_the_reference(name):
    from diffreg_hip.image_backbone2d3d import DeviceImageBackbone
    case = R.CASES[name]
    m = R.build(case, device=DEV)
    x, dino = torch.from_numpy(G[name + "_in_x"]).to(DEV), torch.from_numpy(G[name + "_in_dino"]).to(DEV)
    ib = DeviceImageBackbone(m)
    with torch.no_grad():
        feats, sizes = ib.forward_rows(x, dino)
        outs = ib.forward(x, dino)
    floor = float(G["floor"][0])
    for i in range(4):
        ref = G["%s_out%d_64" % (name, i)]
        assert tuple(outs[i].shape) == ref.shape and outs[i].is_contiguous() and outs[i].dtype == torch.float32
        assert torch.equal(outs[i], nchw(feats[i], sizes[i])), "forward is forward_rows permuted"
        e, d = R.rel_dev(outs[i].cpu(), ref), float(G[name + "_dev32"][i])
        bar = max(floor, 4 * d)
        print("backbone %s out%d: device %.3e from the reference's float64, the reference's float32 %.3e (bar %.3e)" % (name, i, e, d, bar))
        assert e <= bar, (name, i, e, d, bar)


def test_backbone_real_widths():
    from diffreg_hip.image_backbone2d3d import DeviceImageBackbone
    case = R.REAL
    m = R.ImageBackbone(1, case["out"], case["base"]).to(DEV).eval()
    m.load_state_dict(R.make_weights(m, case["seed"], device=DEV))
    x, dino = R.make_inputs(case, device=DEV)
    with torch.no_grad():
        dev = DeviceImageBackbone(m).forward(x, dino)
        t32 = m(x, dino)
        t64 = m.double()(x.double(), dino.double())
    for i in range(4):
        held_torch("real widths out%d %s" % (i, tuple(t64[i].shape)), dev[i], t32[i], t64[i])


def test_accelerate_binds_and_restores_and_falls_back():
    from diffreg_hip.overlay2d3d import accelerate
    case = R.CASES["a"]
    ib = R.build(case, device=DEV)
    stub = torch.nn.Module()
    stub.img_backbone = ib
    stub.denoising_transformer, stub.denoising_coarse_matching = torch.nn.Identity(), torch.nn.Identity()
    stub.get_warped_from_noising_matching3D3D = types.MethodType(lambda self, *a: None, stub)
    x, dino = R.make_inputs(case, device=DEV)
    calls = [0]                                                       # the module's own forward runs its sub-modules; the device path never does
    ib.encoder1.register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
    with torch.no_grad():
        own = ib(x, dino)
    assert calls[0] == 1
    ov = accelerate(stub, image_backbone=True)
    assert "forward" in ib.__dict__
    with torch.no_grad():
        got = ib(x, dino)
    assert calls[0] == 1, "the bound forward ran the module's own code"
    assert all(tuple(a.shape) == tuple(b.shape) and R.rel_dev(a, b) < 1e-5 for a, b in zip(got, own))
    with torch.enable_grad():                                         # gradients enabled: the module's own forward, unchanged
        fb = ib(x, dino)
    assert calls[0] == 2 and all(torch.allclose(a, b, rtol=1e-5, atol=1e-6) for a, b in zip(fb, own))
    ib.train()
    with torch.no_grad():                                             # training mode: the same
        fb = ib(x, dino)
    assert calls[0] == 3 and all(torch.allclose(a, b, rtol=1e-5, atol=1e-6) for a, b in zip(fb, own))
    ib.eval()
    ov.remove()
    assert "forward" not in ib.__dict__ and "_dr_overlay" not in stub.__dict__
    # a module the device path does not cover is refused when binding, never at call time
    ib.decoder1_2[0].act = torch.nn.ReLU()
    with pytest.raises(NotImplementedError):
        accelerate(stub, image_backbone=True)
