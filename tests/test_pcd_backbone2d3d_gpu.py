"""GPU: the 2D-3D point backbone on the device (csrc/backbone2d3d.hip, diffreg_hip/pcd_backbone2d3d.py, overlay2d3d backbone=True).

Kernels against float64 torch (bar 1e-5 of the tensor's maximum: a float32 evaluation of a few roundings per entry after float64 reductions,
~1e-6, with a 10x margin).  The whole backbone against the reference-minted fixture (tests/golden/pcd_backbone2d3d*.npz): outputs
|dev - ref64| <= 1e-4 max|ref64|; per gradient tensor |dev - ref64| <= max(1e-3 max|ref64|, 2 max|ref32 - ref64|) (tests/test_train2d3d_gpu.py);
the neighbour counts of every KPConv call equal.  Outputs are stored quantised at max/2^18 (tests/pcd_backbone2d3d_ref.quantise)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import pcd_backbone2d3d_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GN_CASES = [(16, 2), (32, 4), (64, 8), (128, 16), (256, 32), (512, 32)]


def _rel(dev, ref):
    dev, ref = torch.as_tensor(dev).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    assert dev.shape == ref.shape, (dev.shape, ref.shape)
    return float((dev - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _gn64(a, w, b, G):
    return F.group_norm(a.t().unsqueeze(0), G, w, b, 1e-5).squeeze(0).t()


# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,G", GN_CASES)
@pytest.mark.parametrize("second", ["none", "norm", "raw"])
@pytest.mark.parametrize("act", [True, False])
def test_group_norm_forward_backward(C, G, second, act):
    from diffreg_hip import lib
    torch.manual_seed(C + G)
    N = 1000                                              # not a multiple of the 256-row slab
    a = (torch.randn(N, C) * 2 + 0.5).double()
    b = (torch.randn(N, C) - 0.3).double()
    wa, ba, wb, bb = (1 + 0.3 * torch.randn(C)).double(), (0.2 * torch.randn(C)).double(), (1 + 0.3 * torch.randn(C)).double(), (0.2 * torch.randn(C)).double()
    gout = torch.randn(N, C).double()
    slope = 0.2 if act else None
    leaves = [t.clone().requires_grad_(True) for t in (a, wa, ba, b, wb, bb)]
    A, WA, BA, B, WB, BB = leaves
    y = _gn64(A, WA, BA, G)
    if second == "norm":
        y = y + _gn64(B, WB, BB, G)
    elif second == "raw":
        y = y + B
    ref = F.leaky_relu(y, 0.2) if act else y
    ref.backward(gout)
    f = lambda t: t.float().to(DEV).contiguous()
    sa = lib.group_norm_stats(f(a), G)
    sb = lib.group_norm_stats(f(b), G) if second == "norm" else None
    bdev = f(b) if second != "none" else None
    out = lib.group_norm_apply(f(a), sa, f(wa), f(ba), bdev, sb, f(wb) if sb else None, f(bb) if sb else None, slope)
    e = _rel(out, ref)
    print("GN C=%d G=%d %s act=%s: forward %.2e" % (C, G, second, act, e))
    assert e <= 1e-5
    da, db, dga, dba, dgb, dbb = lib.group_norm_backward(f(gout), out, f(a), sa, f(wa), bdev, sb, f(wb) if sb else None, slope)
    checks = [(da, A.grad, "da"), (dga, WA.grad, "dgamma_a"), (dba, BA.grad, "dbeta_a")]
    if second != "none":
        checks.append((db, B.grad, "db"))
    if second == "norm":
        checks += [(dgb, WB.grad, "dgamma_b"), (dbb, BB.grad, "dbeta_b")]
    for got, want, what in checks:
        e = _rel(got, want)
        print("   %s %.2e" % (what, e))
        assert e <= 1e-5, what


# ---- kNN interpolation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 256])
def test_knn_interpolate_forward_backward(C):
    from diffreg_hip import lib
    torch.manual_seed(C)
    Nq, Ns, H = 777, 300, 24
    s = torch.rand(Ns, 3).double()
    q = torch.rand(Nq, 3).double()
    q[5] = s[17]                                          # a coincident query / support pair (d^2 = 0)
    inds = torch.randint(0, Ns, (Nq, H))
    inds[:, -5:] = Ns                                     # shadow padding
    inds[3] = Ns                                          # an all-shadow row
    inds[5, 0] = 17
    x = torch.randn(Ns, C).double().requires_grad_(True)
    ref = R.knn_interpolate(q, s, x, inds)
    g = torch.randn(Nq, C).double()
    ref.backward(g)
    f = lambda t: t.float().to(DEV).contiguous()
    buf = torch.full((Nq, C + 7), 3.0, device=DEV)
    lib.knn_interpolate(f(q), f(s), inds.to(DEV), f(x.detach()), out=buf, col=0)
    assert torch.equal(buf[:, C:], torch.full((Nq, 7), 3.0, device=DEV)), "columns outside the slice must stay untouched"
    assert float(buf[3, :C].abs().max()) == 0.0
    e = _rel(buf[:, :C], ref)
    gbuf = torch.zeros(Nq, C + 7, device=DEV)
    gbuf[:, :C] = f(g)
    gx = lib.knn_interpolate_backward(f(q), f(s), inds.to(DEV), gbuf, C, col=0)
    eb = _rel(gx, x.grad)
    print("kNN interpolation C=%d: forward %.2e backward %.2e" % (C, e, eb))
    assert e <= 1e-5 and eb <= 1e-5


def test_neighbour_lists_wider_than_64_are_refused():
    from diffreg_hip import lib
    from diffreg_hip import pcd_backbone2d3d as P
    s, q = torch.rand(100, 3, device=DEV), torch.rand(50, 3, device=DEV)
    inds = torch.randint(0, 100, (50, 65), device=DEV)
    with pytest.raises(RuntimeError):
        lib.knn_interpolate(q, s, inds, torch.randn(100, 8, device=DEV))
    with pytest.raises(RuntimeError):
        lib.knn_interpolate_backward(q, s, inds, torch.randn(50, 8, device=DEV), 8)
    pyr = R.to_torch(R.make_pyramid("c"), DEV)
    pyr["neighbors"][0] = torch.cat([pyr["neighbors"][0], torch.full((pyr["neighbors"][0].shape[0], 60), pyr["points"][0].shape[0], device=DEV,
                                                                      dtype=torch.int64)], 1)
    m = _module()
    with pytest.raises(RuntimeError):
        P.point_backbone(m, torch.ones(pyr["points"][0].shape[0], 1, device=DEV), pyr)


# ---- the whole backbone against the fixture ------------------------------------------------------------------------------------------------
def _module():
    m = R.PointBackbone()
    m.load_state_dict({**m.state_dict(), **R.make_weights(m)})
    return m.to(DEV)


@pytest.mark.parametrize("name", ["a", "c"])
def test_backbone_against_reference_fixture(golden, name):
    from diffreg_hip import pcd_backbone2d3d as P
    fx, fo = golden("pcd_backbone2d3d"), golden("pcd_backbone2d3d_%s_out" % name)
    pyr_np = R.make_pyramid(name)
    assert np.array_equal(R.pyramid_checksum(pyr_np), fx[name + "_pyramid_checksum"])
    pyr = R.to_torch(pyr_np, DEV)
    m = _module()
    counts = []
    outs = P.point_backbone(m, torch.ones(pyr["points"][0].shape[0], 1, device=DEV), pyr, counts=counts)
    for i, o in enumerate(outs):
        ref = R.dequantise(fo["out%d_q" % i], fo["out%d_step" % i])
        e = _rel(o[::R.OUT_ROWS[name]], ref)
        print("scene %s out%d %s: |dev - ref64| / max = %.2e" % (name, i, tuple(o.shape), e))
        assert e <= 1e-4, i
    assert len(counts) == 8
    for ci, c in enumerate(counts):
        assert np.array_equal(c.cpu().numpy(), fx["%s_counts_%02d" % (name, ci)].astype(np.int32)), ci
    loss = R.loss_of(outs, R.loss_weights(outs))
    loss.backward()
    l64 = float(fx[name + "_loss64"][0])
    print("scene %s loss dev %.9g ref64 %.9g ref32 %.9g" % (name, float(loss), l64, float(fx[name + "_loss32"][0])))
    worst = 0.0
    n = 0
    for pname, p in m.named_parameters():
        g32, g64 = fx["%s_g32_%s" % (name, pname)].astype(np.float64), fx["%s_g64_%s" % (name, pname)]
        assert p.grad is not None, pname
        dev = R.sub_grad(p.grad).double().cpu().numpy()
        M = float(np.abs(g64).max())
        e, r = float(np.abs(dev - g64).max()), float(np.abs(g32 - g64).max())
        worst = max(worst, e / max(max(1e-3 * M, 2 * r), 1e-30))
        assert e <= max(1e-3 * M, 2 * r, 1e-12), (pname, "device %.3e from float64, float32 reference %.3e, tensor max %.3e" % (e, r, M))
        n += 1
    assert n == 110
    print("scene %s: largest gradient error / bar = %.3f" % (name, worst))


def test_eval_forward_no_grad_and_graph_capture():
    from diffreg_hip import pcd_backbone2d3d as P
    pyr = R.to_torch(R.make_pyramid("c"), DEV)
    m = _module()
    feats = torch.ones(pyr["points"][0].shape[0], 1, device=DEV)
    with torch.no_grad():
        eager = P.point_backbone(m, feats, pyr)
        assert all(not o.requires_grad for o in eager)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            cap = P.point_backbone(m, feats, pyr)
        g.replay()
        torch.cuda.synchronize()
    for a, b in zip(cap, eager):
        assert _rel(a, b) <= 1e-6


# ---- the overlay ----------------------------------------------------------------------------------------------------------------------------
class _StandIn(torch.nn.Module):
    """the attributes of MATR2D3D the overlay touches, with a real PointBackbone-shaped module"""

    def __init__(self):
        super().__init__()
        self.pcd_backbone = _module()
        self.transformer, self.coarse_matching = torch.nn.Module(), torch.nn.Module()
        self.denoising_transformer, self.denoising_coarse_matching = torch.nn.Module(), torch.nn.Module()

    def get_warped_from_noising_matching3D3D(self, *a):
        return a


def test_overlay_backbone_flag():
    from diffreg_hip.overlay2d3d import accelerate
    from diffreg_hip import pcd_backbone2d3d as P
    pyr = R.to_torch(R.make_pyramid("c"), DEV)
    feats = torch.ones(pyr["points"][0].shape[0], 1, device=DEV)
    model = _StandIn().to(DEV)
    pb = model.pcd_backbone
    ov = accelerate(model)
    assert "forward" not in pb.__dict__
    ov.remove()
    for train in (False, True):
        model.train(train)
        ov = accelerate(model, training=train, backbone=True)
        assert "forward" in pb.__dict__
        calls = []
        orig = P.point_backbone
        P.point_backbone = lambda *a, **k: calls.append(1) or orig(*a, **k)
        try:
            with torch.set_grad_enabled(train):
                outs = model.pcd_backbone(feats, pyr)
        finally:
            P.point_backbone = orig
        assert calls == [1]
        with torch.no_grad():
            ref = pb.__class__.forward(pb, feats, pyr)
        for a, b in zip(outs, ref):
            assert _rel(a, b) <= 1e-4
        if train:
            pb.zero_grad(set_to_none=True)
            R.loss_of(outs, R.loss_weights(outs)).backward()
            assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in pb.parameters())
        ov.remove()
        assert "forward" not in pb.__dict__
