"""The Depth-Anything DPT head's forward on the device (csrc/conv2d.hip, csrc/conv_index.h; diffreg_hip/dpt2d3d.py).  Needs a GPU.

Bars.  Error measure everywhere: per tensor, max|a - ref64| / max|ref64| (dpt2d3d_ref.rel_dev).
 * a primitive against torch.nn.functional: the op in float64 on the same float32 inputs, and the device within 4 x the deviation of torch's own
   float32 run from it (the rule of test_front2d3d_gpu.py::held_torch with the margin test_image_backbone2d3d_gpu.py uses for this kernel family;
   no floor).  Measured and bar are printed.
 * the whole head, the three fixture grids: every named intermediate and the output within max(floor, 4 x the reference's recorded float32
   deviation) of the reference's float64 tensor (tests/golden/dpt2d3d_*.npz; floor = the smallest recorded deviation).
Inputs are drawn symmetric about zero, so each ReLU flag changes the result (asserted).  torch's own convolutions run with the vendor convolution
library switched off (torch.backends.cudnn.flags(enabled=False): torch's native float32 kernels), so that no case waits for that library's
per-shape kernel search; the float64 runs take torch's native kernels either way."""
import itertools
import types

import pytest
import torch
import torch.nn.functional as TF

from tests import dpt2d3d_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _native_torch_convolutions():
    with torch.backends.cudnn.flags(enabled=False):
        yield
DEV = "cuda:0"
SIZES = [(3, 5), (5, 7), (33, 35)]                       # 33 x 35 = 1 155 pixels: across a 64-row tile and not a multiple of it
KINDS = {"k3p1": (3, 1, 1), "k1": (1, 1, 0), "k3s2": (3, 2, 1)}       # (k, stride, padding)


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture(ROOT)


@pytest.fixture(scope="module")
def lib():
    from diffreg_hip import lib as L
    return L


def held_torch(what, dev, t32, t64):
    e, d = R.rel_dev(dev, t64), R.rel_dev(t32, t64)
    print("%s: device %.3e from float64, torch float32 %.3e (bar %.3e)" % (what, e, d, 4 * d))
    assert e <= 4 * d, (what, e, d, 4 * d)


def rows(t):
    """[1, C, H, W] -> [H W, C]"""
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).contiguous()


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def conv_inputs(g, cin, cout, k, H, W):
    x = torch.randn(1, cin, H, W, generator=g, device=DEV)
    w = torch.randn(cout, cin, k, k, generator=g, device=DEV) * (1.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=g, device=DEV) * 0.3
    return x, w, b


def act_ref(x, w, b, s, p, relu_in, relu_out, adds, dt):
    y = TF.conv2d(TF.relu(x.to(dt)) if relu_in else x.to(dt), w.to(dt), b.to(dt), stride=s, padding=p)
    if relu_out:
        y = TF.relu(y)
    for a in adds:
        y = y + a.to(dt)
    return y


# ---- dr_conv2d_rows_act_f32 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("kind", list(KINDS))
def test_act_against_torch(lib, kind, size):
    k, s, p = KINDS[kind]
    H, W = size
    g = gen(11)
    for cin, cout in itertools.product((4, 36, 64), (4, 32, 68, 132)):
        x, w, b = conv_inputs(g, cin, cout, k, H, W)
        wp, xr = lib.pack_conv_weight(w), rows(x)
        ho, wo = lib.conv_out_size(H, k, s, p), lib.conv_out_size(W, k, s, p)
        a1, a2 = (torch.randn(1, cout, ho, wo, generator=g, device=DEV) for _ in range(2))
        plain, _ = lib.conv2d_rows(xr, size, wp, k, b, s, p)
        for relu_in, relu_out, n_add in itertools.product((False, True), (False, True), (0, 1, 2)):
            adds = [a1, a2][:n_add]
            t64, t32 = (act_ref(x, w, b, s, p, relu_in, relu_out, adds, dt) for dt in (torch.float64, torch.float32))
            out, osz = lib.conv2d_rows_act(xr, size, wp, k, b, s, p, relu_in=relu_in, relu_out=relu_out,
                                           addend=rows(a1) if n_add >= 1 else None, addend2=rows(a2) if n_add == 2 else None)
            assert osz == (ho, wo) == tuple(t64.shape[2:])
            held_torch("act %s %dx%d %d->%d in=%d out=%d addends=%d" % (kind, H, W, cin, cout, relu_in, relu_out, n_add), R.nchw(out, osz), t32, t64)
            if not relu_in and not relu_out and n_add == 0:
                assert torch.equal(out, plain), "no flag, no addend2: bit-equal to dr_conv2d_rows_f32"
            if not relu_in and not relu_out and n_add == 1:
                assert torch.equal(out, lib.conv2d_rows(xr, size, wp, k, b, s, p, addend=rows(a1))[0])


def test_act_each_flag_changes_the_result(lib):
    x, w, b = conv_inputs(gen(12), 36, 68, 3, 5, 7)
    wp, xr = lib.pack_conv_weight(w), rows(x)
    assert float(x.min()) < 0 < float(x.max())
    f = lambda i, o: lib.conv2d_rows_act(xr, (5, 7), wp, 3, b, 1, 1, relu_in=i, relu_out=o)[0]
    base, only_in, only_out, both = f(False, False), f(True, False), f(False, True), f(True, True)
    assert float(base.min()) < 0
    assert not torch.equal(base, only_in) and not torch.equal(base, only_out) and not torch.equal(only_in, both) and not torch.equal(only_out, both)
    assert float(only_out.min()) == 0.0 and float(both.min()) == 0.0
    assert torch.equal(xr, rows(x)), "RELU_IN leaves the input itself untouched"
    assert torch.equal(both, f(True, True)), "two runs are bit-equal"


@pytest.mark.parametrize("kind", list(KINDS))
def test_act_leading_dimensions_and_unaligned_base(lib, kind):
    """ldx, lda, lda2, ldo > C and every base pointer 4 bytes off a 16-byte boundary (the scalar-load arm); cells around the views stay untouched"""
    k, s, p = KINDS[kind]
    H, W, cin, cout = 5, 7, 36, 68
    g = gen(13)
    x, w, b = conv_inputs(g, cin, cout, k, H, W)
    wp = lib.pack_conv_weight(w)
    ho, wo = lib.conv_out_size(H, k, s, p), lib.conv_out_size(W, k, s, p)
    a1, a2 = (torch.randn(ho * wo, cout, generator=g, device=DEV) for _ in range(2))
    want, _ = lib.conv2d_rows_act(rows(x), (H, W), wp, k, b, s, p, relu_in=True, relu_out=True, addend=a1, addend2=a2)

    def view(src, n, c, pad, fill):
        buf = torch.full((n * (c + pad) + 1,), fill, device=DEV)
        v = buf[1:].view(n, c + pad)[:, :c]
        if src is not None:
            v.copy_(src)
        return buf, v
    _, xv = view(rows(x), H * W, cin, 3, 7.0)
    _, av = view(a1, ho * wo, cout, 5, 0.0)
    _, bv = view(a2, ho * wo, cout, 1, 0.0)
    ob, ov = view(None, ho * wo, cout, 2, -3.0)
    assert xv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4
    lib.conv2d_rows_act(xv, (H, W), wp, k, b, s, p, relu_in=True, relu_out=True, addend=av, addend2=bv, out=ov)
    assert torch.equal(ov.contiguous(), want), "the strided, unaligned call differs from the contiguous one"
    assert float(ob[0]) == -3.0 and bool((ob[1:].view(ho * wo, cout + 2)[:, cout:] == -3.0).all())


# ---- dr_conv_transpose2d_rows_f32 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(3, 5), (10, 13), (17, 23)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("s", [2, 4])
def test_transpose_against_torch(lib, s, size):
    H, W = size
    g = gen(21)
    for cin, cout, with_bias in itertools.product((4, 36, 64), (4, 20, 64), (True, False)):
        x = torch.randn(1, cin, H, W, generator=g, device=DEV)
        w = torch.randn(cin, cout, s, s, generator=g, device=DEV) * (1.0 / cin) ** 0.5
        b = torch.randn(cout, generator=g, device=DEV) * 0.3 if with_bias else None
        t64 = TF.conv_transpose2d(x.double(), w.double(), None if b is None else b.double(), stride=s)
        t32 = TF.conv_transpose2d(x, w, b, stride=s)
        n = H * s * W * s
        buf = torch.full((n, cout + 3), float("nan"), device=DEV)                   # padded ldo, pre-filled with NaN
        out, osz = lib.conv_transpose2d_rows(rows(x), size, lib.pack_conv_transpose_weight(w), s, b, out=buf[:, :cout])
        assert osz == (H * s, W * s) == tuple(t64.shape[2:])
        assert not bool(torch.isnan(buf[:, :cout]).any()), "every output element is written"
        assert bool(torch.isnan(buf[:, cout:]).all()), "the pad columns are untouched"
        held_torch("transpose s=%d %dx%d %d->%d bias=%d" % (s, H, W, cin, cout, with_bias), R.nchw(buf[:, :cout].contiguous(), osz), t32, t64)
        again, _ = lib.conv_transpose2d_rows(rows(x), size, lib.pack_conv_transpose_weight(w), s, b)
        assert torch.equal(again, buf[:, :cout].contiguous())


# ---- dr_conv2d_rows_project_f32 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("k", [1, 3])
def test_project_against_float64(lib, k, size):
    H, W = size
    p = k // 2
    g = gen(31)
    for cmid, cin, relu in itertools.product((4, 32, 36, 64), (4, 36, 128), (True, False)):
        x, w1, b1 = conv_inputs(g, cin, cmid, k, H, W)
        w2 = torch.randn(1, cmid, 1, 1, generator=g, device=DEV) * (1.0 / cmid) ** 0.5
        # b2 centres the pre-ReLU output on zero: all pixels share one w2, so with few hidden channels an undirected b2 can leave every output
        # on one side of the final ReLU (one nonzero pixel of fifteen was drawn), and a deviation measured on one value holds nobody to anything.
        # It is computed from the inputs alone, in float64.
        pre = TF.conv2d(TF.relu(TF.conv2d(x.double(), w1.double(), b1.double(), padding=p)), w2.double())
        b2 = -pre.median().reshape(1).float()

        def ref(dt):
            y = TF.conv2d(TF.relu(TF.conv2d(x.to(dt), w1.to(dt), b1.to(dt), padding=p)), w2.to(dt), b2.to(dt))
            return TF.relu(y) if relu else y
        t64, t32 = ref(torch.float64), ref(torch.float32)
        buf = torch.full((H * W, 3), float("nan"), device=DEV)                      # ldo = 3
        out, osz = lib.conv2d_rows_project(rows(x), size, lib.pack_conv_weight(w1), k, b1, w2.reshape(-1).contiguous(), b2, padding=p,
                                           relu_out=relu, out=buf[:, 0])
        assert osz == (H, W) and not bool(torch.isnan(buf[:, 0]).any()) and bool(torch.isnan(buf[:, 1:]).all())
        if not relu:
            assert float(t64.min()) < 0 < float(t64.max())
        held_torch("project k=%d %dx%d %d->%d relu=%d" % (k, H, W, cin, cmid, relu), buf[:, 0].reshape(1, 1, H, W), t32, t64)
        again, _ = lib.conv2d_rows_project(rows(x), size, lib.pack_conv_weight(w1), k, b1, w2.reshape(-1).contiguous(), b2, padding=p, relu_out=relu)
        assert torch.equal(again, buf[:, 0].contiguous())


def test_project_refuses_68_hidden_channels(lib):
    x = torch.randn(15, 4, device=DEV)
    with pytest.raises(RuntimeError):
        lib.conv2d_rows_project(x, (3, 5), torch.zeros(68, 36, device=DEV), 3, None, torch.zeros(68, device=DEV), None, padding=1)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_their_code_without_a_launch(lib):
    r = lib.raw()
    x, w, w2 = torch.randn(25, 4, device=DEV), torch.randn(4 * 4 * 4, 36, device=DEV), torch.randn(4, device=DEV)
    o = torch.full((400, 4), 5.0, device=DEV)
    X, Wt, O = x.data_ptr(), w.data_ptr(), o.data_ptr()
    act = lambda cin=4, flags=0, xp=X, op=O, ap=None, a2=None, Hi=5, Wi=5: r.dr_conv2d_rows_act_f32(
        Hi, Wi, cin, 4, 3, 1, 1, 1, xp, cin, Wt, None, flags, ap, 4, a2, 4, op, 4, None)
    assert act(op=X) == -1 and act(ap=O) == -1 and act(a2=O) == -1 and act(op=Wt) == -1                 # out aliases an input
    assert act(cin=3, flags=1) == -3 and act(cin=3, flags=2) == -3 and act(cin=3, a2=X) == -3           # flags with Cin % 4 != 0
    assert act(xp=None) == -1 and act(op=None) == -1 and act(flags=8) == -1 and act(Hi=5000, Wi=5000) == -3
    tr = lambda s=2, xp=X, op=O, wp=Wt, H=5, W=5, cout=4: r.dr_conv_transpose2d_rows_f32(H, W, 4, cout, s, xp, 4, wp, None, op, cout, None)
    assert tr(s=0) == -1 and tr(s=9) == -3 and tr(xp=None) == -1 and tr(op=None) == -1 and tr(wp=None) == -1 and tr(op=X) == -1
    assert tr(H=4096, W=2048) == -3 and tr(s=8, cout=1028) == -3
    pr = lambda cmid=4, xp=X, op=O, w2p=w2.data_ptr(), Hi=5, Wi=5: r.dr_conv2d_rows_project_f32(
        Hi, Wi, 4, cmid, 3, 1, 1, 1, xp, 4, Wt, None, w2p, None, 1, op, 1, None)
    assert pr(cmid=68) == -3 and pr(xp=None) == -1 and pr(op=None) == -1 and pr(w2p=None) == -1 and pr(op=X) == -1 and pr(Hi=5000, Wi=5000) == -3
    torch.cuda.synchronize()
    assert bool((o == 5.0).all()), "nothing was launched"


# ---- the whole head ----------------------------------------------------------------------------------------------------------------------------------
def _feats(fx, grid):
    return tuple((a.to(DEV), b.to(DEV)) for a, b in fx["grids"][grid]["feats"])


@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_head_against_the_reference(fx, grid):
    from diffreg_hip.dpt2d3d import DeviceDPTHead
    ph, pw = R.GRIDS[grid]
    head = DeviceDPTHead(R.small_head(device=DEV, weights=fx["weights"]))
    feats = _feats(fx, grid)
    with torch.no_grad():
        depth, named = head.forward_rows(feats, ph, pw)
        out = head.forward(feats, ph, pw)
    assert tuple(out.shape) == (1, 1, 14 * ph, 14 * pw) and out.dtype == torch.float32 and torch.equal(out.reshape(-1), depth)
    g = fx["grids"][grid]
    for n in R.NAMES:
        ref, d = g["ref64"][n], g["dev32"][n]
        got = R.nchw(*named[n])
        assert tuple(got.shape) == ref.shape, n
        e, bar = R.rel_dev(got.cpu(), ref), max(fx["floor"], 4 * d)
        print("head %s %s: device %.3e from the reference's float64, the reference's float32 %.3e (bar %.3e)" % (grid, n, e, d, bar))
        assert e <= bar, (grid, n, e, d, bar)


def test_two_runs_are_bit_equal(fx):
    from diffreg_hip.dpt2d3d import DeviceDPTHead
    head = DeviceDPTHead(R.small_head(device=DEV, weights=fx["weights"]))
    feats = _feats(fx, "10x13")
    with torch.no_grad():
        a, na = head.forward_rows(feats, 10, 13)
        b, nb = head.forward_rows(feats, 10, 13)
    assert torch.equal(a, b) and all(torch.equal(na[n][0], nb[n][0]) for n in R.NAMES)


def test_weights_are_repacked_when_a_parameter_changes(fx):
    from diffreg_hip.dpt2d3d import DeviceDPTHead
    mod = R.small_head(device=DEV, weights=fx["weights"])
    head = DeviceDPTHead(mod)
    feats = _feats(fx, "3x5")
    with torch.no_grad():
        a = head.forward(feats, 3, 5)
        mod.scratch.output_conv2[2].weight.mul_(2.0)                                # `_version` moves
        mod.resize_layers[0].weight.mul_(-1.0)
        b = head.forward(feats, 3, 5)
        want = mod(feats, 3, 5)
    assert not torch.equal(a, b) and R.rel_dev(b, want) < 1e-4


def test_graph_capture_and_replay_equals_eager(fx):
    from diffreg_hip.dpt2d3d import DeviceDPTHead
    head = DeviceDPTHead(R.small_head(device=DEV, weights=fx["weights"]))
    feats = _feats(fx, "5x5")
    with torch.no_grad():
        eager = head.forward(feats, 5, 5).clone()                                   # (also packs the weights outside the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                               # one stream, no parallel branches
            captured = head.forward(feats, 5, 5)
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured, eager)


# ---- binding -----------------------------------------------------------------------------------------------------------------------------------------
def test_bind_takes_the_device_path_and_falls_back_and_undoes(fx):
    from diffreg_hip import dpt2d3d
    mod = R.small_head(device=DEV, weights=fx["weights"])
    feats = _feats(fx, "3x5")
    calls = [0]                                                                     # the module's own forward runs its sub-modules; the device path never does
    mod.scratch.output_conv1.register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
    with torch.no_grad():
        own = mod(feats, 3, 5)
    assert calls[0] == 1
    undo = dpt2d3d.bind(mod)
    assert "forward" in mod.__dict__
    with torch.no_grad():
        got = mod(feats, 3, 5)
    assert calls[0] == 1, "the bound forward ran the module's own code"
    assert tuple(got.shape) == tuple(own.shape) and R.rel_dev(got, own) < 1e-4
    with torch.enable_grad():                                                       # gradients enabled: the module's own forward, unchanged
        fb = mod(feats, 3, 5)
    assert calls[0] == 2 and torch.equal(fb.detach(), own)
    mod.train()
    with torch.no_grad():                                                           # training mode: the same
        fb = mod(feats, 3, 5)
    assert calls[0] == 3 and torch.equal(fb, own)
    mod.eval()
    with torch.no_grad():                                                           # CPU inputs: the same
        mod.cpu()(tuple((a.cpu(), b.cpu()) for a, b in feats), 3, 5)
    assert calls[0] == 4
    undo()
    assert "forward" not in mod.__dict__


def test_accelerate_flag_binds_and_removes(fx):
    from diffreg_hip import overlay2d3d
    mod = R.small_head(device=DEV, weights=fx["weights"])
    stub = lambda: types.SimpleNamespace(forward=None)
    model = lambda: types.SimpleNamespace(depth_model=types.SimpleNamespace(depth_head=mod), denoising_transformer=stub(),
                                          denoising_coarse_matching=stub(), get_warped_from_noising_matching3D3D=None)
    m = model()
    ov = overlay2d3d.accelerate(m, depth_head=True)
    assert "forward" in mod.__dict__
    with torch.no_grad():
        got = mod(_feats(fx, "3x5"), 3, 5)
    assert tuple(got.shape) == (1, 1, 42, 70)
    ov.remove()
    assert "forward" not in mod.__dict__ and "_dr_overlay" not in m.__dict__
    m = model()
    ov = overlay2d3d.accelerate(m)                                                  # opt-in: off by default
    assert "forward" not in mod.__dict__
    ov.remove()
    mod.use_clstoken = True                                                         # refused when binding, before any site is bound
    m = model()
    with pytest.raises(NotImplementedError):
        overlay2d3d.accelerate(m, depth_head=True)
    assert m.denoising_transformer.forward is None
