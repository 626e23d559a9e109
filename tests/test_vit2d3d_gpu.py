"""The fp16 DINOv2 ViT encoder on the device (csrc/vit.hip, csrc/vit_index.h; diffreg_hip/vit2d3d.py).  Needs a GPU.

Bars.  Error measure everywhere: max |a - ref64| over a tensor, ref64 = float64 arithmetic on the same fp16-valued inputs.
 * end to end, the three fixture images (tests/golden/vit2d3d_*.npz, the reference's own recorded runs): every output tensor within 2 x the
   reference's own fp16 deviation from its float64 run, both taken from the fixture.
 * each C entry on its own: fp16 outputs within 2 x the deviation of the same op done by torch in fp16 on the GPU (the reference's arithmetic);
   fp32 outputs additionally within 4 x torch's float32 deviation.  No floor anywhere.
 * guard bands behind every output stay untouched; refused arguments return DR_EINVAL and leave poisoned output untouched.
 * two runs bit-equal; a graph replay bit-equal to the eager run; the workspace query sufficient and one byte less refused; bind / remove /
   bind-time refusals / re-pack after an in-place weight update; one production-width case (D = 1024, 16 heads, one block).
"""
import ctypes
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as TF

from tests import vit2d3d_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
POISON = 777.0


@pytest.fixture(scope="module")
def V():
    from diffreg_hip import vit2d3d
    return vit2d3d


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


@pytest.fixture(scope="module")
def fvit(fx):
    return R.fixture_vit(fx, torch.float16).to(DEV)


@pytest.fixture()
def tile():
    from diffreg_hip import lib
    yield lib.raw().dr_debug_gemm_rows_tile
    lib.raw().dr_debug_gemm_rows_tile(-1)


def dev64(a, ref):
    return (a.double() - ref).abs().max().item()


def held16(what, got, t16, r64):
    e, d = dev64(got, r64), dev64(t16, r64)
    print("%s: device %.3e from float64, torch fp16 %.3e (bar %.3e)" % (what, e, d, 2 * d))
    assert e <= 2 * d, (what, e, d)


def held32(what, got, t32, r64):
    e, d = dev64(got, r64), dev64(t32, r64)
    print("%s: device %.3e from float64, torch float32 %.3e (bar %.3e)" % (what, e, d, 4 * d))
    assert e <= 4 * d, (what, e, d)


def guarded(rows, ld, dtype, guard=3):
    """a poisoned buffer of rows + guard rows; the view of the first `rows`"""
    buf = torch.full((rows + guard, ld), POISON, dtype=dtype, device=DEV)
    return buf, buf[:rows]


def untouched(buf, rows, ncols):
    assert bool((buf[rows:] == POISON).all()), "guard rows written"
    if ncols < buf.shape[1]:
        assert bool((buf[:, ncols:] == POISON).all()), "pad columns written"


# ---- the rows GEMM -------------------------------------------------------------------------------------------------------------------------
GEMM_M = [1, 15, 16, 17, 127, 128, 129, 131]


@pytest.mark.parametrize("tile_cfg", [0, 1, 2])
@pytest.mark.parametrize("N", [16, 112, 128, 384])
@pytest.mark.parametrize("K", [32, 608, 1024])
def test_gemm_rows_every_edge(V, tile, K, N, tile_cfg):
    tile(tile_cfg)
    g = torch.Generator(device=DEV).manual_seed(K * 1000 + N)
    rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
    w = (rn(N, K) * 0.06).half()
    wp = V.pack_weight_f16(w)
    bias16, gamma16 = (rn(N) * 0.1).half(), (torch.rand(N, generator=g, device=DEV) * 1.3 + 0.2).half()
    cs_cols = (N // 16 // 3) * 16 if N >= 48 else 16
    for M in GEMM_M:
        lda = K + 8                                                # lda > K
        abuf = rn(M, lda).half()
        a = abuf[:, :K]
        add16 = rn(M, N).half()
        for use_bias in (False, True):
            b16 = bias16 if use_bias else None
            b32 = bias16.float() if use_bias else None
            lin64 = a.double() @ w.double().t() + (bias16.double() if use_bias else 0.0)
            lin16 = TF.linear(a, w, b16)
            lin32 = TF.linear(a.float(), w.float(), b32)
            tag = "M%d K%d N%d tile%d bias%d " % (M, K, N, tile_cfg, use_bias)
            # F16, the leading columns scaled; `out` offset by one row
            buf, _ = guarded(M + 1, N + 8, torch.float16)
            out = buf[1:M + 1]
            V.gemm_rows_f16(a, wp, N, "f16", out=out, bias=b32, colscale=0.125, colscale_cols=cs_cols)
            scale = torch.ones(N, device=DEV, dtype=torch.float64)
            scale[:cs_cols] = 0.125
            t16 = lin16.clone()
            t16[:, :cs_cols] = t16[:, :cs_cols] * 0.125
            held16(tag + "f16", out[:, :N], t16, lin64 * scale)
            untouched(buf, M + 1, N)
            assert bool((buf[0] == POISON).all())
            # GELU
            buf, out = guarded(M, N, torch.float16)
            V.gemm_rows_f16(a, wp, N, "gelu_f16", out=out, bias=b32)
            held16(tag + "gelu", out, TF.gelu(lin16), TF.gelu(lin64))
            untouched(buf, M, N)
            # LayerScale + residual into the fp32 stream
            x16 = rn(M, N).half()
            buf, out = guarded(M, N + 4, torch.float32)
            out[:, :N] = x16.float()
            V.gemm_rows_f16(a, wp, N, "scale_resid_f32", out=out, bias=b32, gamma=gamma16.float())
            r64 = x16.double() + gamma16.double() * lin64
            held16(tag + "resid", out[:, :N], x16 + lin16 * gamma16, r64)
            held32(tag + "resid", out[:, :N], x16.float() + lin32 * gamma16.float(), r64)
            untouched(buf, M, N)
            # fp32 rows with addend
            buf, out = guarded(M, N, torch.float32)
            V.gemm_rows_f16(a, wp, N, "f32", out=out, bias=b32, addend=add16.float())
            held16(tag + "f32", out, lin16 + add16, lin64 + add16.double())
            held32(tag + "f32", out, lin32 + add16.float(), lin64 + add16.double())
            untouched(buf, M, N)


def test_gemm_rows_refusals_leave_output_untouched(V):
    a = torch.randn(16, 64, device=DEV).half()
    wp = V.pack_weight_f16(torch.randn(32, 64, device=DEV).half())
    out = torch.full((16, 32), POISON, dtype=torch.float16, device=DEV)
    assert V.gemm_rows_f16_raw(a, 16, 48, 32, 64, wp, out, 32, "f16") == EINVAL          # K % 32
    assert V.gemm_rows_f16_raw(a, 16, 64, 24, 64, wp, out, 32, "f16") == EINVAL          # N % 16
    assert V.gemm_rows_f16_raw(a, 16, 64, 32, 64, wp, out, 32, "f16") == 0
    torch.cuda.synchronize()
    assert not bool((out == POISON).any())
    out.fill_(POISON)
    assert V.gemm_rows_f16_raw(a, 16, 48, 32, 64, wp, out, 32, "f16") == EINVAL
    assert V.gemm_rows_f16_raw(a, 16, 64, 24, 64, wp, out, 32, "f16") == EINVAL
    torch.cuda.synchronize()
    assert bool((out == POISON).all())
    with pytest.raises(NotImplementedError):
        V.pack_weight_f16(torch.randn(24, 64, device=DEV).half())


def test_gemm_rows_two_runs_bit_equal(V):
    a, w = torch.randn(131, 1024, device=DEV).half(), (torch.randn(384, 1024, device=DEV) * 0.06).half()
    wp = V.pack_weight_f16(w)
    assert torch.equal(V.gemm_rows_f16(a, wp, 384, "f16"), V.gemm_rows_f16(a, wp, 384, "f16"))


# ---- attention -------------------------------------------------------------------------------------------------------------------------------
def attn_refs(qkv, H):
    L = qkv.shape[0]

    def run(t):
        q, k, v = t.reshape(L, 3, H, 64).permute(1, 2, 0, 3)
        return ((q @ k.transpose(-2, -1)).softmax(dim=-1) @ v).transpose(0, 1).reshape(L, H * 64)
    return run(qkv), run(qkv.double())


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("L", [1, 16, 31, 32, 33, 127, 128, 129, 131])
def test_attention_rows_every_edge(V, L, H):
    g = torch.Generator(device=DEV).manual_seed(L * 10 + H)
    qkv = torch.randn(L, 3 * H * 64, generator=g, device=DEV)
    qkv[:, :H * 64] *= 0.125 * 2.0                                  # q arrives scaled (epilogue of the qkv GEMM)
    buf = torch.full((L + 3, 3 * H * 64 + 8), POISON, dtype=torch.float16, device=DEV)
    buf[:L, :3 * H * 64] = qkv.half()
    qv = buf[:L, :3 * H * 64]                                       # a padded leading dimension
    obuf, out = guarded(L, H * 64 + 4, torch.float16)
    V.attention_rows_f16(qv, H, out=out[:, :H * 64])
    t16, r64 = attn_refs(qv.contiguous(), H)
    held16("attention L%d H%d" % (L, H), out[:, :H * 64], t16, r64)
    untouched(obuf, L, H * 64)
    out2 = V.attention_rows_f16(qv, H)
    assert torch.equal(out2, out[:, :H * 64])                       # two runs bit-equal


def test_attention_rows_running_maximum_moves(V):
    """scores of every row grow with the key index over a span of more than 60: the running maximum moves in every key tile and the accumulators
    must be rescaled each time"""
    L, H = 131, 1
    qkv = torch.zeros(L, 192, device=DEV)
    qkv[:, :64] = 1.0
    qkv[:, 64:128] = (torch.arange(L, device=DEV, dtype=torch.float32) / L)[:, None]       # s[i][j] = 64 j / L
    qkv[:, 128:] = torch.randn(L, 64, device=DEV)
    qkv = qkv.half()
    s = qkv[:, :64].double() @ qkv[:, 64:128].double().t()
    assert (s.max(dim=1).values - s.min(dim=1).values).min().item() > 60
    out = V.attention_rows_f16(qkv, H)
    t16, r64 = attn_refs(qkv, H)
    held16("attention, moving maximum", out, t16, r64)


def test_attention_rows_refuses_other_head_dims(V):
    qkv = torch.zeros(16, 96, dtype=torch.float16, device=DEV)
    out = torch.full((16, 32), POISON, dtype=torch.float16, device=DEV)
    assert V.attention_rows_f16_raw(qkv, 16, 1, 32, 96, out, 32) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == POISON).all())


# ---- LayerNorm, patch rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 131])
@pytest.mark.parametrize("C", [32, 128, 1024])
def test_layernorm_rows(V, C, rows):
    g = torch.Generator(device=DEV).manual_seed(C + rows)
    x = (torch.randn(rows, C, generator=g, device=DEV) * 3 + 1).half()
    x[rows // 2] = 2.5                                              # a constant row: zero variance
    gam, bet = (torch.rand(C, generator=g, device=DEV) + 0.5).half(), (torch.randn(C, generator=g, device=DEV) * 0.1).half()
    xs = torch.full((rows, C + 4), POISON, device=DEV)
    xs[:, :C] = x.float()
    r64 = TF.layer_norm(x.double(), (C,), gam.double(), bet.double(), 1e-6)
    buf, out = guarded(rows, C + 4, torch.float16)
    V.layernorm_rows_f16(xs[:, :C], gam.float(), bet.float(), 1e-6, out=out[:, :C])
    held16("layernorm C%d rows%d" % (C, rows), out[:, :C], TF.layer_norm(x, (C,), gam, bet, 1e-6), r64)
    untouched(buf, rows, C)
    assert torch.equal(out[rows // 2, :C], bet)                     # the constant row is beta exactly
    buf, out = guarded(rows, C, torch.float32)
    V.layernorm_rows_f16(xs[:, :C], gam.float(), bet.float(), 1e-6, out_f32=True, out=out)
    held16("layernorm fp32 out C%d rows%d" % (C, rows), out, TF.layer_norm(x, (C,), gam, bet, 1e-6), r64)
    held32("layernorm fp32 out C%d rows%d" % (C, rows), out, TF.layer_norm(x.float(), (C,), gam.float(), bet.float(), 1e-6), r64)
    untouched(buf, rows, C)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("i", range(3))
def test_patch_rows(V, fx, i, dtype):
    img = torch.from_numpy(fx["img%d.x" % i])[0].to(DEV).to(dtype)
    H, W = img.shape[-2:]
    Np = (H // 14) * (W // 14)
    buf, out = guarded(Np, 608 + 8, torch.float16)
    V.patch_rows_f16(img, 14, out=out[:, :608])
    ref = TF.unfold(img[None].float(), 14, stride=14)[0].t().half()           # [Np, 588] in the flattened Conv2d weight's k order
    assert torch.equal(out[:, :588], ref)
    assert bool((out[:, 588:608] == 0).all())                        # the pad columns are exactly zero
    untouched(buf, Np, 608)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def device_outputs(dev, x):
    ff = dev.forward_features(x)
    il = dev.get_intermediate_layers(x, [0, 1], return_class_token=True, norm=True)
    out = {k: ff[k] for k in ("x_norm_patchtokens", "x_norm_clstoken", "x_prenorm")}
    for k, (o, c) in enumerate(il):
        out["inter%d" % k], out["inter%d_cls" % k] = o, c
    return out


@pytest.mark.parametrize("i", range(3))
def test_fixture_images_within_twice_the_reference_fp16_deviation(V, fx, fvit, i):
    dev = V.DeviceViT(fvit)
    x = torch.from_numpy(fx["img%d.x" % i]).to(DEV)
    got = device_outputs(dev, x)
    bad = []
    for k, t in got.items():
        assert t.dtype == torch.float16
        r64, r16 = fx["img%d.f64.%s" % (i, k)], fx["img%d.f16.%s" % (i, k)]
        assert tuple(t.shape) == r64.shape, k
        e, d = np.abs(t.double().cpu().numpy() - r64).max(), np.abs(r16 - r64).max()
        print("image %d %-20s device %.3e  reference fp16 %.3e  ratio %.2f" % (i, k, e, d, e / d))
        if not e <= 2 * d:
            bad.append((k, e, d))
    assert not bad, bad
    again = device_outputs(dev, x)
    assert all(torch.equal(got[k], again[k]) for k in got)          # two runs bit-equal


def test_reshape_and_last_n_of_get_intermediate_layers(V, fvit):
    dev = V.DeviceViT(fvit)
    x = torch.randn(2, 3, 42, 70, device=DEV).half()                # B > 1 loops over the images
    a = dev.get_intermediate_layers(x, 1, reshape=True)
    b = fvit.get_intermediate_layers(x, 1, reshape=True)
    assert len(a) == 1 and a[0].shape == b[0].shape == (2, 128, 3, 5) and a[0].dtype == b[0].dtype
    assert (a[0].float() - b[0].float()).abs().max().item() < 0.05
    with pytest.raises(NotImplementedError):
        dev.forward_features(x, masks=torch.zeros(2, 15, dtype=torch.bool, device=DEV))


def test_graph_replay_bit_equal(V, fx, fvit):
    dev = V.DeviceViT(fvit)
    img = torch.from_numpy(fx["img2.x"])[0].to(DEV)
    eager = dev._run(img, [0])                                      # also warms: weights packed, position rows cached
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dev._run(img, [0])
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one stream, no branches
        cap = dev._run(img, [0])
    for t in (cap[0], cap[1], cap[2][0]):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap[0], eager[0]) and torch.equal(cap[1], eager[1]) and torch.equal(cap[2][0], eager[2][0])


def test_workspace_query_is_sufficient_and_one_byte_less_is_refused(V, fx, fvit):
    from diffreg_hip import lib
    dev = V.DeviceViT(fvit)
    img = torch.from_numpy(fx["img2.x"])[0].to(DEV)
    ref_pre, ref_norm, _ = dev._run(img)
    Wt, pos = dev._weights(), dev._pos_rows(140, 182)
    need = V.vit_workspace_bytes(140, 182, 14, 128, 512)
    assert need > 0 and V.vit_workspace_bytes(140, 182, 14, 100, 512) == 0
    guard = 4096
    ws = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    x_pre = torch.full((131 + 3, 128), POISON, device=DEV)
    x_norm = torch.full((131 + 3, 128), POISON, dtype=torch.float16, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    cfg = lib.VitConfigF16(140, 182, 14, 128, 2, 512, 2, 1e-6, img.data_ptr(), 0, p(Wt["patch_w"]), p(Wt["patch_b"]), p(Wt["cls"]), p(pos),
                           dev._blocks_c, p(Wt["norm_g"]), p(Wt["norm_b"]), p(x_pre), p(x_norm), 0, None, None, p(ws), need - 1)
    st = lib.stream_of(img)
    assert lib.raw().dr_vit_forward_f16(ctypes.byref(cfg), st) == EINVAL
    torch.cuda.synchronize()
    assert bool((x_pre == POISON).all()) and bool((ws == 0x5A).all())
    cfg.workspace_bytes = need
    assert lib.raw().dr_vit_forward_f16(ctypes.byref(cfg), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(x_pre[:131], ref_pre) and torch.equal(x_norm[:131], ref_norm)
    assert bool((ws[need:] == 0x5A).all()) and bool((x_pre[131:] == POISON).all()) and bool((x_norm[131:] == POISON).all())


def shifted(t):
    """the values of t one float further on in an allocation with slack: data_ptr() + 4 is a 4-byte-aligned, in-bounds copy"""
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=t.device)
    buf[1:1 + t.numel()] = t.reshape(-1)
    return buf


def test_forward_refusal_domain(V):
    """dr_vit_forward_f16's own domain, one field perturbed per case: the workspace on 256 bytes, x_prenorm, pos, patch_b and every block pointer on
    16, the takes inside the depth, heads x 64 = D, eps >= 0, img_f32 a flag, the queried workspace size.  Every case is DR_EINVAL before any
    launch: outputs and workspace stay poisoned.  28 x 28 image, D = 64, one head, Dh = 128, one block."""
    from diffreg_hip import lib
    vit = R.draw_weights(small().to(DEV), seed=11).eval()
    dev = V.DeviceViT(vit)
    L, D, Dh = 5, 64, 128
    img = torch.randn(3, 28, 28, generator=torch.Generator(device=DEV).manual_seed(12), device=DEV).half()
    Wt, pos = dev._weights(), dev._pos_rows(28, 28)
    need = V.vit_workspace_bytes(28, 28, 14, D, Dh)
    assert need > 0
    sh = dict(pos=shifted(pos), patch_b=shifted(Wt["patch_b"]), qkv_b=shifted(vit.blocks[0].attn.qkv.bias.float()))
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(change):
        c = types.SimpleNamespace()
        c.ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
        c.outs = [torch.full((L + 3, D), POISON, dtype=dt, device=DEV) for dt in (torch.float32, torch.float16, torch.float32)]
        c.blocks = (lib.VitBlockF16 * 1)(dev._blocks_c[0])
        c.take, c.take_out = (ctypes.c_int * 1)(0), (ctypes.c_void_p * 1)(c.outs[2].data_ptr())
        c.cfg = lib.VitConfigF16(28, 28, 14, D, 1, Dh, 1, 1e-6, img.data_ptr(), 0, p(Wt["patch_w"]), p(Wt["patch_b"]), p(Wt["cls"]), p(pos),
                                 c.blocks, p(Wt["norm_g"]), p(Wt["norm_b"]), p(c.outs[0]), p(c.outs[1]), 1, c.take, c.take_out, p(c.ws), need)
        change(c)
        c.rc = lib.raw().dr_vit_forward_f16(ctypes.byref(c.cfg), lib.stream_of(img))
        torch.cuda.synchronize()
        return c

    field = lambda name, value: lambda c: setattr(c.cfg, name, value(c) if callable(value) else value)
    cases = {
        "workspace + 128 B": field("workspace", lambda c: c.cfg.workspace + 128),
        "x_prenorm + 4 B": field("x_prenorm", lambda c: c.cfg.x_prenorm + 4),
        "pos + 4 B": field("pos", sh["pos"].data_ptr() + 4),
        "patch_b + 4 B": field("patch_b", sh["patch_b"].data_ptr() + 4),
        "a block's qkv_b + 4 B": lambda c: setattr(c.blocks[0], "qkv_b", sh["qkv_b"].data_ptr() + 4),
        "take[0] = depth": lambda c: c.take.__setitem__(0, 1),
        "a NULL take_out[0]": lambda c: c.take_out.__setitem__(0, None),
        "heads = 2": field("heads", 2),
        "eps = NaN": field("eps", float("nan")),
        "img_f32 = 2": field("img_f32", 2),
        "workspace_bytes - 1": field("workspace_bytes", need - 1),
    }
    for name, change in cases.items():
        c = run(change)
        print("dr_vit_forward_f16, %s: status %d" % (name, c.rc))
        assert c.rc == EINVAL, name
        assert all(bool((o == POISON).all()) for o in c.outs) and bool((c.ws == 0x5A).all()), name
    base = run(lambda c: None)                                      # the unperturbed call is inside the domain
    assert base.rc == 0 and not any(bool((o[:L] == POISON).any()) for o in base.outs)
    assert all(bool((o[L:] == POISON).all()) for o in base.outs) and bool((base.ws[need:] == 0x5A).all())


# ---- binding ------------------------------------------------------------------------------------------------------------------------------------
def test_bind_remove_and_repack(V, fx):
    vit = R.fixture_vit(fx, torch.float16).to(DEV)
    enc = R.EncoderStandIn(vit)
    x = torch.from_numpy(fx["img0.x"]).to(DEV)
    own = enc(x)[16]
    orig = vit.forward_features
    binding = V.bind(enc)
    direct = binding.device.forward_features(x)["x_norm_patchtokens"]
    got = enc(x.float())[16]                                        # the encoder casts its input, as the reference does
    assert got.dtype == torch.float16 and torch.equal(got, direct.permute(0, 2, 1).reshape(1, 128, 3, 5))
    assert (got.float() - own.float()).abs().max().item() < 0.05
    with torch.enable_grad():                                       # gradients enabled: still the device path
        assert torch.equal(enc(x)[16], got)
    # an in-place weight update: the next call uses the new weights
    with torch.no_grad():
        vit.blocks[1].mlp.fc2.weight.mul_(0.5)
        vit.norm.bias.add_(0.25)
    new = enc(x)[16]
    binding.remove()
    assert "forward_features" not in vit.__dict__ and vit.forward_features.__func__ is orig.__func__
    own_new = enc(x)[16]
    assert not torch.equal(new, got)
    assert (new.float() - own_new.float()).abs().max().item() < 0.05 < (got.float() - own_new.float()).abs().max().item()


def small(**kw):
    cfg = dict(patch_size=14, img_size=28, embed_dim=64, depth=1, num_heads=1, mlp_ratio=2)
    cfg.update(kw)
    return R.ViT(**cfg).half()


class GatedFFN(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.w12, self.w3 = nn.Linear(dim, 2 * dim), nn.Linear(dim, dim)


def test_bind_time_refusals(V):
    V.DeviceViT(small())                                            # the covered module binds
    cases = {}
    m = small(); m.blocks[0].mlp = GatedFFN(64).half(); cases["swiglu"] = m
    m = small(); m.blocks[0].mlp = nn.Identity(); cases["identity ffn"] = m
    m = small(); m.blocks[0].mlp.act = nn.ReLU(); cases["relu"] = m
    m = small(); m.blocks[0].mlp.act = nn.GELU(approximate="tanh"); cases["tanh gelu"] = m
    cases["head dim 32"] = small(num_heads=2)
    cases["D % 32"] = small(embed_dim=48)
    m = small(); m.patch_embed.norm = nn.LayerNorm(64).half(); cases["patch norm"] = m
    m = small(); m.blocks[0].mlp.drop = nn.Dropout(0.1); cases["dropout"] = m
    cases["float32"] = small().float()
    for name, mod in cases.items():
        with pytest.raises(NotImplementedError):
            V.DeviceViT(mod)
        enc = R.EncoderStandIn(mod)
        with pytest.raises(NotImplementedError):
            V.bind(enc)
        assert "forward_features" not in mod.__dict__, name


def test_accelerate_flag_binds_the_encoder(V, fx):
    import types
    from diffreg_hip import overlay2d3d
    vit = R.fixture_vit(fx, torch.float16).to(DEV)
    stub = lambda: types.SimpleNamespace(forward=None)
    model = types.SimpleNamespace(encoder=R.EncoderStandIn(vit), denoising_transformer=stub(), denoising_coarse_matching=stub(),
                                  get_warped_from_noising_matching3D3D=None)
    ov = overlay2d3d.accelerate(model, dino=True)
    assert "forward_features" in vit.__dict__
    ov.remove()
    assert "forward_features" not in vit.__dict__
    model = types.SimpleNamespace(encoder=R.EncoderStandIn(vit), denoising_transformer=stub(), denoising_coarse_matching=stub(),
                                  get_warped_from_noising_matching3D3D=None)
    ov = overlay2d3d.accelerate(model)                              # opt-in: off by default
    assert "forward_features" not in vit.__dict__
    ov.remove()


# ---- production widths ---------------------------------------------------------------------------------------------------------------------------
def test_production_width_one_block(V):
    with torch.device(DEV):
        vit = R.ViT(patch_size=14, img_size=70, embed_dim=1024, depth=1, num_heads=16, mlp_ratio=4)
    R.draw_weights(vit, seed=5)                                     # drawn on the device
    vit = vit.half().eval()
    x = torch.randn(1, 3, 42, 70, generator=torch.Generator(device=DEV).manual_seed(6), device=DEV).half()
    got = V.DeviceViT(vit).forward_features(x)
    with torch.no_grad():
        t16 = vit.forward_features(x)
        r64 = vit.double().forward_features(x.double())
    for k in ("x_norm_patchtokens", "x_norm_clstoken", "x_prenorm"):
        held16("production width " + k, got[k], t16[k], r64[k])
