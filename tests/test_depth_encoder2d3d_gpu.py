"""Depth-Anything's float32 ViT encoder forward on the device (csrc/vit_f32.hip, csrc/vit_f32_index.h; diffreg_hip/depth_encoder2d3d.py).
Needs a GPU.

Bars.  Error measure: per tensor, max |device - float64|.
 * a primitive (rows GEMM, attention on packed qkv rows) and the production-width block against torch: the op in float64 on the same float32
   inputs, and the device within max(floor, 4 x the deviation of torch's own float32 run from it): DESIGN 5m's rule.  Floors, from the number
   format and not from what the kernels give: a float32 accumulation of K products in any fixed order carries a rounding error of about
   sqrt(K) 2^-24 of its partial sums, and torch's own run can fall far below that by chance on the 16-column, one-row cases, so the GEMM's floor is
   sqrt(K) 2^-24 max |float64 result|; the attention output is a convex combination of v behind an exp whose argument (up to ~8 here) carries a
   2^-24 relative rounding, so its floor is 8 x 2^-24 max |float64 result|.  The production-width case has 131 x 1 024 outputs per tensor and no
   floor.
 * the whole encoder, the three fixture images: every stored tensor within max(floor, 4 x its recorded float32 deviation) of the reference's
   float64 tensor (tests/golden/depth_encoder2d3d_*.npz; floor = the smallest recorded deviation).
Measured and bar are printed."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as TF

from tests import depth_encoder2d3d_ref as R
from tests.helpers import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
DR_OK, DR_EINVAL = 0, -1
EPS24 = 2.0 ** -24
TILES = [-1, 0, 1, 2]                               # the shape's own rule, then each forceable tile
MS, NS = [1, 31, 33, 129, 131], [16, 128, 384]      # N = 16 is the smallest the contract allows


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


@pytest.fixture(scope="module")
def E():
    from diffreg_hip import depth_encoder2d3d as mod
    return mod


@pytest.fixture
def force():
    from diffreg_hip import lib
    lib.ensure_init()
    yield lambda t: lib.raw().dr_debug_gemm_rows_f32_tile(t)
    lib.raw().dr_debug_gemm_rows_f32_tile(-1)


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def held(what, dev, t32, t64, floor):
    e, d = (dev.double() - t64).abs().max().item(), (t32.double() - t64).abs().max().item()
    bar = max(floor, 4 * d)
    print("%s: device %.3e from float64, torch float32 %.3e (bar %.3e)" % (what, e, d, bar))
    assert e <= bar, (what, e, d, bar)


# ---- dr_gemm_rows_f32 ------------------------------------------------------------------------------------------------------------------------------
def epilogue(acc, mode, bias, gamma, addend, resid, cs, cs_cols):
    """the four epilogues on an accumulator [M, N] in its own dtype"""
    v = acc if bias is None else acc + bias.to(acc.dtype)
    if mode == "colscale":
        v = torch.cat((v[:, :cs_cols] * cs, v[:, cs_cols:]), dim=1)
    elif mode == "gelu":
        v = TF.gelu(v)
    elif mode == "scale_resid":
        v = resid.to(acc.dtype) + gamma.to(acc.dtype) * v
    elif addend is not None:
        v = v + addend.to(acc.dtype)
    return v


@pytest.mark.parametrize("K", [128, 608, 1024, 4096])          # 608 = the patch embedding's 3 x 14 x 14 = 588 in its padded form
def test_gemm_rows_against_float64(E, force, K):
    g = gen(100 + K)
    for M in MS:
        for N in NS:
            lda, ldw, ldo = K + 4, K + 8, N + 3                                      # the padded leading dimensions
            a_buf = torch.randn(M, lda, generator=g, device=DEV)
            w_buf = torch.randn(N, ldw, generator=g, device=DEV) * K ** -0.5
            bias, gamma = torch.randn(N, generator=g, device=DEV) * 0.3, torch.rand(N, generator=g, device=DEV) + 0.5
            addend, resid = torch.randn(M, N + 5, generator=g, device=DEV), torch.randn(M, N, generator=g, device=DEV)
            acc64 = a_buf[:, :K].double() @ w_buf[:, :K].double().t()
            acc32 = a_buf[:, :K] @ w_buf[:, :K].t()
            floor = K ** 0.5 * EPS24
            for mode in ("colscale", "gelu", "scale_resid", "addend"):
                for with_bias in (True, False):
                    kw = dict(bias=bias if with_bias else None, gamma=gamma if mode == "scale_resid" else None,
                              addend=addend[:, :N] if mode == "addend" else None)
                    cs, cols = (0.125, 16 * (N // 32)) if mode == "colscale" else (1.0, 0)
                    r64 = epilogue(acc64, mode, kw["bias"], gamma, kw["addend"], resid, cs, cols)
                    r32 = epilogue(acc32, mode, kw["bias"], gamma, kw["addend"], resid, cs, cols)
                    for tile in TILES:
                        for padded in (False, True):
                            a = a_buf[:, :K] if padded else a_buf[:, :K].contiguous()
                            w = w_buf[:, :K] if padded else w_buf[:, :K].contiguous()
                            buf, check = guarded((M, ldo if padded else N), torch.float32, DEV, fill=NAN)
                            out = buf[:, :N]
                            if mode == "scale_resid":
                                out.copy_(resid)
                            force(tile)
                            E.gemm_rows_f32(a, w, mode, out=out, colscale=cs, colscale_cols=cols, **kw)
                            check()
                            assert not padded or bool(torch.isnan(buf[:, N:]).all()), "a pad column of out was written"
                            what = "gemm M %d K %d N %d %s bias %d tile %d ld %d" % (M, K, N, mode, with_bias, tile, padded)
                            held(what, out, r32, r64, floor * r64.abs().max().item())


def test_gemm_rows_small_integers_are_exact(E, force):
    """small-integer operands: every product and partial sum is exact in float32 in ANY order, so a missing, doubled or misplaced k group, row or
    column shows as a wrong integer; the in-place residual mode adds exactly once"""
    g = gen(7)
    for M, K, N in ((131, 1024, 384), (33, 608, 16), (129, 4096, 128)):
        a = torch.randint(-4, 5, (M, K), generator=g, device=DEV).float()
        w = torch.randint(-4, 5, (N, K), generator=g, device=DEV).float()
        bias = torch.randint(-8, 9, (N,), generator=g, device=DEV).float()
        resid = torch.randint(-8, 9, (M, N), generator=g, device=DEV).float()
        want = (a.double() @ w.double().t() + bias.double())
        for tile in TILES:
            force(tile)
            assert torch.equal(E.gemm_rows_f32(a, w, "addend", bias=bias).double(), want), (M, K, N, tile)
            out = resid.clone()
            E.gemm_rows_f32(a, w, "scale_resid", out=out, bias=bias, gamma=torch.full((N,), 2.0, device=DEV))
            assert torch.equal(out.double(), resid.double() + 2.0 * want), (M, K, N, tile)


def test_gemm_rows_tile_rule_is_the_shapes(E):
    """the automatic tile is a function of (M, K, N): two runs of one shape are bit-equal, and equal to the forced tile the rule names"""
    from diffreg_hip import lib
    g = gen(8)
    for (M, K, N), tile in (((131, 128, 384), 0), ((131, 1024, 384), 2), ((2049, 608, 2048), 0), ((1, 4096, 16), 2)):
        a, w = torch.randn(M, K, generator=g, device=DEV), torch.randn(N, K, generator=g, device=DEV)
        auto, again = E.gemm_rows_f32(a, w, "addend"), E.gemm_rows_f32(a, w, "addend")
        lib.raw().dr_debug_gemm_rows_f32_tile(tile)
        try:
            forced = E.gemm_rows_f32(a, w, "addend")
        finally:
            lib.raw().dr_debug_gemm_rows_f32_tile(-1)
        assert torch.equal(auto, again) and torch.equal(auto, forced), (M, K, N, tile)


def test_gemm_rows_refusals_leave_the_output_untouched(E, force):
    M, K, N = 33, 64, 32
    a, w = torch.randn(M, K + 4, device=DEV), torch.randn(N, K + 4, device=DEV)
    bias, add = torch.randn(N + 1, device=DEV), torch.randn(M, N, device=DEV)
    out = torch.full((M, N), 7.0, device=DEV)
    ok = dict(a=a, M=M, K=K, N=N, lda=K + 4, w=w, ldw=K + 4, out=out, ldo=N, mode="addend")
    off = lambda t, n: types.SimpleNamespace(data_ptr=lambda: t.data_ptr() + 4 * n, device=t.device)      # a base pointer n floats further on
    bad = [dict(K=K + 16), dict(K=16), dict(N=N + 8), dict(N=8), dict(M=0), dict(lda=K - 4), dict(lda=K + 2), dict(ldw=K + 3), dict(ldo=N - 1),
           dict(a=off(a, 1)), dict(w=off(w, 2)), dict(gamma=bias), dict(mode="gelu", addend=add), dict(addend=add, ld_addend=N - 1),
           dict(colscale_cols=16), dict(mode="colscale", colscale_cols=8), dict(mode="colscale", colscale_cols=N + 16),
           dict(out=a, ldo=K + 4), dict(out=w, ldo=K + 4), dict(addend=out, ld_addend=N), dict(bias=out),
           dict(mode="scale_resid", gamma=out)]
    for change in bad:
        kw = dict(ok, **change)
        assert E.gemm_rows_f32_raw(**kw) == DR_EINVAL, change
    force(3)                                                                          # a tile that does not exist
    assert E.gemm_rows_f32_raw(**ok) == DR_EINVAL
    force(-1)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert E.gemm_rows_f32_raw(**ok) == DR_OK                                        # (the unchanged arguments are accepted)


# ---- dr_patch_rows_f32 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", R.IMAGES, ids=lambda s: "%dx%d" % s)
def test_patch_rows_against_unfold(E, size):
    H, W = size
    img = torch.randn(3, H, W, generator=gen(3), device=DEV)
    Np = (H // 14) * (W // 14)
    buf, check = guarded((Np, 608 + 8), torch.float32, DEV, fill=NAN)
    E.patch_rows_f32(img, 14, out=buf[:, :608])
    check()
    want = TF.unfold(img[None], 14, stride=14)[0].t()                                # [Np, 588] in the flattened Conv2d weight's k order
    assert torch.equal(buf[:, :588], want) and bool((buf[:, 588:608] == 0).all()) and bool(torch.isnan(buf[:, 608:]).all())


# ---- attention on packed qkv rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 16, 26, 131, 257])
def test_attention_on_packed_qkv_rows(E, L):
    H, d = 2, 64
    g = gen(40 + L)
    qkv = torch.randn(L, 3 * H * d, generator=g, device=DEV)
    qkv[:, :H * d] *= 0.5                                                             # q as the qkv GEMM leaves it: already scaled
    out = E.attention_rows_f32(qkv, H)

    def ref(t):
        q, k, v = t.reshape(L, 3, H, d).permute(1, 2, 0, 3)
        return ((q @ k.transpose(-2, -1)).softmax(dim=-1) @ v).transpose(0, 1).reshape(L, H * d)
    r64 = ref(qkv.double())
    held("attention L %d" % L, out, ref(qkv), r64, 8 * EPS24 * r64.abs().max().item())


# ---- the whole encoder -----------------------------------------------------------------------------------------------------------------------------
def device_all(dev, x):
    with torch.no_grad():
        ff = dev.forward_features(x)
        il = dev.get_intermediate_layers(x, 4, return_class_token=True)
    rec = {"x_norm_patchtokens": ff["x_norm_patchtokens"], "x_norm_clstoken": ff["x_norm_clstoken"], "x_prenorm": ff["x_prenorm"]}
    for k, (o, cl) in enumerate(il):
        rec["inter%d" % k], rec["inter%d_cls" % k] = o, cl
    return rec, ff


@pytest.mark.parametrize("img", range(len(R.IMAGES)))
def test_encoder_against_the_reference(E, fx, img):
    dev = E.DeviceViTF32(R.fixture_vit(fx, torch.float32, DEV))
    x = torch.from_numpy(fx["img%d.x" % img]).to(DEV)
    got, ff = device_all(dev, x)
    assert tuple(ff["x_norm_regtokens"].shape) == (1, 0, 128) and ff["masks"] is None
    floor = min(float(fx["img%d.dev32.%s" % (i, n)]) for i in range(len(R.IMAGES)) for n in R.TENSORS)
    for n in R.TENSORS:
        ref, d = torch.from_numpy(fx["img%d.f64.%s" % (img, n)]), float(fx["img%d.dev32.%s" % (img, n)])
        assert tuple(got[n].shape) == ref.shape and got[n].dtype == torch.float32, n
        e, bar = (got[n].cpu().double() - ref).abs().max().item(), max(floor, 4 * d)
        print("encoder img%d %s: device %.3e from the reference's float64, the reference's float32 %.3e (bar %.3e)" % (img, n, e, d, bar))
        assert e <= bar, (img, n, e, d, bar)


def test_encoder_signature_variants(E, fx):
    """n as a list, norm=False, reshape=True and B = 2 against the restatement in float32 (shapes and 1e-4: the bars are held above)"""
    vit = R.fixture_vit(fx, torch.float32, DEV)
    dev = E.DeviceViTF32(vit)
    x = torch.randn(2, 3, 42, 70, generator=gen(5), device=DEV)
    with torch.no_grad():
        for kw in (dict(n=[1, 3], norm=False), dict(n=2, reshape=True), dict(n=1, return_class_token=True, reshape=True)):
            got, want = dev.get_intermediate_layers(x, **kw), vit.get_intermediate_layers(x, **kw)
            flat = lambda o: [t for e in o for t in (e if isinstance(e, tuple) else (e,))]
            assert len(got) == len(want)
            for a, b in zip(flat(got), flat(want)):
                assert a.shape == b.shape and (a - b).abs().max().item() < 1e-4


def test_encoder_two_runs_are_bit_equal(E, fx):
    dev = E.DeviceViTF32(R.fixture_vit(fx, torch.float32, DEV))
    x = torch.from_numpy(fx["img2.x"]).to(DEV)
    a, _ = device_all(dev, x)
    b, _ = device_all(dev, x)
    assert all(torch.equal(a[n], b[n]) for n in R.TENSORS)


def test_encoder_graph_capture_and_replay_equals_eager(E, fx):
    dev = E.DeviceViTF32(R.fixture_vit(fx, torch.float32, DEV))
    x = torch.from_numpy(fx["img0.x"]).to(DEV)
    with torch.no_grad():
        eager = [t.clone() for pair in dev.get_intermediate_layers(x, 4, return_class_token=True) for t in pair]      # (also caches outside the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                                # one stream, no parallel branches
            captured = [t for pair in dev.get_intermediate_layers(x, 4, return_class_token=True) for t in pair]
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))


def test_encoder_workspace_query_is_sufficient_and_one_byte_less_is_refused(E, fx):
    dev = E.DeviceViTF32(R.fixture_vit(fx, torch.float32, DEV))
    x = torch.from_numpy(fx["img2.x"]).to(DEV)[0]
    n = E.vit_workspace_bytes_f32(140, 182, 14, 128, 512)
    assert n > 0 and n % 256 == 0 and E.vit_workspace_bytes_f32(140, 183, 14, 128, 512) == 0 and E.vit_workspace_bytes_f32(140, 182, 14, 96, 512) == 0
    ws, check = guarded((n,), torch.uint8, DEV)
    pre, nrm, _ = dev._run(x, workspace=ws)
    check()                                                                           # nothing beyond the queried size is touched
    own, own_n, _ = dev._run(x)
    assert torch.equal(pre, own) and torch.equal(nrm, own_n)
    with pytest.raises(RuntimeError, match="invalid argument"):
        dev._run(x, workspace=ws[:n - 1])


def shifted(t):
    """the values of t one float further on in an allocation with slack: data_ptr() + 4 is a 4-byte-aligned, in-bounds copy"""
    buf = torch.zeros(t.numel() + 4, dtype=t.dtype, device=t.device)
    buf[1:1 + t.numel()] = t.reshape(-1)
    return buf


def test_forward_refusal_domain(E):
    """dr_vit_forward_f32's own domain, one field perturbed per case: the workspace on 256 bytes, x_prenorm and every weight MATRIX on 16, every
    vector (pos, a bias) on 4 only, norm_take a flag, the takes inside the depth, eps >= 0, the queried workspace size.  A refusal is DR_EINVAL
    before any launch (outputs and workspace stay poisoned); a vector moved by 4 bytes is taken and gives the same bits.  28 x 28 image, D = 64,
    one head, Dh = 128, one block."""
    from diffreg_hip import lib
    POISON = 777.0
    vit = R.draw_weights(R.ViTF32(patch_size=14, img_size=28, embed_dim=64, depth=1, num_heads=1, mlp_ratio=2).to(DEV).eval(), seed=11)
    dev = E.DeviceViTF32(vit)
    L, D, Dh = 5, 64, 128
    img = torch.randn(3, 28, 28, generator=gen(12), device=DEV)
    Wt, pos = dev._weights(), dev._pos_rows(28, 28)
    need = E.vit_workspace_bytes_f32(28, 28, 14, D, Dh)
    assert need > 0
    sh = dict(pos=shifted(pos), patch_w=shifted(Wt["patch_w"]), qkv_w=shifted(vit.blocks[0].attn.qkv.weight),
              qkv_b=shifted(vit.blocks[0].attn.qkv.bias))
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def run(change):
        c = types.SimpleNamespace()
        c.ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
        c.outs = [torch.full((L + 3, D), POISON, device=DEV) for _ in range(3)]
        c.blocks = (lib.VitBlockF32 * 1)(dev._blocks_c[0])
        c.take, c.take_out = (ctypes.c_int * 1)(0), (ctypes.c_void_p * 1)(c.outs[2].data_ptr())
        c.cfg = lib.VitConfigF32(28, 28, 14, D, 1, Dh, 1, 1e-6, img.data_ptr(), p(Wt["patch_w"]), p(Wt["patch_b"]), p(Wt["cls"]), p(pos), c.blocks,
                                 p(Wt["norm_g"]), p(Wt["norm_b"]), p(c.outs[0]), p(c.outs[1]), 1, 1, c.take, c.take_out, p(c.ws), need)
        change(c)
        c.rc = lib.raw().dr_vit_forward_f32(ctypes.byref(c.cfg), lib.stream_of(img))
        torch.cuda.synchronize()
        return c

    field = lambda name, value: lambda c: setattr(c.cfg, name, value(c) if callable(value) else value)
    block = lambda name: lambda c: setattr(c.blocks[0], name, sh[name].data_ptr() + 4)
    refused = {
        "workspace + 128 B": field("workspace", lambda c: c.cfg.workspace + 128),
        "x_prenorm + 4 B": field("x_prenorm", lambda c: c.cfg.x_prenorm + 4),
        "patch_w + 4 B": field("patch_w", sh["patch_w"].data_ptr() + 4),
        "a block's qkv_w + 4 B": block("qkv_w"),
        "norm_take = 2": field("norm_take", 2),
        "take[0] = depth": lambda c: c.take.__setitem__(0, 1),
        "eps = NaN": field("eps", NAN),
        "workspace_bytes - 1": field("workspace_bytes", need - 1),
    }
    taken = {"pos + 4 B": field("pos", sh["pos"].data_ptr() + 4), "a block's qkv_b + 4 B": block("qkv_b")}
    for name, change in refused.items():
        c = run(change)
        print("dr_vit_forward_f32, %s: status %d" % (name, c.rc))
        assert c.rc == DR_EINVAL, name
        assert all(bool((o == POISON).all()) for o in c.outs) and bool((c.ws == 0x5A).all()), name
    base = run(lambda c: None)                                                        # the unperturbed call is inside the domain
    assert base.rc == DR_OK and not any(bool((o[:L] == POISON).any()) for o in base.outs)
    for name, change in taken.items():
        c = run(change)
        print("dr_vit_forward_f32, %s: status %d" % (name, c.rc))
        assert c.rc == DR_OK, name
        assert all(torch.equal(o, b) for o, b in zip(c.outs, base.outs)), name        # (the guard rows behind the L rows included)
        assert bool((c.ws[need:] == 0x5A).all()), name


def test_production_width_block_against_float64(E):
    """D = 1 024, 16 heads, one block, 131 tokens: the GEMM shapes' K and N of ViT-L/14 (qkv 3 072, fc1 4 096, fc2 over K = 4 096)"""
    vit = R.ViTF32(patch_size=14, img_size=70, embed_dim=1024, depth=1, num_heads=16, mlp_ratio=4).to(DEV).eval()
    R.draw_weights(vit, seed=50)
    v64 = R.ViTF32(patch_size=14, img_size=70, embed_dim=1024, depth=1, num_heads=16, mlp_ratio=4).to(DEV).double().eval()
    v64.load_state_dict(vit.state_dict())
    x = torch.randn(1, 3, 140, 182, generator=gen(51), device=DEV)
    dev = E.DeviceViTF32(vit)
    with torch.no_grad():
        got = dev.forward_features(x)
        t32, t64 = vit.forward_features(x), v64.forward_features(x.double())
        gi = dev.get_intermediate_layers(x, 1, return_class_token=True)[0]
        i32, i64 = vit.get_intermediate_layers(x, 1, return_class_token=True)[0], v64.get_intermediate_layers(x.double(), 1, return_class_token=True)[0]
    for n in ("x_prenorm", "x_norm_patchtokens", "x_norm_clstoken"):
        held("production width " + n, got[n], t32[n], t64[n], 0.0)
    held("production width inter", gi[0], i32[0], i64[0], 0.0)


# ---- the module ------------------------------------------------------------------------------------------------------------------------------------
def test_bind_time_refusals(E, fx):
    make = lambda: R.fixture_vit(fx, torch.float32, DEV)
    E.DeviceViTF32(make())

    def refused(change):
        vit = make()
        change(vit)
        with pytest.raises(NotImplementedError):
            E.DeviceViTF32(vit)
    refused(lambda v: v.half())                                                       # not float32 at all
    refused(lambda v: v.blocks[2].mlp.fc1.half())                                     # not ENTIRELY float32
    refused(lambda v: setattr(v, "num_register_tokens", 4))
    refused(lambda v: setattr(v, "register_tokens", torch.zeros(1, 4, 128, device=DEV)))
    # what DeviceViT refuses
    refused(lambda v: setattr(v.blocks[1], "mlp", torch.nn.Identity()))
    refused(lambda v: setattr(v.blocks[0].mlp, "act", torch.nn.GELU(approximate="tanh")))
    refused(lambda v: setattr(v.blocks[0].mlp, "act", torch.nn.ReLU()))
    refused(lambda v: setattr(v, "num_heads", 4))                                     # head dim 32
    refused(lambda v: setattr(v.patch_embed, "norm", torch.nn.LayerNorm(128).to(DEV)))
    refused(lambda v: setattr(v.blocks[3], "sample_drop_ratio", 0.1))
    refused(lambda v: setattr(v.blocks[0].attn, "attn_drop", torch.nn.Dropout(0.1)))
    refused(lambda v: setattr(v.blocks[0].norm2, "eps", 1e-5))


def test_weights_are_refreshed_after_an_in_place_update(E, fx):
    vit = R.fixture_vit(fx, torch.float32, DEV)
    dev = E.DeviceViTF32(vit)
    x = torch.from_numpy(fx["img0.x"]).to(DEV)
    with torch.no_grad():
        a = dev.forward_features(x)["x_prenorm"]
        vit.patch_embed.proj.weight.mul_(-1.0)                                        # the one weight the module keeps a padded copy of
        vit.blocks[1].mlp.fc2.weight.mul_(2.0)
        vit.blocks[3].ls1.gamma.add_(0.5)
        vit.pos_embed.add_(0.25)
        b = dev.forward_features(x)["x_prenorm"]
        want = vit.forward_features(x)["x_prenorm"]
    assert not torch.equal(a, b) and (b - want).abs().max().item() < 1e-4


def _depth_model(fx):
    vit = R.fixture_vit(fx, torch.float32, DEV)
    head = lambda feats, ph, pw: feats[3][0][:, :, :1].reshape(-1, 1, ph, pw)        # any callable that reads the four (tokens, class token) pairs
    return R.DepthModelStandIn(vit, head).to(DEV).eval(), vit


def test_bind_takes_the_device_path_and_falls_back_and_undoes(E, fx):
    dm, vit = _depth_model(fx)
    x = torch.from_numpy(fx["img0.x"]).to(DEV)
    calls = [0]                                                                       # the module's own method runs its blocks; the device path never does
    vit.blocks[0].register_forward_hook(lambda *a: calls.__setitem__(0, calls[0] + 1))
    with torch.no_grad():
        own = dm(x)
    assert calls[0] == 1
    undo = E.bind(dm)
    assert "get_intermediate_layers" in vit.__dict__ and isinstance(undo.device, E.DeviceViTF32)
    with torch.no_grad():
        got = dm(x)
    assert calls[0] == 1, "the bound method ran the module's own code"
    assert got.shape == own.shape and (got - own).abs().max().item() < 1e-4
    with torch.enable_grad():                                                         # gradients enabled: the module's own method, unchanged
        fb = dm(x)
    assert calls[0] == 2 and torch.equal(fb.detach(), own)
    dm.train()
    with torch.no_grad():                                                             # training mode: the same
        fb = dm(x)
    assert calls[0] == 3 and torch.equal(fb, own)
    dm.eval()
    with torch.no_grad():                                                             # not a float32 batch: the same (and the module's own dtype error)
        with pytest.raises(RuntimeError):
            dm(x.double())
    assert calls[0] == 3
    undo()
    assert "get_intermediate_layers" not in vit.__dict__


def test_accelerate_flag_binds_and_removes(E, fx):
    from diffreg_hip import overlay2d3d
    from tests import dpt2d3d_ref as DR
    from tests.conftest import ROOT
    stub = lambda: types.SimpleNamespace(forward=None)

    def model(dm):
        return types.SimpleNamespace(depth_model=dm, denoising_transformer=stub(), denoising_coarse_matching=stub(),
                                     get_warped_from_noising_matching3D3D=None)
    dm, vit = _depth_model(fx)
    x = torch.from_numpy(fx["img0.x"]).to(DEV)
    with torch.no_grad():
        own = dm(x)
    m = model(dm)
    ov = overlay2d3d.accelerate(m, depth_encoder=True)
    assert "get_intermediate_layers" in vit.__dict__
    with torch.no_grad():
        got = dm(x)
    assert got.shape == own.shape and (got - own).abs().max().item() < 1e-4
    ov.remove()
    assert "get_intermediate_layers" not in vit.__dict__ and "_dr_overlay" not in m.__dict__
    m = model(dm)
    ov = overlay2d3d.accelerate(m)                                                    # opt-in: off by default
    assert "get_intermediate_layers" not in vit.__dict__
    ov.remove()
    # with depth_head=True as well: the image tensor to the depth map in the library (the DPT head's fixture module behind this encoder)
    head = DR.small_head(device=DEV, weights=DR.load_fixture(ROOT)["weights"])
    dm2 = R.DepthModelStandIn(vit, head).to(DEV).eval()
    with torch.no_grad():
        own2 = dm2(x)
    m = model(dm2)
    ov = overlay2d3d.accelerate(m, depth_encoder=True, depth_head=True)
    assert "get_intermediate_layers" in vit.__dict__ and "forward" in head.__dict__
    with torch.no_grad():
        got2 = dm2(x)
    assert got2.shape == own2.shape and (got2 - own2).abs().max().item() <= 1e-4 * max(1.0, own2.abs().max().item())
    ov.remove()
    assert "get_intermediate_layers" not in vit.__dict__ and "forward" not in head.__dict__
    vit.num_register_tokens = 4                                                       # refused when binding, and no site stays bound
    m = model(dm2)
    with pytest.raises(NotImplementedError):
        overlay2d3d.accelerate(m, depth_encoder=True, depth_head=True)
    assert m.denoising_transformer.forward is None and "forward" not in head.__dict__ and "get_intermediate_layers" not in vit.__dict__
