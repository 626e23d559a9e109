"""Every form of csrc/conv2d.hip's implicit-GEMM kernel (conv2d_mfma_kernel), one at a time, against torch's float64 convolution at its tile
edges: the 64 x 64 tile with the 8-term window (S), the 64 x 64 tile with the 32-term window (M) and the single-buffer 128 x 128 tile (L), for
the three slot maps (forward, data gradient, transposed), the three epilogues (plain, ACT, PROJECT) and the two load arms (16-byte, scalar).
The cases and the form each one must select are tests/conv_plan.py's table; every call asserts conv_plan's form and arm for its own shape and
pointers before it runs, and tests/test_conv_plan_cpu.py holds conv_plan to the source.  Needs a GPU.

References: torch.nn.functional.conv2d / conv_transpose2d / autograd through conv2d in float64 on the device, on the same float32 inputs
(torch's native kernels: the vendor convolution library is switched off as in test_dpt2d3d_gpu.py).  Computed once per (case, inputs) and shared.

Checks.
 * indexing, exact: x in [-3, 3], weights in [-2, 2], bias and addends small integers.  Every partial sum is then an integer below 2^24
   (|sum| <= 6 * 1 152, times 2 * 36 for the project entry's second product), exact in float32 in any order: torch.equal with float64.
 * rounding: normal inputs scaled as conv_inputs does; the device's deviation from float64 (max|a - ref| / max|ref|) at most 4 x that of torch's
   own float32 run -- held_torch of the existing conv tests, restated below with the same number.  Both deviations are printed.
 * arms: the scalar arm (every base pointer 4 bytes off a 16-byte boundary, every leading dimension C + an odd pad) is bit-equal to the
   16-byte arm; two runs are bit-equal.
 * nothing outside is touched: EVERY device call of this file reads its operands from views whose pad columns, guard rows and surroundings hold
   NaN and writes into a NaN-filled buffer with pad columns and guard rows; afterwards every output element is finite and every other cell of the
   output buffer is still NaN.  (A read of a NaN would reach the output through the multiply-add, except under RELU_IN, which maps NaN to 0:
   the calls without that flag carry this check for the loads.)
 * the ACT epilogue on M: the four (relu_in, relu_out) x 0 / 1 / 2 addends; with no flag and no addend2 bit-equal to dr_conv2d_rows_f32.  On L and
   on every other forward case: relu_in + relu_out + two addends, and the bit-equality with the plain entry.
 * the threshold pairs (180 x 181 | 181 x 181) share their first 180 image rows of input: away from the last image row's receptive field both
   forms are held to the same float64 reference under the same bar, and are bit-equal to each other there -- the tile shape and the number of LDS
   buffers change nothing in the order of any output element's sum (asserted; observed on an MI355X)."""
import itertools

import pytest
import torch
import torch.nn.functional as TF

from tests import conv_plan as P
from tests.dpt2d3d_ref import rel_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F32, F64 = torch.float32, torch.float64
IDS = [c["id"] for c in P.CASES]
RATIOS = {}                     # what -> (device deviation, torch float32 deviation)


@pytest.fixture(autouse=True)
def _native_torch_convolutions():
    with torch.backends.cudnn.flags(enabled=False):
        yield


@pytest.fixture(scope="module")
def lib():
    from diffreg_hip import lib as L
    return L


def held_torch(what, dev, t32, t64):
    """the bar of test_dpt2d3d_gpu.py / test_image_backbone2d3d_gpu.py: 4 x torch float32's own deviation from float64, no floor"""
    e, d = rel_dev(dev, t64), rel_dev(t32, t64)
    RATIOS[what] = (e, d)
    print("%s: device %.3e from float64, torch float32 %.3e (bar %.3e, ratio to bar %.3f)" % (what, e, d, 4 * d, e / (4 * d)))
    assert e <= 4 * d, (what, e, d, 4 * d)


def rows(t):
    """[1, C, H, W] -> [H W, C]"""
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1]).contiguous()


def out_hw(g):
    return P.conv_out_size(g["H"], g["k"], g["s"], g["p"]), P.conv_out_size(g["W"], g["k"], g["s"], g["p"])


# ---- inputs and references, once per (case, kind) ------------------------------------------------------------------------------------------------------
_IN, _REF, _PACKED = {}, {}, {}


def inputs(cid, kind):
    """kind "int": small integers (exact sums); "normal": conv_inputs' scaling.  A paired case takes its pair's first H image rows."""
    if (cid, kind) in _IN:
        return _IN[(cid, kind)]
    c = P.BY_ID[cid]
    g, entry = c["geom"], c["entry"]
    if c["pair"]:
        big, gb = inputs(c["pair"], kind), P.BY_ID[c["pair"]]["geom"]
        assert gb["W"] == g["W"] and gb["H"] > g["H"] and (g["k"], g["s"], g["p"]) == (3, 1, 1)
        n = g["H"] * g["W"]                                   # k3 s1 p1: the output image is the input image
        T = {k: (v[:, :, :g["H"]].contiguous() if k in ("x", "go") else v[:n].contiguous() if k in ("a1", "a2") else v) for k, v in big.items()}
        _IN[(cid, kind)] = T
        return T
    gen = torch.Generator(device=DEV)
    gen.manual_seed(500 + 2 * IDS.index(cid) + (kind == "int"))
    if kind == "int":
        draw = lambda lim, *shape: torch.randint(-lim, lim + 1, shape, generator=gen, device=DEV).float()
        scale = lambda fan: 1.0
    else:
        draw = lambda lim, *shape: torch.randn(*shape, generator=gen, device=DEV)
        scale = lambda fan: (1.0 / fan) ** 0.5
    H, W, cin, cout = g["H"], g["W"], g["cin"], g["cout"]
    T = {}
    if entry == "Trans":
        s = g["s"]
        T["x"] = draw(3, 1, cin, H, W)
        T["w"] = draw(2, cin, cout, s, s) * scale(cin)
        T["b"] = draw(4, cout) * (1.0 if kind == "int" else 0.3)
    else:
        k = g["k"]
        ho, wo = out_hw(g)
        T["w"] = draw(2, cout, cin, k, k) * scale(cin * k * k)
        if entry == "Bwd":
            T["go"] = draw(3, 1, cout, ho, wo)
            T["a1"] = draw(5, H * W, cin)
        else:
            T["x"] = draw(3, 1, cin, H, W)
            T["b"] = draw(4, cout) * (1.0 if kind == "int" else 0.3)
            if entry == "Fwd":
                T["a1"], T["a2"] = draw(5, ho * wo, cout), draw(5, ho * wo, cout)
            else:
                T["w2"] = draw(2, cout) * scale(cout)
                if kind == "int":
                    T["b2"] = draw(4, 1)
                else:
                    # b2 centres the pre-ReLU output on zero (see test_dpt2d3d_gpu.py::test_project_against_float64), from the inputs alone
                    pre = TF.conv2d(TF.relu(TF.conv2d(T["x"].double(), T["w"].double(), T["b"].double(), padding=g["p"])),
                                    T["w2"].double().reshape(1, -1, 1, 1))
                    T["b2"] = -pre.median().reshape(1).float()
    lead = T["go"] if entry == "Bwd" else T["x"]
    assert float(lead.min()) < 0 < float(lead.max()) and float(T["w"].min()) < 0 < float(T["w"].max())
    _IN[(cid, kind)] = T
    return T


def base_ref(cid, kind, dt, relu_in=False):
    """the case's operation in dtype dt as rows [n, C]: Fwd conv(relu_in?(x)) + b; Bwd grad_x by autograd; Trans conv_transpose + b;
    PROJECT w2 . relu(conv + b1) + b2 (before the last ReLU)"""
    key = (cid, kind, dt, relu_in)
    if key in _REF:
        return _REF[key]
    c = P.BY_ID[cid]
    g, entry, T = c["geom"], c["entry"], inputs(cid, kind)
    if entry == "Trans":
        r = rows(TF.conv_transpose2d(T["x"].to(dt), T["w"].to(dt), T["b"].to(dt), stride=g["s"]))
    elif entry == "Bwd":
        xx = torch.zeros(1, g["cin"], g["H"], g["W"], dtype=dt, device=DEV, requires_grad=True)
        (TF.conv2d(xx, T["w"].to(dt), None, stride=g["s"], padding=g["p"]) * T["go"].to(dt)).sum().backward()
        r = rows(xx.grad)
    else:
        x = TF.relu(T["x"].to(dt)) if relu_in else T["x"].to(dt)
        y = TF.conv2d(x, T["w"].to(dt), T["b"].to(dt), stride=g["s"], padding=g["p"])
        if entry == "Fwd/PROJECT":
            y = TF.conv2d(TF.relu(y), T["w2"].to(dt).reshape(1, -1, 1, 1), T["b2"].to(dt))
        r = rows(y)
    _REF[key] = r
    return r


def act_ref(cid, kind, dt, relu_in, relu_out, n_add):
    T, y = inputs(cid, kind), base_ref(cid, kind, dt, relu_in)
    if relu_out:
        y = TF.relu(y)
    for a in (T["a1"], T["a2"])[:n_add]:
        y = y + a.to(dt)
    return y


# ---- the device calls: every operand in a NaN frame ----------------------------------------------------------------------------------------------------
def framed(src, n, C, pad, mis):
    """a [n, C] view with leading dimension C + pad whose base is 4 mis bytes past a 16-byte boundary, inside a NaN-filled buffer: pad columns,
    one guard row before and after, and at least 4 floats around those -> (buffer, view)"""
    ld = C + pad
    lead = 4 + (mis - ld) % 4
    buf = torch.full((lead + (n + 2) * ld + 4,), NAN, device=DEV)
    v = buf[lead:lead + (n + 2) * ld].view(n + 2, ld)[1:n + 1, :C]
    if src is not None:
        v.copy_(src)
    assert v.data_ptr() % 16 == 4 * mis and v.stride(0) == ld
    return buf, v


def flat(src, mis):
    """a contiguous copy of src whose base is 4 mis bytes past a 16-byte boundary, NaN before and after"""
    n = src.numel()
    buf = torch.full((4 + mis + n + 4,), NAN, device=DEV)
    v = buf[4 + mis:4 + mis + n].view(src.shape)
    v.copy_(src)
    assert v.data_ptr() % 16 == 4 * mis and v.is_contiguous()
    return v


def device(lib, cid, kind, arm, entry=None, relu_in=False, relu_out=False, n_add=0):
    """one call of the case's entry on the given load arm -> the result as contiguous rows.  Asserts the form and the arm conv_plan predicts,
    that every output element was written with a finite value, and that nothing around the output was."""
    c = P.BY_ID[cid]
    g, T = c["geom"], inputs(cid, kind)
    entry = entry or P.entries_of(c)[0]
    assert entry in P.entries_of(c) and P.case_plan(c) == c["form"], (cid, entry, P.case_plan(c))
    mis, apad = (0, 4) if arm == "vec" else (1, 3)
    H, W, cin, cout = g["H"], g["W"], g["cin"], g["cout"]
    size = (H, W)
    if (cid, kind) not in _PACKED:
        pack = {"Trans": lib.pack_conv_transpose_weight, "Bwd": lib.pack_conv_weight_t}.get(entry, lib.pack_conv_weight)
        _PACKED[(cid, kind)] = (pack(T["w"]), rows(T["go"] if entry == "Bwd" else T["x"]))
    packed, a_rows = _PACKED[(cid, kind)]
    w = flat(packed, mis)
    if entry == "Bwd":
        ho, wo = out_hw(g)
        n_a, c_a, n_o, c_o = ho * wo, cout, H * W, cin
    elif entry == "Trans":
        n_a, c_a, n_o, c_o = H * W, cin, H * g["s"] * W * g["s"], cout
    else:
        ho, wo = out_hw(g)
        n_a, c_a, n_o, c_o = H * W, cin, ho * wo, (1 if entry == "Fwd/PROJECT" else cout)
    _, av = framed(a_rows, n_a, c_a, apad, mis)
    ob, ov = framed(None, n_o, c_o, 3, mis)
    adds = [framed(T["a%d" % (i + 1)], n_o, c_o, pad, mis)[1] for i, pad in zip(range(n_add), (5, 1))] + [None, None]
    assert P.arm((av.data_ptr(), w.data_ptr()), av.stride(0)) == arm, (cid, arm)
    if entry == "Fwd/plain":
        assert not relu_in and not relu_out and n_add <= 1
        _, osz = lib.conv2d_rows(av, size, w, g["k"], flat(T["b"], mis), g["s"], g["p"], addend=adds[0], out=ov)
        assert osz == (ho, wo)
    elif entry == "Fwd/ACT":
        lib.conv2d_rows_act(av, size, w, g["k"], flat(T["b"], mis), g["s"], g["p"], relu_in=relu_in, relu_out=relu_out, addend=adds[0],
                            addend2=adds[1], out=ov)
    elif entry == "Bwd":
        lib.conv2d_rows_backward_data(av, size, w, g["k"], g["s"], g["p"], addend=adds[0], out=ov)
    elif entry == "Trans":
        lib.conv_transpose2d_rows(av, size, w, g["s"], flat(T["b"], mis), out=ov)
    else:
        lib.conv2d_rows_project(av, size, w, g["k"], flat(T["b"], mis), flat(T["w2"], mis), flat(T["b2"], mis), padding=g["p"], relu_out=relu_out,
                                out=ov[:, 0])
    assert bool(torch.isfinite(ov).all()), "%s %s %s: an output element is unwritten or not finite" % (cid, entry, arm)
    assert int(torch.isnan(ob).sum()) == ob.numel() - n_o * c_o, "%s %s %s: a cell outside the output was written" % (cid, entry, arm)
    return ov.contiguous()


def announce(cid):
    c = P.BY_ID[cid]
    r, n, d = P.case_extents(c)
    print("\n[%s] %s: rows %d cols %d depth %d, %d large tiles -> form %s" % (cid, c["entry"], r, n, d, P.large_tiles(r, n), P.case_plan(c)))


# ---- indexing, exact -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_indexing_is_exact_on_integers(lib, cid):
    announce(cid)
    c = P.BY_ID[cid]
    entry = c["entry"]
    for arm in P.ARMS:
        if entry == "Fwd":
            ref = act_ref(cid, "int", F64, False, False, 1)
            assert float(ref.min()) < 0 < float(ref.max())
            assert torch.equal(device(lib, cid, "int", arm, "Fwd/plain", n_add=1).double(), ref), (cid, arm, "plain")
            ref = act_ref(cid, "int", F64, True, True, 2)
            assert float(ref.min()) < 0 < float(ref.max()) and bool((ref != ref.flatten()[0]).any())
            assert torch.equal(device(lib, cid, "int", arm, "Fwd/ACT", relu_in=True, relu_out=True, n_add=2).double(), ref), (cid, arm, "ACT")
        elif entry == "Bwd":
            ref = base_ref(cid, "int", F64) + inputs(cid, "int")["a1"].double()
            assert float(ref.min()) < 0 < float(ref.max())
            assert torch.equal(device(lib, cid, "int", arm, n_add=1).double(), ref), (cid, arm)
        elif entry == "Trans":
            ref = base_ref(cid, "int", F64)
            assert float(ref.min()) < 0 < float(ref.max())
            assert torch.equal(device(lib, cid, "int", arm).double(), ref), (cid, arm)
        else:
            ref = base_ref(cid, "int", F64)
            assert float(ref.min()) < 0 < float(ref.max()) and float(ref.abs().max()) < 2 ** 24
            assert torch.equal(device(lib, cid, "int", arm, relu_out=False).double(), ref), (cid, arm, "no last ReLU")
            assert torch.equal(device(lib, cid, "int", arm, relu_out=True).double(), TF.relu(ref)), (cid, arm, "last ReLU")
        assert float(ref.abs().max()) < 2 ** 24


# ---- rounding, the two arms, two runs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_rounding_is_held_to_torch_and_the_arms_agree(lib, cid):
    announce(cid)
    c = P.BY_ID[cid]
    entry, what = c["entry"], "%s form %s" % (cid, c["form"])
    if entry == "Fwd":
        vec = device(lib, cid, "normal", "vec", "Fwd/plain")
        held_torch(what + " plain", vec, base_ref(cid, "normal", F32), base_ref(cid, "normal", F64))
        assert torch.equal(vec, device(lib, cid, "normal", "scalar", "Fwd/plain")), "the scalar arm differs from the 16-byte arm"
        assert torch.equal(vec, device(lib, cid, "normal", "vec", "Fwd/plain")), "two runs differ"
        assert torch.equal(vec, device(lib, cid, "normal", "vec", "Fwd/ACT")), "ACT without a flag or an addend differs from the plain entry"
        one = device(lib, cid, "normal", "vec", "Fwd/plain", n_add=1)
        assert torch.equal(one, device(lib, cid, "normal", "vec", "Fwd/ACT", n_add=1)), "ACT with one addend differs from the plain entry"
        assert torch.equal(one, device(lib, cid, "normal", "scalar", "Fwd/ACT", n_add=1))
        full = dict(relu_in=True, relu_out=True, n_add=2)
        act = device(lib, cid, "normal", "vec", "Fwd/ACT", **full)
        held_torch(what + " ACT in=1 out=1 addends=2", act, act_ref(cid, "normal", F32, True, True, 2), act_ref(cid, "normal", F64, True, True, 2))
        assert torch.equal(act, device(lib, cid, "normal", "scalar", "Fwd/ACT", **full)), "ACT: the scalar arm differs from the 16-byte arm"
        assert torch.equal(act, device(lib, cid, "normal", "vec", "Fwd/ACT", **full)), "ACT: two runs differ"
    elif entry == "Fwd/PROJECT":
        for relu in (False, True):
            vec = device(lib, cid, "normal", "vec", relu_out=relu)
            t32, t64 = (TF.relu(base_ref(cid, "normal", dt)) if relu else base_ref(cid, "normal", dt) for dt in (F32, F64))
            if not relu:
                assert float(t64.min()) < 0 < float(t64.max())
            held_torch(what + " relu=%d" % relu, vec, t32, t64)
            assert torch.equal(vec, device(lib, cid, "normal", "scalar", relu_out=relu)), "the scalar arm differs from the 16-byte arm"
            assert torch.equal(vec, device(lib, cid, "normal", "vec", relu_out=relu)), "two runs differ"
    else:
        vec = device(lib, cid, "normal", "vec")
        held_torch(what, vec, base_ref(cid, "normal", F32), base_ref(cid, "normal", F64))
        assert torch.equal(vec, device(lib, cid, "normal", "scalar")), "the scalar arm differs from the 16-byte arm"
        assert torch.equal(vec, device(lib, cid, "normal", "vec")), "two runs differ"


# ---- the ACT epilogue on the 32-term window ------------------------------------------------------------------------------------------------------------
def test_act_epilogue_on_form_M(lib):
    cid = "fwd_M"
    announce(cid)
    x = inputs(cid, "normal")["x"]
    assert float(x.min()) < 0 < float(x.max()), "RELU_IN changes the input"
    seen = {}
    for relu_in, relu_out, n_add in itertools.product((False, True), (False, True), (0, 1, 2)):
        opts = dict(relu_in=relu_in, relu_out=relu_out, n_add=n_add)
        vec = device(lib, cid, "normal", "vec", "Fwd/ACT", **opts)
        held_torch("fwd_M form M ACT in=%d out=%d addends=%d" % (relu_in, relu_out, n_add), vec,
                   act_ref(cid, "normal", F32, relu_in, relu_out, n_add), act_ref(cid, "normal", F64, relu_in, relu_out, n_add))
        assert torch.equal(vec, device(lib, cid, "normal", "scalar", "Fwd/ACT", **opts)), ("the arms differ", opts)
        if not relu_in and not relu_out and n_add < 2:
            assert torch.equal(vec, device(lib, cid, "normal", "vec", "Fwd/plain", n_add=n_add)), "bit-equal to dr_conv2d_rows_f32"
        seen[(relu_in, relu_out, n_add)] = vec
    for n_add in (0, 1, 2):                                               # each flag changes the result
        assert len({seen[(i, o, n_add)].cpu().numpy().tobytes() for i in (False, True) for o in (False, True)}) == 4
    assert float(seen[(False, False, 0)].min()) < 0 and float(seen[(True, True, 0)].min()) == 0.0


# ---- the two sides of the tile-count threshold ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small,large", [("fwd_M_510", "fwd_L"), ("bwd_M_510", "bwd_L")])
def test_threshold_pair_shares_a_reference(lib, small, large):
    announce(small)
    announce(large)
    gs, gl = P.BY_ID[small]["geom"], P.BY_ID[large]["geom"]
    assert P.BY_ID[small]["pair"] == large and P.BY_ID[small]["form"] == "M" and P.BY_ID[large]["form"] == "L"
    key = "go" if P.BY_ID[small]["entry"] == "Bwd" else "x"
    assert torch.equal(inputs(small, "normal")[key], inputs(large, "normal")[key][:, :, :gs["H"]])
    n = (gs["H"] - 1) * gs["W"]                       # k3 s1 p1: image row H - 1 of the small case sees the padding, of the large case a row
    t64, t32 = base_ref(large, "normal", F64)[:n], base_ref(large, "normal", F32)[:n]
    assert rel_dev(base_ref(small, "normal", F64)[:n], t64) < 1e-13, "the two float64 references agree away from the last image row"
    dm, dl = device(lib, small, "normal", "vec")[:n], device(lib, large, "normal", "vec")[:n]
    held_torch("%s form M, first %d image rows" % (small, gs["H"] - 1), dm, t32, t64)
    held_torch("%s form L, first %d image rows" % (large, gs["H"] - 1), dl, t32, t64)
    same = torch.equal(dm, dl)
    print("forms M and L bit-equal on the shared rows: %s (largest difference %.3e)" % (same, float((dm - dl).abs().max())))
    assert same, "the 64 x 64 and the 128 x 128 tile sum every output element in the same order"


def test_report_the_largest_ratio_to_the_bar():
    """not a check of its own: prints the largest device deviation / bar of this file's run (run with -s)"""
    if not RATIOS:
        return
    what = max(RATIOS, key=lambda k: RATIOS[k][0] / (4 * RATIOS[k][1]))
    e, d = RATIOS[what]
    print("\nlargest ratio of device deviation to bar over %d comparisons: %.3f (%s: device %.3e, torch float32 %.3e)"
          % (len(RATIOS), e / (4 * d), what, e, d))
    assert e <= 4 * d
