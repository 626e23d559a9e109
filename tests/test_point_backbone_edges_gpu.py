"""The point-convolution primitives under both backbones (csrc/backbone.hip, csrc/backbone_bwd.hip, the kNN-interpolation and neighbour-count
kernels of csrc/backbone2d3d.hip), entry by entry, against the float64 statement of tests/point_backbone_ref.py at the shapes where their lane and
slab arithmetic changes: every CPL instantiation of the two KPConv kernels at Cin on and off a multiple of 64, H = 1 .. 64 neighbour lanes, K = 1 ..
16 kernel points, Nq % 4 = 1, the three shadow ids, queries of count 0 and all-shadow rows; R = 1 / 2 / 5 / 64 row slabs of the column reductions
with C off a multiple of 32 and every leading dimension wider than C; the pools and the interpolation at their index and tie edges.  Needs a GPU.

The bar (as tests/test_image_backbone2d3d_gpu.py::held_torch): a value's deviation from float64, max |a - ref| / max |ref| per tensor, is at most
4 x the deviation of torch's own float32 evaluation of the same expression on the device; where torch's is 0 the result must be equal.  Counts,
indices, padding zeros and sentinels are exact.  tests/test_point_backbone_edges_oracle.py proves on the CPU that the builders decide every
discrete choice away from float32 ties, so a miss here is the kernel's."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import point_backbone_ref as R
from tests.conftest import ROOT
from tests.helpers import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.25            # an exactly representable value no kernel of these computes


def codes():
    """the return codes, read from the public header"""
    text = open(os.path.join(ROOT, "include", "diffreg_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(DR_[A-Z_]+)\s+\(?(-?\d+)\)?", text)}


def at(t, off=0):
    """device pointer of element `off` of a tensor's storage view"""
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def held(what, dev, t32, t64):
    e, d = R.rel_dev(dev, t64), R.rel_dev(t32, t64)
    print("%s: device %.3e from float64, torch float32 %.3e (bar %.3e)" % (what, e, d, 4 * d))
    assert e <= 4 * d, (what, e, d, 4 * d)
    return d


def on_dev(c):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}


def kp_refs(c, influence="linear", aggregation="sum", G=None):
    """float64 and torch-float32 forward (+ gradients of <weighted, G> when G is given) of one case on the device"""
    out = {}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        x = c["x"].detach().to(dt).clone().requires_grad_(G is not None)
        wf, cnt = R.kpconv_weighted(c["q"], c["s"], c["idx"], x, c["kp"], c["extent"], influence, aggregation, dtype=dt)
        if G is not None:
            (wf * G.to(dt)).sum().backward()
            out["g" + name] = x.grad
        out["w" + name], out["c" + name] = wf.detach(), cnt
    return out


def upstream(seed, shape):
    """a large upstream gradient: normal values from the device's generator (the hashed builders are for what a decision hangs on)"""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV)


def padded_grad(G, ld):
    """the upstream gradient in the library's padded layout; the padding columns hold a value the kernel must not read"""
    gw = torch.full((G.shape[0], ld), SENT, device=DEV)
    gw[:, :G.shape[1]] = G
    return gw


# ---- 1. KPConv gather: lanes and channel groups ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.KPCONV_CASES, ids=R.kpconv_id)
def test_kpconv_gather_lanes_and_channel_groups(case):
    from diffreg_hip import lib
    cin, H, K, shadow = case
    c = on_dev(R.kpconv_case(cin, H, K, shadow))
    Nq, Ns, KC = c["q"].shape[0], c["s"].shape[0], K * cin
    G = upstream(21 + cin + H, (Nq, KC))
    ref = kp_refs(c, G=G)
    wf = lib.kpconv_gather(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"])
    assert wf.shape[1] == (KC + 3) // 4 * 4 and not wf[:, KC:].any()
    cnt = lib.kpconv_neighbor_count(c["idx"], c["x"], Ns)
    assert torch.equal(cnt.long(), ref["c64"]) and torch.equal(ref["c64"], c["counts"])
    assert int(cnt[c["qneg"]]) == 0 and not cnt[-5:].any() and not wf[-5:].any()
    held("weighted", wf[:, :KC], ref["w32"], ref["w64"])
    un, _ = R.kpconv_weighted(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"], normalise=False)
    held("weighted = unnormalised / device count", wf[:, :KC], ref["w32"], un / cnt.clamp(min=1)[:, None])
    held("weighted, the query of count 0", wf[c["qneg"], :KC], ref["w32"][c["qneg"]], un[c["qneg"]])
    gx = lib.kpconv_gather_backward(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"], padded_grad(G, wf.shape[1]))
    held("grad_x", gx, ref["g32"], ref["g64"])


# ---- 2. influence and aggregation modes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("influence,aggregation", R.MODE_CASES)
def test_kpconv_modes(influence, aggregation):
    from diffreg_hip import lib
    c = on_dev(R.mode_case())
    Nq, Ns, cin = c["q"].shape[0], c["s"].shape[0], c["x"].shape[1]
    KC = c["kp"].shape[0] * cin
    G = upstream(22, (Nq, KC))
    ref = kp_refs(c, influence, aggregation, G)
    wf = lib.kpconv_gather(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"], influence, aggregation)
    held("weighted", wf[:, :KC], ref["w32"], ref["w64"])
    qi = c["tie"][0]
    held("weighted, the mirror tie's query", wf[qi, :KC], ref["w32"][qi], ref["w64"][qi])
    gx = lib.kpconv_gather_backward(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"], padded_grad(G, wf.shape[1]), influence, aggregation)
    held("grad_x", gx, ref["g32"], ref["g64"])
    if aggregation == "closest":
        # the tie's neighbour alone (support 0, at bit-equal distance from kernel points 1 and 2): the first of the two takes it
        lone = torch.full((1, c["idx"].shape[1]), Ns, dtype=torch.long, device=DEV)
        lone[0, 0] = 0
        w1 = lib.kpconv_gather(c["q"][qi:qi + 1].contiguous(), c["s"], lone, c["x"], c["kp"], c["extent"], "constant", "closest")
        assert torch.equal(w1[0, cin:2 * cin], c["x"][0]) and not w1[0, 2 * cin:3 * cin].any() and not w1[0, :cin].any()


# ---- 3. padding columns and strides -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [11, 75], ids=["ld_plus11", "ld_plus75"])
def test_kpconv_padding_columns_and_ld(pad):
    """ld_weighted = K Cin + pad: the padding columns of every row < Nq are written 0, nothing else outside the K Cin values is touched; the backward
    reads K Cin columns of a grad_weighted of that leading dimension.  Its geometry gives every support to exactly one query (29 queries x 17
    private supports), so no two atomics meet and the result does not depend on their order: bit-equal to the tight call."""
    from diffreg_hip import lib
    raw = lib.raw()
    cin, H, K = 65, 17, 15
    c = on_dev(R.kpconv_case(cin, H, K, "mixed"))
    Nq, Ns, KC = c["q"].shape[0], c["s"].shape[0], K * cin
    ld = KC + pad
    tight = lib.kpconv_gather(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"])
    out, check = guarded((Nq + 2, ld), torch.float32, DEV, fill=SENT)
    rc = raw.dr_kpconv_gather_mode_f32(Nq, Ns, H, cin, K, at(c["q"]), at(c["s"]), at(c["idx"]), at(c["x"]), at(c["kp"]), float(c["extent"]), 1, 0, at(out),
                                       ld, stream())
    assert rc == 0
    check()
    assert torch.equal(out[:Nq, :KC], tight[:, :KC])
    assert not out[:Nq, KC:].any() and bool((out[Nq:] == SENT).all())
    # backward on private supports
    nq = 29
    q = c["q"][:nq].contiguous()
    off = R.T(R.synth.hash_uniform(23, pad, (nq, H, 3), -0.5, 0.5).astype(np.float32)).to(DEV) * float(c["radius"])
    s = torch.cat([(q[:, None, :] + off).reshape(-1, 3), c["s"][:Ns - nq * H]], 0).contiguous()
    idx = torch.arange(nq * H, device=DEV).view(nq, H)
    idx[3, 5], idx[nq - 1, H - 1] = -1, Ns + 7
    G = R.T(R.synth.hash_normal(24, pad, (nq, KC)).astype(np.float32)).to(DEV)
    cc = dict(q=q, s=s, idx=idx, x=c["x"], kp=c["kp"], extent=c["extent"])
    ref = kp_refs(cc, G=G)
    g_tight = lib.kpconv_gather_backward(q, s, idx, c["x"], c["kp"], c["extent"], padded_grad(G, (KC + 3) // 4 * 4))
    gx, check = guarded((Ns, cin), torch.float32, DEV, fill=SENT)
    gw = padded_grad(G, ld)
    rc = raw.dr_kpconv_gather_backward_mode_f32(nq, Ns, H, cin, K, at(q), at(s), at(idx), at(c["x"]), at(c["kp"]), float(c["extent"]), 1, 0, at(gw), ld,
                                                at(gx), stream())
    assert rc == 0
    check()
    assert torch.equal(gx, g_tight)
    assert gx[:nq * H].any() and not gx[nq * H:].any()
    held("grad_x, private supports", gx, ref["g32"], ref["g64"])


# ---- 4. refusals without a launch --------------------------------------------------------------------------------------------------------------
def test_kpconv_refusals():
    """Outside its domain the forward entry answers before any launch: H = 65, K = 17, Cin = 513, ld_weighted < K Cin are DR_ENOSUP; extent <= 0,
    influence 3 and a null pointer are DR_EINVAL; `weighted` is untouched.  The backward entry returns the same codes.  The header promises for it
    only that grad_x is "zeroed here"; what a refused call leaves in grad_x is not stated, and today it differs by code: DR_EINVAL is answered before
    anything is enqueued, DR_ENOSUP after the memset of grad_x [Ns, Cin] (launch_kpconv_gather_backward zeroes first).  So only the codes are
    asserted for the backward entry, with a grad_x large enough for either behaviour."""
    from diffreg_hip import lib
    lib.ensure_init()
    raw, E = lib.raw(), codes()
    assert E["DR_OK"] == 0 and E["DR_ENOSUP"] != E["DR_EINVAL"]
    Nq, Ns = 9, 20
    q, s = torch.rand(Nq, 3, device=DEV), torch.rand(Ns, 3, device=DEV)
    idx = torch.zeros(Nq, 65, dtype=torch.long, device=DEV)
    x = torch.ones(Ns, 513, device=DEV)
    kp = torch.zeros(17, 3, device=DEV)
    out, check = guarded((Nq, 17 * 513), torch.float32, DEV, fill=SENT)
    gw = torch.ones(Nq, 17 * 513, device=DEV)
    gx, gcheck = guarded((Ns, 513), torch.float32, DEV, fill=SENT)
    good = dict(H=8, Cin=32, K=15, ext=0.1, inf=1, ld=15 * 32, q=q, s=s)
    bad = [("H65", dict(H=65), "DR_ENOSUP"), ("K17", dict(K=17, ld=17 * 32), "DR_ENOSUP"), ("Cin513", dict(Cin=513, ld=15 * 513), "DR_ENOSUP"),
           ("ld_short", dict(ld=15 * 32 - 1), "DR_ENOSUP"), ("extent0", dict(ext=0.0), "DR_EINVAL"), ("extent_neg", dict(ext=-0.1), "DR_EINVAL"),
           ("influence3", dict(inf=3), "DR_EINVAL"), ("null_q", dict(q=None), "DR_EINVAL"), ("null_s", dict(s=None), "DR_EINVAL")]
    for name, change, code in bad:
        a = dict(good, **change)
        pq, ps = (at(a["q"]) if a["q"] is not None else None), (at(a["s"]) if a["s"] is not None else None)
        rc = raw.dr_kpconv_gather_mode_f32(Nq, Ns, a["H"], a["Cin"], a["K"], pq, ps, at(idx), at(x), at(kp), a["ext"], a["inf"], 0, at(out), a["ld"], stream())
        assert rc == E[code], (name, rc)
        rc = raw.dr_kpconv_gather_backward_mode_f32(Nq, Ns, a["H"], a["Cin"], a["K"], pq, ps, at(idx), at(x), at(kp), a["ext"], a["inf"], 0, at(gw), a["ld"],
                                                    at(gx), stream())
        assert rc == E[code], (name, "backward", rc)
    rc = raw.dr_kpconv_gather_mode_f32(Nq, Ns, 8, 32, 15, at(q), at(s), at(idx), at(x), at(kp), 0.1, 1, 0, None, 15 * 32, stream())
    assert rc == E["DR_EINVAL"]
    check()
    gcheck()
    assert bool((out == SENT).all())


# ---- 5. col_stats / norm_apply / norm_backward: slabs, channel tails, leading dimensions ---------------------------------------------------------
def view_in(src, ld, off=1):
    """src [N, C] as columns off .. off + C - 1 of a sentinel-filled [N, ld] buffer -> (buffer, pointer of the view)"""
    buf = torch.full((src.shape[0], ld), SENT, device=DEV)
    buf[:, off:off + src.shape[1]] = src
    return buf, at(buf, off)


def out_view(N, C, ld, off=1):
    buf, check = guarded((N, ld), torch.float32, DEV, fill=SENT)
    return buf, at(buf, off), check


def around_untouched(buf, C, off=1):
    return bool((buf[:, :off] == SENT).all()) and bool((buf[:, off + C:] == SENT).all())


def raw_stats(lib, ptr_x, N, C, ld):
    raw = lib.raw()
    mean, cm = guarded((C,), torch.float32, DEV, fill=SENT)
    rstd, cr = guarded((C,), torch.float32, DEV, fill=SENT)
    wsb = raw.dr_col_stats_workspace_bytes(N, C)
    ws, cw = guarded((wsb,), torch.uint8, DEV)
    assert raw.dr_col_stats_f32(N, C, ptr_x, ld, at(mean), at(rstd), at(ws), wsb, stream()) == 0
    cm(); cr(); cw()
    return mean, rstd


def run_norm(lib, a, b, G, form, act):
    """the three entries through views of leading dimension C + 3 (a, grad_out) / C + 5 (b, grad_a) / C + 2 (out, grad_b) -> dict of results"""
    raw = lib.raw()
    N, C = a.shape
    has_b, nb = form != "a", form == "ab_norm"
    abuf, pa = view_in(a, C + 3)
    bbuf, pb = view_in(b, C + 5) if has_b else (None, None)
    gbuf, pg = view_in(G, C + 3)
    ma, ra = raw_stats(lib, pa, N, C, C + 3)
    mb, rb = raw_stats(lib, pb, N, C, C + 5) if nb else (None, None)
    obuf, po, ocheck = out_view(N, C, C + 2)
    rc = raw.dr_norm_apply_f32(N, C, pa, C + 3, at(ma), at(ra), pb, C + 5 if has_b else 0, at(mb) if nb else None, at(rb) if nb else None, R.SLOPE,
                               1 if act else 0, po, C + 2, stream())
    assert rc == 0
    ocheck()
    gabuf, pga, gacheck = out_view(N, C, C + 5)
    gbbuf, pgb, gbcheck = out_view(N, C, C + 2) if has_b else (None, None, None)
    wsb = raw.dr_norm_backward_workspace_bytes(N, C)
    ws, wcheck = guarded((wsb,), torch.uint8, DEV)
    rc = raw.dr_norm_backward_f32(N, C, pg, C + 3, po, C + 2, pa, C + 3, at(ma), at(ra), pb, C + 5 if has_b else 0, at(mb) if nb else None,
                                  at(rb) if nb else None, R.SLOPE, 1 if act else 0, pga, C + 5, pgb, C + 2, at(ws), wsb, stream())
    assert rc == 0
    gacheck(); wcheck()
    if has_b:
        gbcheck()
    # nothing around the views moved, and the inputs are as they were
    assert around_untouched(obuf, C) and around_untouched(gabuf, C) and (not has_b or around_untouched(gbbuf, C))
    assert around_untouched(abuf, C) and torch.equal(abuf[:, 1:1 + C], a) and torch.equal(gbuf[:, 1:1 + C], G)
    assert not has_b or (around_untouched(bbuf, C) and torch.equal(bbuf[:, 1:1 + C], b))
    return dict(mean_a=ma, rstd_a=ra, mean_b=mb, rstd_b=rb, out=obuf[:, 1:1 + C], ga=gabuf[:, 1:1 + C], gb=gbbuf[:, 1:1 + C] if has_b else None)


def norm_refs(a, b, G, form, act):
    out = {}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        aa = a.detach().to(dt).clone().requires_grad_(True)
        bb = b.detach().to(dt).clone().requires_grad_(True) if form != "a" else None
        y = R.norm_block64(aa, bb, form, act) if dt == torch.float64 else R.norm_block_torch32(aa, bb, form, act)
        (y * G.to(dt)).sum().backward()
        out["out" + name], out["ga" + name], out["gb" + name] = y.detach(), aa.grad, (bb.grad if bb is not None else None)
    return out


def stats32(x):
    m = x.mean(0)
    return m, 1.0 / torch.sqrt(((x - m) ** 2).mean(0) + R.EPS)


@pytest.mark.parametrize("case", R.NORM_CASES, ids=R.norm_id)
def test_norm_slabs_tails_and_leading_dimensions(case):
    from diffreg_hip import lib
    lib.ensure_init()
    N, C = case
    c = on_dev(R.norm_case(N, C))
    for form, act in R.NORM_COMBOS:
        a, b, G = c["a_" + form], c["b_" + form], c["G"]
        got = run_norm(lib, a, b, G, form, act)
        ref = norm_refs(a, b, G, form, act)
        tag = "%s act=%d " % (form, act)
        _, m64, r64 = R.xhat64(a)
        m32, r32 = stats32(a)
        held(tag + "mean_a", got["mean_a"], m32, m64)
        held(tag + "rstd_a", got["rstd_a"], r32, r64)
        if form == "ab_norm":
            _, m64, r64 = R.xhat64(b)
            m32, r32 = stats32(b)
            held(tag + "mean_b", got["mean_b"], m32, m64)
            held(tag + "rstd_b", got["rstd_b"], r32, r64)
        held(tag + "out", got["out"], ref["out32"], ref["out64"])
        held(tag + "grad_a", got["ga"], ref["ga32"], ref["ga64"])
        if form != "a":
            held(tag + "grad_b", got["gb"], ref["gb32"], ref["gb64"])
        if N == 1 and form == "a":
            # one row, from the definition: xhat = 0, rstd = 1 / sqrt(eps), nothing flows back
            assert torch.equal(got["mean_a"], a[0]) and not got["out"].any() and not got["ga"].any()
            assert bool((got["rstd_a"] == torch.tensor(1.0 / np.sqrt(1e-5), dtype=torch.float64).float().item()).all())
        if case == R.NORM_SPECIAL:
            assert float(got["mean_a"][0]) == 2.5 and float(got["rstd_a"][0]) == float(np.float32(1.0 / np.sqrt(1e-5)))
            held(tag + "out, the column of mean 1e4", got["out"][:, -1], ref["out32"][:, -1], ref["out64"][:, -1])
            held(tag + "grad_a, the column of mean 1e4", got["ga"][:, -1], ref["ga32"][:, -1], ref["ga64"][:, -1])
            held(tag + "grad_a, the constant column", got["ga"][:, 0], ref["ga32"][:, 0], ref["ga64"][:, 0])


# ---- 6. LeakyReLU at exactly zero -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["a", "ab_id"])
def test_leaky_relu_at_exactly_zero_takes_the_slope(form):
    """16 entries whose normalised value is exactly 0 in float32 (columns built from pairs mu +- d around a representable mean; b = 0 there): the
    output is 0 and the gradient passes with the slope, as torch's LeakyReLU backward does (x > 0 ? g : slope g)"""
    from diffreg_hip import lib
    lib.ensure_init()
    c = on_dev(R.leaky_zero_case())
    a, b, G, Z = c["a"], c["b"], c["G"], c["zeros"]
    got = run_norm(lib, a, b, G, form, True)
    assert int((got["out"] == 0).sum()) >= 8 and bool((got["out"][Z] == 0).all()) and int(Z.sum()) == 16
    assert bool((got["mean_a"][:4] == 0.5).all())
    ref = norm_refs(a, b, G, form, True)
    held(form + " out", got["out"], ref["out32"], ref["out64"])
    held(form + " grad_a", got["ga"], ref["ga32"], ref["ga64"])
    held(form + " grad_a at the zeros", got["ga"][Z], ref["ga32"][Z], ref["ga64"][Z])
    if form == "ab_id":
        assert torch.equal(got["gb"][Z], G[Z] * np.float32(R.SLOPE))
        held(form + " grad_b", got["gb"], ref["gb32"], ref["gb64"])


# ---- 7. gather_pool forward and backward -------------------------------------------------------------------------------------------------------
def pool_refs(p, H, first, G):
    out = {}
    fn = R.closest_pool64 if first else R.max_pool64
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        x = p["x"].detach().to(dt).clone().requires_grad_(True)
        y = fn(x, p["inds"][:, :H], dtype=dt)
        (y * G.to(dt)).sum().backward()
        out["y" + name], out["g" + name] = y.detach(), x.grad
    return out


def run_pool(lib, p, H, ld, first, G):
    raw = lib.raw()
    n2, d, n1 = p["inds"].shape[0], p["x"].shape[1], p["n1"]
    out, ocheck = guarded((n2, d), torch.float32, DEV, fill=SENT)
    assert raw.dr_gather_pool_f32(n2, H, ld, d, at(p["x"]), n1, at(p["inds"]), 1 if first else 0, at(out), stream()) == 0
    ocheck()
    gx, gcheck = guarded((n1, d), torch.float32, DEV, fill=SENT)
    assert raw.dr_gather_pool_backward_f32(n2, H, ld, d, at(p["x"]), n1, at(p["inds"]), 1 if first else 0, at(G), at(gx), stream()) == 0
    gcheck()
    return out, gx


@pytest.mark.parametrize("first", [False, True], ids=["max", "closest"])
@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.pool_id)
def test_gather_pool_indices_and_ties(case, first):
    from diffreg_hip import lib
    lib.ensure_init()
    n2, H, d, ld = case
    p = on_dev(R.pool_case(*case))
    ref = pool_refs(p, H, first, p["G"])
    out, gx = run_pool(lib, p, H, ld, first, p["G"])
    assert torch.equal(out, ref["y64"].float())                      # a maximum and a gather are exact
    held("grad_x", gx, ref["g32"], ref["g64"])
    if n2 >= 8:
        inds, n1 = p["inds"][:, :H], p["n1"]
        real = (inds >= 0) & (inds < n1)
        assert not out[(~real).all(1)].any()
        if not first:
            assert bool((out[2] < 0).all()) and not out[3].any() and torch.equal(out[4], out[5])


# ---- 8. kNN interpolation ----------------------------------------------------------------------------------------------------------------------
def knn_refs(c):
    out = {}
    for name, dt in (("64", torch.float64), ("32", torch.float32)):
        x = c["x"].detach().to(dt).clone().requires_grad_(True)
        y = R.knn_interpolate64(c["q"], c["s"], x, c["idx"], dtype=dt)
        (y * c["G"].to(dt)).sum().backward()
        out["y" + name], out["g" + name] = y.detach(), x.grad
    return out


@pytest.mark.parametrize("case", R.KNN_CASES, ids=R.knn_id)
def test_knn_interpolate_channels_lanes_and_shadows(case):
    from diffreg_hip import lib
    C, H = case
    c = on_dev(R.knn_case(C, H))
    Nq, Ns = c["q"].shape[0], c["s"].shape[0]
    ref = knn_refs(c)
    out = lib.knn_interpolate(c["q"], c["s"], c["idx"], c["x"])
    held("out", out, ref["y32"], ref["y64"])
    held("out, queries standing on a support", out[10:20], ref["y32"][10:20], ref["y64"][10:20])
    assert not out[Nq - 3:].any()
    # the out= / col= form: columns 4 .. 4 + C - 1 of a wider buffer, sentinels either side
    wide, check = guarded((Nq, C + 9), torch.float32, DEV, fill=SENT)
    assert lib.knn_interpolate(c["q"], c["s"], c["idx"], c["x"], out=wide, col=4) is wide
    check()
    assert torch.equal(wide[:, 4:4 + C], out) and bool((wide[:, :4] == SENT).all()) and bool((wide[:, 4 + C:] == SENT).all())
    gx = lib.knn_interpolate_backward(c["q"], c["s"], c["idx"], c["G"], C)
    held("grad_x", gx, ref["g32"], ref["g64"])
    gwide = torch.full((Nq, C + 9), SENT, device=DEV)
    gwide[:, 4:4 + C] = c["G"]
    gx2 = lib.knn_interpolate_backward(c["q"], c["s"], c["idx"], gwide, C, col=4)
    d = held("grad_x from a column slice", gx2, ref["g32"], ref["g64"])
    assert R.rel_dev(gx2, gx) <= 4 * d


# ---- 9. two runs ---------------------------------------------------------------------------------------------------------------------------------
def test_two_runs():
    """forward entries are bit-equal over two calls; the backward entries that accumulate with float atomics are held to float64 both times and to
    each other within the same bar"""
    from diffreg_hip import lib
    lib.ensure_init()
    cin, H, K = 129, 33, 15
    c = on_dev(R.kpconv_case(cin, H, K, "mixed"))
    KC = K * cin
    G = upstream(25, (c["q"].shape[0], KC))
    ref = kp_refs(c, G=G)
    f = [lib.kpconv_gather(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"]) for _ in range(2)]
    assert torch.equal(f[0], f[1])
    n = [lib.kpconv_neighbor_count(c["idx"], c["x"], c["s"].shape[0]) for _ in range(2)]
    assert torch.equal(n[0], n[1])
    g = [lib.kpconv_gather_backward(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"], padded_grad(G, f[0].shape[1])) for _ in range(2)]
    d = [held("kpconv grad_x, run %d" % i, g[i], ref["g32"], ref["g64"]) for i in range(2)][0]
    assert R.rel_dev(g[0], g[1]) <= 4 * d
    for first in (False, True):
        case = (300, 17, 96, 20)
        p = on_dev(R.pool_case(*case))
        pr = pool_refs(p, 17, first, p["G"])
        r = [run_pool(lib, p, 17, 20, first, p["G"]) for _ in range(2)]
        assert torch.equal(r[0][0], r[1][0])
        d = [held("pool grad_x (first_only %d), run %d" % (first, i), r[i][1], pr["g32"], pr["g64"]) for i in range(2)][0]
        assert R.rel_dev(r[0][1], r[1][1]) <= 4 * d
    k = on_dev(R.knn_case(65, 3))
    kr = knn_refs(k)
    o = [lib.knn_interpolate(k["q"], k["s"], k["idx"], k["x"]) for _ in range(2)]
    assert torch.equal(o[0], o[1])
    g = [lib.knn_interpolate_backward(k["q"], k["s"], k["idx"], k["G"], 65) for _ in range(2)]
    d = [held("knn grad_x, run %d" % i, g[i], kr["g32"], kr["g64"]) for i in range(2)][0]
    assert R.rel_dev(g[0], g[1]) <= 4 * d
    a = on_dev(R.norm_case(1027, 33))
    s = [run_norm(lib, a["a_ab_norm"], a["b_ab_norm"], a["G"], "ab_norm", True) for _ in range(2)]
    assert all(torch.equal(s[0][key], s[1][key]) for key in ("mean_a", "rstd_a", "out", "ga", "gb"))
