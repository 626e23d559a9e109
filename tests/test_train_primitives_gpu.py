"""The backward primitives every training path runs on (csrc/train.hip, csrc/attention_bwd.hip), one at a time, against float64 on the CPU at
the edges of their launch geometry: head-dim buckets and their ends, block / wave / grid-stride boundaries, sizes that train (375 x 381,
564 x 629, 1 024 x 1 530), degenerate sizes (1 x 1), per-element different masks, non-default parameters.

Every reference is computed here, in float64, by torch autograd through the DEFINITION of the operation (not through the library and not through
the written-out adjoints of oracle/train_oracle.py); inputs are float32 values cast up, so both sides see the same numbers.  Every output the
library writes lies between guard bands.  The bounds are the ones the suite already asserts for each primitive (tests/test_train_gpu.py,
tests/test_train_branches_gpu.py): the largest absolute error over EVERY entry divided by the largest entry of the float64 reference.

Where a reference gradient vanishes identically (a softmax over ONE key is constant, LayerNorm over ONE channel is constant) the quotient
has no denominator; the error is then measured against the size of the terms that cancel (`floor` of rel_err, stated at each use).

Each test prints its figures ("[fig] ...") before it asserts; run with -s to see them.  Needs a GPU."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch

from diffreg_hip import lib
from oracle import diffreg_oracle as orc
from oracle import train_oracle as tro
from tests.helpers import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NAN = float("nan")


def dev(t):
    return None if t is None else t.to(DEV)


def gen(*key):
    g = torch.Generator()
    g.manual_seed(int(sum((i + 1) * 1000003 ** (i % 3) * int(k) for i, k in enumerate(key)) % (2 ** 31)))
    return g


def rel_err(got, ref, floor=None):
    """max |got - ref| over every entry / max |ref|; when the reference vanishes identically (below 1e-9 of `floor`, the size of the
    terms that cancel in it) the denominator is `floor`"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite entries in the device result"
    err, m = float((got - ref).abs().max()), float(ref.abs().max())
    if floor is not None and m <= 1e-9 * floor:
        m = floor
    return err / m


def fig(what, **figures):
    print("[fig] %s: %s" % (what, "  ".join("%s %.3e" % kv for kv in figures.items())))


def out_bands(*shapes):
    """guarded float32 outputs filled with NaN -> (tensors, check-all)"""
    pairs = [guarded(s, F32, DEV, fill=NAN) for s in shapes]
    return [p[0] for p in pairs], lambda: [p[1]() for p in pairs]


# ================================================================================================================================
# attention forward + backward
# ================================================================================================================================
def attn_masks(B, L, S, g):
    """per batch element different masks; at least one key of every batch element stays live"""
    qm = torch.rand(B, L, generator=g) > 0.2
    km = torch.rand(B, S, generator=g) > 0.3
    for b in range(B):
        km[b, (7 * b + 3) % S] = True
    return qm, km


def attn_inputs(B, L, S, H, d, masked):
    g = gen(B, L, S, H, d)
    C = H * d
    q, k = torch.randn(B, L, C, generator=g), torch.randn(B, S, C, generator=g)
    v, go = torch.randn(B, S, C, generator=g) * 2, torch.randn(B, L, C, generator=g)
    qm, km = attn_masks(B, L, S, g) if masked else (None, None)
    return q, k, v, go, qm, km


def attn_reference(q, k, v, go, H, qm, km, dtype=F64):
    """softmax(q k^T / sqrt(d)) v per head, key j dead for query l when q_mask[l] && !k_mask[j]; -> (out, dq, dk, dv) by autograd in `dtype`"""
    B, L, C = q.shape
    d = C // H
    qd, kd, vd = (t_.to(dtype, copy=True).requires_grad_(True) for t_ in (q, k, v))
    qh, kh, vh = (z.view(B, -1, H, d).transpose(1, 2) for z in (qd, kd, vd))
    logit = qh @ kh.transpose(-1, -2) / d ** 0.5
    if qm is not None:
        logit = logit.masked_fill(qm[:, None, :, None] & ~km[:, None, None, :], float("-inf"))
    out = (torch.softmax(logit, -1) @ vh).transpose(1, 2).reshape(B, L, C)
    gq, gk, gv = torch.autograd.grad(out, (qd, kd, vd), go.to(dtype))
    return out.detach(), gq, gk, gv


def attn_floors(q, k, v, go, H):
    """size of the terms of dS = scale P (dP - delta) that cancel when the reference gradient is identically 0 (S = 1): scale max |dO| . |V|, times
    the largest |k| (dq) or |q| (dk)"""
    B, L, C = q.shape
    d = C // H
    gh, vh = (z.double().abs().view(B, -1, H, d).transpose(1, 2) for z in (go, v))
    t = float((gh @ vh.transpose(-1, -2)).max()) / d ** 0.5
    return t * float(k.abs().max()), t * float(q.abs().max())


# ascending d, so every head-dim bucket of the backward (64 | 96 | 128 | 160) first sees a small d and then a larger one in this process
ATTN_D = [(2, 130, 70, H, d) for d in (4, 16, 64, 68, 96, 100, 124, 128, 132, 156, 160) for H in (1, 4)]
ATTN_LS = [(2, L, S, 4, 108) for L, S in ((1, 1), (1, 200), (200, 1), (31, 33), (32, 32), (33, 31), (64, 97), (129, 128))] + \
          [(2, 564, 629, 4, 64), (2, 1024, 1530, 4, 64)]
ATTN_CASES = [c + (m,) for c in ATTN_D + ATTN_LS for m in (False, True)]
ATTN_BOUND = 1e-5


@pytest.mark.parametrize("B,L,S,H,d,masked", ATTN_CASES, ids=["B%d-L%d-S%d-H%d-d%d-%s" % (c[:5] + ("masked" if c[5] else "full",)) for c in ATTN_CASES])
def test_attention_forward_and_backward(B, L, S, H, d, masked):
    """dr_attention_f32 / dr_attention_backward_f32 at every head-dim bucket and its two ends (d <= 64 | 96 | 128 | 160), L or S of 1, below / at / past
    the 32-row blocks, fewer other-blocks than waves, and the sizes that train.  out, dq, dk, dv <= 1e-5 of the float64 maximum; two calls are
    bit-identical."""
    q, k, v, go, qm, km = attn_inputs(B, L, S, H, d, masked)
    ref, gq, gk, gv = attn_reference(q, k, v, go, H, qm, km)
    (out, dq, dk, dv), chk = out_bands(q.shape, q.shape, k.shape, v.shape)
    lib.attention(dev(q), dev(k), dev(v), H, dev(qm), dev(km), out=out)
    lib.attention_backward(dev(q), dev(k), dev(v), out, dev(go), H, dev(qm), dev(km), out=(dq, dk, dv))
    chk()
    fq, fk = attn_floors(q, k, v, go, H)
    e = dict(out=rel_err(out, ref), dq=rel_err(dq, gq, fq), dk=rel_err(dk, gk, fk), dv=rel_err(dv, gv))
    fig("attention B%d L%d S%d H%d d%d %s" % (B, L, S, H, d, "masked" if masked else "full"), **e)
    for nm, x in e.items():
        assert x < ATTN_BOUND, (nm, x)
    dq2, dk2, dv2 = lib.attention_backward(dev(q), dev(k), dev(v), out, dev(go), H, dev(qm), dev(km))
    assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)          # fixed summation orders: bit-reproducible


@pytest.mark.parametrize("masked", [False, True])
def test_attention_row_stride_beyond_the_heads(masked):
    """ld > H d: q, k, v are column slices of one [rows, 3 C] buffer (the raw ABI; the wrapper would copy them), out / grad_o / the three gradients
    columns C .. 2 C - 1 of [rows, 3 C] buffers of their own.  Same bounds; the other columns of every written buffer come back untouched."""
    B, L, H, d = 2, 130, 4, 108
    S, C = L, H * d
    ld = 3 * C
    q, k, v, go, qm, km = attn_inputs(B, L, S, H, d, masked)
    ref, gq, gk, gv = attn_reference(q, k, v, go, H, qm, km)
    qkv = dev(torch.cat([q, k, v], 2).reshape(B * L, ld).contiguous())
    SENT = 12345.0
    (O, GO, DQ, DK, DV), chk = out_bands(*[(B * L, ld)] * 5)
    for t_ in (O, GO, DQ, DK, DV):
        t_.fill_(SENT)
    GO[:, C:2 * C] = dev(go.reshape(B * L, C))
    at = lambda t_, col: ctypes.c_void_p(t_.data_ptr() + 4 * col)
    mq, mk = lib.mask_u8(dev(qm)), lib.mask_u8(dev(km))
    lib.ensure_init()
    scale = 1.0 / d ** 0.5
    wsb = lib.raw().dr_attention_backward_workspace_bytes(B, H, L)
    ws, chk_ws = guarded((wsb,), torch.uint8, DEV)

    def run():
        lib.check(lib.raw().dr_attention_f32(B, H, L, S, d, at(qkv, 0), at(qkv, C), at(qkv, 2 * C), ld, lib.ptr(mq), lib.ptr(mk), scale, at(O, C), lib.stream_of(qkv)))
        lib.check(lib.raw().dr_attention_backward_f32(B, H, L, S, d, at(qkv, 0), at(qkv, C), at(qkv, 2 * C), at(O, C), at(GO, C), ld, lib.ptr(mq), lib.ptr(mk),
                                                      scale, at(DQ, C), at(DK, C), at(DV, C), lib.ptr(ws), wsb, lib.stream_of(qkv)))
        torch.cuda.synchronize()
    run()
    chk(); chk_ws()
    cut = lambda t_: t_[:, C:2 * C].reshape(B, L, C)
    e = dict(out=rel_err(cut(O), ref), dq=rel_err(cut(DQ), gq), dk=rel_err(cut(DK), gk), dv=rel_err(cut(DV), gv))
    fig("attention ld = 3 C, %s" % ("masked" if masked else "full"), **e)
    for nm, x in e.items():
        assert x < ATTN_BOUND, (nm, x)
    for t_ in (O, DQ, DK, DV):
        assert bool((t_[:, :C] == SENT).all()) and bool((t_[:, 2 * C:] == SENT).all()), "padding columns written"
    first = [cut(t_).clone() for t_ in (DQ, DK, DV)]
    run()
    assert all(torch.equal(a, cut(b)) for a, b in zip(first, (DQ, DK, DV)))


# ================================================================================================================================
# Sinkhorn backward
# ================================================================================================================================
SK_CASES = [(2, 375, 381, 3, 1.0), (2, 564, 629, 3, 1.0), (2, 1024, 1530, 3, 0.5), (3, 3, 63, 1, 1.0), (2, 15, 64, 5, 2.0), (1, 1, 1, 3, 1.0),
            (4, 63, 255, 3, 1.0), (1, 256, 256, 2, -0.7)]
SK_ID = lambda c: "P%d-%dx%d-T%d-a%g" % c


def sk_inputs(P, N, M, masked):
    """seeded randn x 3 scores, randn upstream gradient; masked: pair b loses its last 3 b rows and 5 b columns (entries under a mask are -inf, as
    the matching head hands them over)"""
    g = gen(P, N, M, 77)
    sc, gc = torch.randn(P, N, M, generator=g) * 3, torch.randn(P, N, M, generator=g)
    nb = torch.arange(P)[:, None]
    sm = torch.arange(N)[None] < (N - 3 * nb if masked else N + 0 * nb)
    tm = torch.arange(M)[None] < (M - 5 * nb if masked else M + 0 * nb)
    if masked:
        sc = sc.masked_fill(~(sm[:, :, None] & tm[:, None, :]), float("-inf"))
    return sc, gc, sm, tm


def sk_dustbin_l1(sc, a, iters, sm, tm, gc):
    """sum |dL/dZ| over the dustbin row and column of the extended matrix Z (float64): the scale of grad_bin_score's rounding error (the value itself is
    their signed sum and may cancel).  The recurrences of matching.py:61-93 with Z as the leaf; -> (L1, dL/dZ[:, :N, :M] to hold against the oracle's)"""
    B, N, M = sc.shape
    Z = torch.full((B, N + 1, M + 1), float(a), dtype=F64)
    Z[:, :N, :M] = sc
    Z.requires_grad_(True)
    rows, cols = sm.sum(1, keepdim=True), tm.sum(1, keepdim=True)
    nu0 = -(rows + cols).log()                                                   # float32 marginals (quirk Q22), promoted on use
    log_mu = torch.cat([nu0.expand(B, N), cols.log() + nu0], 1)
    log_nu = torch.cat([nu0.expand(B, M), rows.log() + nu0], 1)
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v[:, None, :], dim=2)
        v = log_nu - torch.logsumexp(Z + u[:, :, None], dim=1)
    conf = (Z + u[:, :, None] + v[:, None, :] - nu0[:, :, None]).exp()[:, :-1, :-1]
    gZ, = torch.autograd.grad((conf * gc).sum(), Z)
    return float(gZ[:, :N, M].abs().sum() + gZ[:, N, :].abs().sum()), gZ[:, :N, :M]


def sk_reference_pair(sc, gc, sm, tm, iters, a, dtype=F64):
    """one pair: autograd through oracle.diffreg_oracle.sinkhorn_log(...).exp()[:, :-1, :-1] -> (grad_scores [1,N,M], grad_bin_score)"""
    s = sc.to(dtype, copy=True).requires_grad_(True)
    al = torch.tensor(a, dtype=dtype, requires_grad=True)
    conf = orc.sinkhorn_log(s, al, iters, sm, tm).exp()[:, :-1, :-1]
    gs, ga = torch.autograd.grad((conf * gc.to(dtype)).sum(), (s, al))
    return gs, ga


@functools.lru_cache(maxsize=None)
def sk_reference(case, masked):
    """-> (inputs, float64 grad_scores [P,N,M], grad_bin_score per pair [P], dustbin L1 per pair [P]); one pair at a time (the pairs of a batch
    are independent problems)"""
    P, N, M, iters, a = case
    a = float(np.float32(a))
    sc, gc, sm, tm = sk_inputs(P, N, M, masked)
    gs, ga, l1 = [], [], []
    for b in range(P):
        sl = slice(b, b + 1)
        g1, a1 = sk_reference_pair(sc[sl], gc[sl], sm[sl], tm[sl], iters, a)
        s1, gz = sk_dustbin_l1(sc[sl].double(), a, iters, sm[sl], tm[sl], gc[sl].double())
        assert float((gz - g1).abs().max()) <= 1e-12 * max(float(g1.abs().max()), 1e-300)      # the two float64 evaluations are one function
        gs.append(g1); ga.append(a1); l1.append(s1)
    gs, ga = torch.cat(gs), torch.stack(ga)
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(ga).all())
    return (sc, gc, sm, tm, a), gs, ga, torch.tensor(l1, dtype=F64)


def sk_check(case, masked, what):
    P, N, M, iters, _ = case
    (sc, gc, sm, tm, a), gs_ref, ga_ref, l1 = sk_reference(case, masked)
    (gs, ga), chk = out_bands((P, N, M), (P,))
    total = lib.sinkhorn_backward(dev(sc), torch.tensor(a), iters, dev(sm) if masked else None, dev(tm) if masked else None, dev(gc), out=(gs, ga))[1]
    chk()
    e_s = rel_err(gs, gs_ref)
    e_a = (ga.double().cpu() - ga_ref).abs()
    fig("%s %s %s" % (what, SK_ID(case), "masked" if masked else "full"), grad_scores=e_s, grad_bin_over_l1=float((e_a / l1).max()),
        grad_bin_abs=float(e_a.max()), dustbin_l1=float(l1.max()))
    assert e_s < 1e-4, e_s
    assert bool((e_a <= 1e-4 * l1 + 1e-7).all()), (e_a, l1)                                  # every pair on its own
    assert abs(float(total) - float(ga_ref.sum())) <= 1e-4 * float(l1.sum()) + 1e-7 * P
    if masked:
        assert float(gs[~dev(sm[:, :, None] & tm[:, None, :])].abs().sum()) == 0.0           # entries under a mask: exactly 0
    return gs, ga


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", SK_CASES, ids=SK_ID)
def test_sinkhorn_backward(case, masked):
    """dr_sinkhorn_backward_f32 (the multi-launch form the library runs) at the sizes that train, iters = 1 (no v-adjoint launch), iters > 3, P > 2,
    N + 1 / M + 1 on the 4-row / 64-column block edges, fewer rows than row parts, per-pair different masks, bin_score != 1.
    grad_scores <= 1e-4 of the float64 maximum; grad_bin_score of EVERY pair within 1e-4 of the L1 norm of the dustbin entries it sums (+ 1e-7)."""
    gs, ga = sk_check(case, masked, "sinkhorn_backward")
    P, N, M, iters, a = case
    sc, gc, sm, tm = sk_inputs(P, N, M, masked)
    gs2, _ = lib.sinkhorn_backward(dev(sc), torch.tensor(float(np.float32(a))), iters, dev(sm) if masked else None, dev(tm) if masked else None, dev(gc))
    assert torch.equal(gs, gs2)                                                              # fixed summation orders


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", [c for c in SK_CASES if c[1] <= 375], ids=SK_ID)
def test_sinkhorn_backward_single_workgroup_form(case, masked):
    """the single-workgroup kernel the source keeps as the multi-launch form's reference (diagnostics knob DR_SKB_ONE_WG): held to the same float64
    values with the same bounds -- a diagnostic reference that is wrong is worse than none"""
    lib.ensure_init()
    lib.raw().dr_debug_enable_env(1)
    os.environ["DR_SKB_ONE_WG"] = "1"
    try:
        sk_check(case, masked, "sinkhorn_backward (one workgroup)")
    finally:
        os.environ.pop("DR_SKB_ONE_WG")
        lib.raw().dr_debug_enable_env(1 if os.environ.get("DR_DIAGNOSTICS") == "1" else 0)


# ================================================================================================================================
# LayerNorm forward + backward
# ================================================================================================================================
LN_CASES = [(r, c, "plain") for r, c in ((1, 432), (3, 64), (5, 1), (777, 432), (1024, 256), (1025, 256), (1128, 432), (2500, 528), (4100, 33), (300, 2048))] + \
           [(1128, 432, "scaled"), (777, 432, "constant row")]


def ln_inputs(rows, C, kind):
    g = gen(rows, C, 5)
    x = torch.randn(rows, C, generator=g)
    if kind == "scaled":                                     # row r times 10^(-3 .. +3): six orders of magnitude over the rows
        x = x * (10.0 ** torch.linspace(-3, 3, rows))[:, None]
    if kind == "constant row":                               # variance 0: y = beta, the gradient scales with 1 / sqrt(eps).  (0.75 C sums exactly in
        x[rows // 2] = 0.75                                  # float32, so the row's mean is exact on both sides and the case is the variance-0 path itself)
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    gy = torch.randn(rows, C, generator=g)
    return x, gam, bet, gy


def ln_reference(x, gam, bet, gy, eps=1e-5, dtype=F64):
    xd, gd, bd = (t_.to(dtype, copy=True).requires_grad_(True) for t_ in (x, gam, bet))
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (xd - mean) * rstd * gd + bd
    gx, gg, gb = torch.autograd.grad(y, (xd, gd, bd), gy.to(dtype))
    return y.detach(), gx, gg, gb, rstd.detach()


@pytest.mark.parametrize("rows,C,kind", LN_CASES)
def test_layernorm_forward_and_backward(rows, C, kind):
    """dr_layernorm_f32 / dr_layernorm_backward_f32: fewer rows than a workgroup's four waves, the backward's grid-stride loop on its first trip only
    (1 024 rows), one row into its second (1 025), well into it (4 100), C below / off / at multiples of the 64 lanes, C = 2 048 (the documented
    maximum: 64 KiB of dynamic LDS), rows of six orders of magnitude, a row of variance 0.  y within 2e-5 (of the row's maximum where the rows are
    scaled); grad_x, grad_gamma, grad_beta <= 1e-4 of their float64 maximum on every entry."""
    x, gam, bet, gy = ln_inputs(rows, C, kind)
    y_ref, gx_ref, gg_ref, gb_ref, rstd = ln_reference(x, gam, bet, gy)
    (y, st, gx, gg, gb), chk = out_bands((rows, C), (rows, 2), (rows, C), (C,), (C,))
    lib.layernorm(dev(x), dev(gam), dev(bet), out=(y, st))
    lib.layernorm_backward(dev(x), dev(gam), st, dev(gy), out=(gx, gg, gb))
    chk()
    assert bool(torch.isfinite(y).all())
    row_err = (y.double().cpu() - y_ref).abs().max(1).values
    e_y = float((row_err / y_ref.abs().max(1).values).max()) if kind == "scaled" else float(row_err.max())
    # C = 1: xhat = 0, so grad_x and grad_gamma vanish identically; the terms that cancel are rstd g gy and sum_rows |gy|
    f_x = float((gy.double().abs() * gam.double().abs() * rstd).max())
    f_g = float(gy.double().abs().sum(0).max()) * math.sqrt(C)
    e = dict(y=e_y, gx=rel_err(gx, gx_ref, f_x), ggamma=rel_err(gg, gg_ref, f_g), gbeta=rel_err(gb, gb_ref))
    fig("layernorm %d x %d %s" % (rows, C, kind), **e)
    assert e["y"] < 2e-5, e
    assert e["gx"] < 1e-4 and e["ggamma"] < 1e-4 and e["gbeta"] < 1e-4, e


# ================================================================================================================================
# masked row softmax + backward
# ================================================================================================================================
SM_CASES = [(1, 1, 1, 1), (2, 4, 50, 70), (3, 2, 33, 64), (1, 4, 7, 63), (2, 4, 129, 629)]


def softmax_reference(sc, dP, scale, qm, km, dtype=F64):
    s = sc.to(dtype, copy=True).requires_grad_(True)
    a = s
    if qm is not None:
        a = a.masked_fill(qm[:, None, :, None] & ~km[:, None, None, :], float("-inf"))
    P = torch.softmax(a * scale, dim=3)
    dS, = torch.autograd.grad(P, s, dP.to(dtype))
    return P.detach(), dS


@pytest.mark.parametrize("mag,scale", [(1.0, 0.3), (80.0, 1.0)])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,H,L,S", SM_CASES)
def test_softmax_rows_and_backward(B, H, L, S, masked, mag, scale):
    """dr_softmax_rows_f32 / dr_softmax_backward_f32: one key, fewer keys than lanes, exactly 64, a row count off the four waves of a workgroup, per
    batch element different masks, scores of magnitude 80 at scale 1 (the subtraction of the row maximum matters).  P within 1e-6, dS <= 1e-5 of
    its float64 maximum."""
    g = gen(B, H, L, S, int(mag))
    sc, dP = torch.randn(B, H, L, S, generator=g) * mag, torch.randn(B, H, L, S, generator=g)
    qm, km = attn_masks(B, L, S, g) if masked else (None, None)
    P_ref, dS_ref = softmax_reference(sc, dP, scale, qm, km)
    (P, dS), chk = out_bands(sc.shape, sc.shape)
    lib.softmax_rows(dev(sc), scale, dev(qm), dev(km), out=P)
    lib.softmax_backward(P, dev(dP), scale, out=dS)
    chk()
    assert bool(torch.isfinite(P).all())
    # S = 1: P = 1 and dS vanishes identically; the terms that cancel are scale P dP
    e = dict(P=float((P.double().cpu() - P_ref).abs().max()), dS=rel_err(dS, dS_ref, scale * float(dP.abs().max())))
    fig("softmax %s %s mag %g scale %g" % ((B, H, L, S), "masked" if masked else "full", mag, scale), **e)
    assert e["P"] < 1e-6 and e["dS"] < 1e-5, e
    if masked:
        dead = (qm[:, None, :, None] & ~km[:, None, None, :]).expand(B, H, L, S)
        assert float(P.cpu()[dead].abs().sum()) == 0.0 and float(dS.cpu()[dead].abs().sum()) == 0.0


# ================================================================================================================================
# dual softmax + backward
# ================================================================================================================================
DS_CASES = [(1, 1, 1), (2, 70, 90), (3, 64, 257), (1, 300, 600), (2, 564, 629)]
# conf of six cases misses the suite's 1e-6 on the device, and so does plain float32: the same function through torch in float32 on the CPU against its
# float64 value (the "floor").  The cause is the format, not the kernel: x = sim / T is rounded to float32 (half an ulp of |x| <= 14 at T = 0.7 is
# 4.8e-7, of |x| <= 80 at T = 0.1 it is 3.8e-6), that error is a RELATIVE error of both softmax factors, and these sizes have entries of conf near 1.
# For exactly these cases the bound is 4 x the measured floor (the floor is within a factor of 4 of 1e-6); every other case keeps 1e-6.
#   (P, N, M, masked, T): float32 CPU floor            device error measured on an MI355X
DS_CONF_FLOOR = {(1, 300, 600, False, 0.1): 1.679e-6,  # 1.649e-6
                 (1, 300, 600, True, 0.1): 1.679e-6,   # 1.649e-6
                 (2, 564, 629, False, 0.1): 1.450e-6,  # 1.450e-6
                 (2, 564, 629, True, 0.1): 1.450e-6,   # 1.450e-6
                 (2, 564, 629, False, 0.7): 1.329e-6,  # 1.329e-6
                 (2, 564, 629, True, 0.7): 1.377e-6}   # 1.436e-6


def dual_softmax_reference(sim, g, T, sm, tm, dtype=F64):
    s = sim.to(dtype, copy=True).requires_grad_(True)
    s1 = s2 = s / T
    if sm is not None:
        s1 = s1.masked_fill(~sm[:, :, None], float("-inf"))
        s2 = s2.masked_fill(~tm[:, None, :], float("-inf"))
    conf = torch.softmax(s1, 1) * torch.softmax(s2, 2)
    gs, = torch.autograd.grad(conf, s, g.to(dtype))
    return conf.detach(), gs


@pytest.mark.parametrize("T", [0.1, 0.7])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("P,N,M", DS_CASES)
def test_dual_softmax_and_backward(P, N, M, masked, T):
    """dr_dual_softmax_f32 / dr_dual_softmax_backward_f32: one pair and three, a second column block (M > 256: one column past it, and several blocks),
    the sizes that train, per-pair different masks (pair b loses 3 (b + 1) rows and 5 (b + 1) columns, one of each always stays), two temperatures.
    conf within 1e-6 (4 x the float32 floor on the six cases of DS_CONF_FLOOR, where float32 itself misses 1e-6), grad_sim <= 2e-6 of its float64
    maximum."""
    g = gen(P, N, M, 9)
    sim, gc = torch.randn(P, N, M, generator=g) * 2, torch.randn(P, N, M, generator=g)
    sm = tm = None
    if masked:
        nb = torch.arange(P)[:, None] + 1
        sm = torch.arange(N)[None] < (N - 3 * nb).clamp(min=1)
        tm = torch.arange(M)[None] < (M - 5 * nb).clamp(min=1)
    T32 = float(np.float32(T))                                                     # the library takes the temperature as a float32
    conf_ref, gs_ref = dual_softmax_reference(sim, gc, T32, sm, tm)
    (conf, gs), chk = out_bands(sim.shape, sim.shape)
    lib.dual_softmax(dev(sim), T, dev(sm), dev(tm), out=conf)
    lib.dual_softmax_backward(dev(sim), T, dev(sm), dev(tm), dev(gc), out=gs)
    chk()
    assert bool(torch.isfinite(conf).all())
    # N = M = 1: conf = 1 and grad_sim vanishes identically; the terms that cancel are g conf / T
    e = dict(conf=float((conf.double().cpu() - conf_ref).abs().max()), grad_sim=rel_err(gs, gs_ref, float(gc.abs().max()) / T32))
    fig("dual softmax %s %s T %g" % ((P, N, M), "masked" if masked else "full", T), **e)
    conf_bound = 4.0 * DS_CONF_FLOOR[(P, N, M, masked, T)] if (P, N, M, masked, T) in DS_CONF_FLOOR else 1e-6
    assert e["conf"] < conf_bound and e["grad_sim"] < 2e-6, (e, conf_bound)
    if masked:
        live = (sm[:, :, None] & tm[:, None, :])
        assert float(conf.cpu()[~live].abs().sum()) == 0.0 and float(gs.cpu()[~live].abs().sum()) == 0.0


# ================================================================================================================================
# rotary position code
# ================================================================================================================================
@pytest.mark.parametrize("unit_scale", [True, False])
@pytest.mark.parametrize("rows,C", [(1, 2), (37, 432), (1000, 528)])
def test_rotary_forward_and_inverse(rows, C, unit_scale):
    """dr_rotary_f32: out = R(+-theta) x scale on the channel pairs (2 k, 2 k + 1), against float64.  An output is two float32 products, their sum
    and the product with scale: at most 2 ulp of (|x_2k| + |x_2k+1|) scale, held at 4 x 2^-24 of it per entry.  inverse(forward(x)) = x scale^2 to
    float32 rounding: both passes' roundings and cos^2 + sin^2 of float32 tables, held at 8 x 2^-24 of the same magnitude."""
    g = gen(rows, C, 3)
    x = torch.randn(rows, C, generator=g)
    th = torch.rand(rows, C // 2, generator=g) * 200.0 - 100.0
    cs, sn = th.cos(), th.sin()
    scale = 1.0 if unit_scale else float(np.float32(1.0 / math.sqrt(C)))
    xe, xo, c64, s64 = x[:, 0::2].double(), x[:, 1::2].double(), cs.double(), sn.double()
    mag = torch.stack([xe.abs() + xo.abs()] * 2, -1).reshape(rows, C)
    eps = 2.0 ** -24

    def ref(sign):
        return torch.stack([(xe * c64 - xo * sign * s64) * scale, (xo * c64 + xe * sign * s64) * scale], -1).reshape(rows, C)
    (fw, inv, back), chk = out_bands(x.shape, x.shape, x.shape)
    lib.rotary(dev(x), dev(cs), dev(sn), scale=scale, out=fw)
    lib.rotary(dev(x), dev(cs), dev(sn), inverse=True, scale=scale, out=inv)
    lib.rotary(fw, dev(cs), dev(sn), inverse=True, scale=scale, out=back)
    chk()
    e_f = float(((fw.double().cpu() - ref(1.0)).abs() / (mag * scale)).max()) / eps
    e_i = float(((inv.double().cpu() - ref(-1.0)).abs() / (mag * scale)).max()) / eps
    e_b = float(((back.double().cpu() - x.double() * scale * scale).abs() / (mag * scale * scale)).max()) / eps
    fig("rotary %d x %d scale %g (in units of 2^-24 of the pair's magnitude)" % (rows, C, scale), forward=e_f, inverse=e_i, round_trip=e_b)
    assert e_f <= 4.0 and e_i <= 4.0 and e_b <= 8.0, (e_f, e_i, e_b)


# ================================================================================================================================
# ReLU backward
# ================================================================================================================================
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_relu_backward(n):
    """dr_relu_backward_f32 at the 256-thread block edges, with exact +0.0 and -0.0 planted in y (first, last and every 97th entry): bit-equal to
    where(y > 0, g, 0)"""
    g = gen(n, 1)
    y, gy = torch.randn(n, generator=g), torch.randn(n, generator=g)
    y[::97] = 0.0
    y[48::97] = -0.0
    y[-1] = -0.0 if n > 1 else 0.0
    (out,), chk = out_bands((n,))
    lib.relu_backward(dev(y), dev(gy), out=out)
    chk()
    assert torch.equal(out.cpu(), torch.where(y > 0, gy, torch.zeros_like(gy)))


# ================================================================================================================================
# focal loss backward
# ================================================================================================================================
FOCAL_EDGES = [0.0, 5e-7, 1e-6, 1.0 - 1e-6, 1.0 - 5e-7, 1.0]


@pytest.mark.parametrize("batch", ["mixed", "no positive", "no negative"])
@pytest.mark.parametrize("gamma,alpha,pw,nw", [(2.0, 0.25, 1.0, 1.0), (1.5, 0.4, 0.7, 2.0)])
def test_focal_loss_backward(gamma, alpha, pw, nw, batch):
    """dr_focal_loss_backward_f32 with the default and a second parameter set, conf planted at and around both clamp edges (on a positive and on a
    negative entry), a batch without positives and one without negatives, against oracle.train_oracle.focal_loss_backward (the definition: the
    clamp makes autograd awkward) evaluated in float64 on the same float32 values.  <= 2e-6 of the float64 maximum over every entry (the bound of
    test_matching_head_backward_against_reference_autograd), and the same over the entries away from the clamp (conf in [0.01, 0.99]) on their own
    maximum -- the planted entries next to conf = 1e-6 carry gradients 1e4 times everything else and would hide the rest."""
    P, N, M = 2, 40, 56
    g = gen(P, N, M, 21)
    conf = torch.rand(P, N, M, generator=g)
    gt = (torch.rand(P, N, M, generator=g) < 0.02).float()
    if batch == "no positive":
        gt.zero_()
    if batch == "no negative":
        gt.fill_(1.0)
    k = len(FOCAL_EDGES)
    conf[0, 0, :k] = torch.tensor(FOCAL_EDGES, dtype=F64).float()
    conf[1, 3, :k] = torch.tensor(FOCAL_EDGES, dtype=F64).float()
    if batch == "mixed":
        gt[0, 0, :k] = 1.0
        gt[1, 3, :k] = 0.0
    ref = tro.focal_loss_backward(conf.double(), gt.double(), alpha=alpha, gamma=gamma, pos_w=pw, neg_w=nw)
    (got,), chk = out_bands((P, N, M))
    lib.focal_loss_backward(dev(conf), dev(gt), alpha=alpha, gamma=gamma, pos_w=pw, neg_w=nw, out=got)
    chk()
    mid = (conf >= 0.01) & (conf <= 0.99)
    e = dict(all=rel_err(got, ref), inner=rel_err(got.cpu()[mid], ref[mid]))
    fig("focal backward gamma %g alpha %g w %g / %g, %s" % (gamma, alpha, pw, nw, batch), **e)
    assert e["all"] <= 2e-6 and e["inner"] <= 2e-6, e
    dead = (conf < float(np.float32(1e-6))) | (conf > float(np.float32(1.0) - np.float32(1e-6)))
    assert int(dead.sum()) >= 4 and float(got.cpu()[dead].abs().sum()) == 0.0               # outside the clamp: no gradient at all
