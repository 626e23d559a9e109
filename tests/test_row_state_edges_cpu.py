"""The bars of tests/test_row_state_edges_gpu.py, held to account without a GPU.  Each kernel of csrc/rowops.hip / csrc/stateops.hip that the device
tests compare is restated here on the host, lane by lane and slice by slice, in the kernel's own precision; the restatement goes through the SAME
comparison function as the device's output and must pass, and the restatement with one deliberate error must fail at the shapes named below.
No mutated code is compiled for the GPU.

  LayerNorm, lane predicate c <= C4     C = 260 / 516 / 764 (a lane of the last load reaches one float4 past the row) -- and NOT at C = 256 / 512 /
                                        768, where no lane has such a c: those widths cannot tell the two predicates apart
  LayerNorm, one-pass variance          rows of mean 1e3 and std 1e-2 at any width (E[x^2] - mean^2 cancels)
  pair_min that skips the last slice    1 x 61441 with the minimum in the one-entry slice 15; 600 x 700 with it at (G - 1) per
  Fourier with sin and cos swapped      every shape
  ddim, first-step x - shift in float64 float32 state with a shift at a step of the schedule's middle (1e-7 of the state against a bar of 1e-9;
                                        at the loop's own first step (999, 949) c = 1e-4 hides it)"""
import math

import numpy as np
import pytest
import torch

from tests import test_row_state_edges_gpu as T

f32 = np.float32
LANES = np.arange(64)


def wave(v, op):
    """the xor-shuffle reduction of common.h over the 64 lanes"""
    for m in (32, 16, 8, 4, 2, 1):
        v = op(v, v[LANES ^ m])
    return v[0]


def fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------------
def ln_restated(c, mutant=None):
    """layernorm_kernel / layernorm_vec_kernel on the host buffers of a T.ln_case -> (framed out, framed rowmax)"""
    rows, C, ld, start = c["rows"], c["C"], c["ld"], c["start"]
    x = c["x_raw"].numpy()
    res = None if c["res_raw"] is None else c["res_raw"].numpy()
    g, b = c["gamma"].numpy(), c["beta"].numpy()
    out, rowmax = T.blank(rows, C, ld, c["off"])[0].numpy(), T.blank(1, rows)[0].numpy()
    form = T.ln_form(C, c["layout"])
    W, NV = (4, form) if form else (1, 16)
    CW = C // W
    post, pre = c["res_mode"] == "post", c["res_mode"] == "pre"
    for r in range(rows):
        base = start + r * ld
        loads, s = [], np.zeros(64, f32)
        for i in range(NV):
            cc = LANES + 64 * i
            act = (cc <= CW) if mutant == "lane_le" else (cc < CW)
            idx = np.minimum(base + W * cc[:, None] + np.arange(W)[None, :], x.size - 1)
            v = np.where(act[:, None], x[idx], f32(0))
            if post:
                v = np.where(act[:, None], v + res[idx], v)
            s = s + ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3]) if W == 4 else v[:, 0])
            loads.append((cc, act, idx, v))
        mean = wave(s, np.add) / f32(C)
        s2 = np.zeros(64, f32)                                # the second pass over the registers: what the float32 sum above left of the mean
        for cc, act, idx, v in loads:
            d = np.where(act[:, None], v - mean, f32(0))
            s2 = s2 + ((d[:, 0] + d[:, 1]) + (d[:, 2] + d[:, 3]) if W == 4 else d[:, 0])
        if mutant != "plain_mean":
            mean = mean + wave(s2, np.add) / f32(C)
        q = np.zeros(64, f32)
        for cc, act, idx, v in loads:
            d = v if mutant == "one_pass" else np.where(act[:, None], v - mean, f32(0))
            for w in range(W):
                q = fma32(d[:, w], d[:, w], q)
        var = wave(q, np.add) / f32(C)
        if mutant == "one_pass":
            var = var - mean * mean
        with np.errstate(invalid="ignore"):
            rstd = f32(1) / np.sqrt(f32(var + f32(1e-5)))
        ymax = np.zeros(64, f32)
        for cc, act, idx, v in loads:
            gi = np.minimum(W * cc[:, None] + np.arange(W)[None, :], C - 1)
            y = (v - mean) * rstd * g[gi] + b[gi]
            if pre:
                y = y + res[idx]
            out[idx[act]] = y[act]
            ymax = np.maximum(ymax, np.where(act, np.abs(y).max(1), f32(0)))
        rowmax[T.MARGIN + r] = wave(ymax, np.maximum)
    return torch.from_numpy(out), (None if post else torch.from_numpy(rowmax))


def test_layernorm_rotation_meets_every_form():
    """every row count, residual and layout (the two float4 layouts for the float4 forms, all four for the scalar one) meets every kernel form"""
    seen = {}
    for k, C in enumerate(T.LN_WIDTHS):
        for rows, res, layout in T.ln_rotation(k):
            s = seen.setdefault(T.ln_form(C, layout), (set(), set(), set()))
            s[0].add(rows); s[1].add(res); s[2].add(layout)
    assert sorted(seen) == [0, 1, 2, 3]
    for form, (rows, res, layouts) in seen.items():
        assert rows == set(T.LN_ROWS) and res == set(T.LN_RES), (form, rows, res)
        assert layouts == (set(T.LN_LAYOUTS) if form == 0 else {"contiguous", "ld+4"}), (form, layouts)
    assert [T.ln_form(C, "contiguous") for C in (256, 260, 512, 516, 768, 772, 1024)] == [1, 2, 2, 3, 3, 0, 0]
    assert all(T.ln_form(C, l) == 0 for C in T.LN_PRODUCT_WIDTHS for l in ("ld+1", "offset1"))


LN_SHAPES = [(C, rows, res, layout) for C in (63, 256, 260, 516, 764, 772) for rows, res, layout in ((5, "pre", "contiguous"), (3, "post", "ld+4"))]


@pytest.mark.parametrize("C,rows,res,layout", LN_SHAPES)
def test_layernorm_restatement_passes_and_mutants_fail(C, rows, res, layout):
    for kind in T.LN_KINDS:
        c = T.ln_case(rows, C, res, layout, kind, 77 + C)
        ratio, ulps = T.ln_check(c, *ln_restated(c))
        print("restated LayerNorm C=%d %s %s %s: error / torch float32's %.2f, %.1f float32 ulps" % (C, res, layout, kind, ratio, ulps))
        if kind == "offset":
            with pytest.raises(AssertionError):
                T.ln_check(c, *ln_restated(c, "one_pass"))
        if T.ln_form(C, layout) and C in (260, 516, 764):
            with pytest.raises(AssertionError):
                T.ln_check(c, *ln_restated(c, "lane_le"))
        if C == 256:                                          # no lane of NV = 1 has c == 64: the boundary width itself cannot see this mutant
            assert T.same_bits(ln_restated(c, "lane_le")[0], ln_restated(c)[0])


# ---- Fourier ---------------------------------------------------------------------------------------------------------------------------------
def fourier_restated(p, D, L, ldo, mutant=None):
    rows = p.shape[0]
    emb = T.blank(rows, ldo)[0].numpy()
    body = emb[T.MARGIN:T.MARGIN + rows * ldo].reshape(rows, ldo)
    body[:] = 0.0
    pn = p.numpy()
    body[:, :D] = pn
    for l in range(L):
        th = f32(2.0 ** l) * pn
        s, c = np.sin(th), np.cos(th)
        if mutant == "swap":
            s, c = c, s
        body[:, D + 2 * D * l:D + 2 * D * l + D] = s
        body[:, D + 2 * D * l + D:D + 2 * D * (l + 1)] = c
    return torch.from_numpy(emb)


@pytest.mark.parametrize("D,rows,L,ldo", [(2, 1, 1, 6), (2, 257, 10, 44), (3, 63, 10, 63), (3, 257, 10, 64)])
def test_fourier_restatement_passes_and_swapped_fails(D, rows, L, ldo):
    p = 640.0 * torch.rand(rows, D, generator=T.gen(rows + L))
    st = T.fourier_check(fourier_restated(p, D, L, ldo), p, D, L, ldo)
    print("restated Fourier: %.3e from float64, torch float32 %.3e" % (st["dev"], st["torch"]))
    with pytest.raises(AssertionError):
        T.fourier_check(fourier_restated(p, D, L, ldo, "swap"), p, D, L, ldo)


def test_centring_bar_takes_one_ulp_of_the_mean_and_no_more():
    g = T.gen(3)
    pts, (R, t) = 640.0 * torch.rand(257, 3, generator=g), T.pose(g)
    emu = T.warp_f32(pts, R, t)
    mean = emu.double().mean(0).float()
    T.centred_check(emu - mean, pts, R, t, "exact")
    T.centred_check(emu - torch.nextafter(mean, torch.full((3,), math.inf)), pts, R, t, "one ulp")
    with pytest.raises(AssertionError):
        T.centred_check(emu - torch.nextafter(torch.nextafter(mean, torch.full((3,), math.inf)), torch.full((3,), math.inf)), pts, R, t, "two ulps")
    fused = (R.double() @ pts.double().t()).t().float() + t                      # the product summed in float64: not the stated float32 order
    assert not T.same_bits(fused, emu)
    with pytest.raises(AssertionError):
        T.centred_check(fused - mean, pts, R, t, "another summation order")


# ---- pair_min --------------------------------------------------------------------------------------------------------------------------------
def pair_min_restated(x, N, M, sm=None, tm=None, split=False, mutant=None):
    """pair_min_kernel (split False) / pair_min_split_kernel on a host state [P, N M] -> framed [P] minima"""
    P, NM = x.shape
    out = T.blank(1, P, dtype=torch.float64)[0]
    xs = x if sm is None else x.masked_fill(~(sm[:, :, None] & tm[:, None, :]).reshape(P, NM), math.inf)
    for p in range(P):
        if not split:
            out[T.MARGIN + p] = torch.cat([xs[p], torch.tensor([math.inf], dtype=torch.float64)]).min()
            continue
        G, per, _, _ = T.pm_geometry(NM)
        part = [xs[p, g * per:min(NM, (g + 1) * per)] for g in range(G - 1 if mutant == "skip_last" else G)]
        out[T.MARGIN + p] = min([float(s.min()) if s.numel() else math.inf for s in part] + [math.inf])
    return out


@pytest.mark.parametrize("N,M", [(1, 61441), (600, 700), (512, 513), (128, 128)])
def test_pair_min_restatement_passes_and_skipped_slice_fails(N, M):
    P, NM = 2, N * M
    x = torch.rand(P, NM, generator=T.gen(NM), dtype=torch.float64) + 1.0
    G, per, last, _ = T.pm_geometry(NM)
    caught = []
    for k, pos in enumerate(T.pm_positions(NM)):
        y = x.clone()
        y[k % P, pos] = 0.5
        exp = y.min(1).values
        T.pm_check(pair_min_restated(y, N, M, split=True), P, exp, "restated split")
        T.pm_check(pair_min_restated(y, N, M), P, exp, "restated one workgroup")
        try:
            T.pm_check(pair_min_restated(y, N, M, split=True, mutant="skip_last"), P, exp, "mutant")
        except AssertionError:
            caught.append(pos)
    if last == G - 1:
        assert (G - 1) * per in caught and NM - 1 in caught, caught
    else:                                                     # 512 x 513: slice G - 1 is empty, skipping it changes nothing -- the plants in
        assert caught == []                                   # slice 60 are there for a kernel that mishandles the empty slices behind it
    sm, tm = torch.ones(P, N, dtype=torch.bool), torch.ones(P, M, dtype=torch.bool)
    sm[1] = False
    exp = torch.tensor([float(x[0].min()), math.inf], dtype=torch.float64)
    T.pm_check(pair_min_restated(x, N, M, sm, tm, split=True), P, exp, "restated, a pair with nothing inside its masks")


# ---- ddim ------------------------------------------------------------------------------------------------------------------------------------
def ddim_restated(c, mutant=None):
    """ddim_kernel on the host: numpy scalars of the kernel's own types"""
    P, N, M = c["P"], c["N"], c["M"]
    k = T.ddim_coefficients_host(c["t"], c["tn"])
    x = c["x"].numpy().reshape(P, N * M)
    x0 = c["x0"].numpy().reshape(P, N * M)
    out, _ = T.framed(c["x"].view(P, N * M))
    body = out.numpy()[T.MARGIN:T.MARGIN + P * N * M].reshape(P, N * M)
    for p in range(P):
        xs = x[p]
        if c["shift"] is not None:
            sh = np.float64(c["shift"][p])
            if c["first"] and mutant != "f64_sub":
                xs = (xs.astype(f32) - f32(sh)).astype(np.float64)
            else:
                xs = xs - sh
        eps = (k["sra"] * xs - x0[p].astype(np.float64)) / k["srm1"]
        xn = (x0[p] * f32(k["sqrt_an"])).astype(np.float64) + k["c"] * eps
        if c["xi"] is not None:
            xi = c["xi"].numpy().reshape(P, N * M)[p]
            xn = xn + ((f32(k["sigma"]) * xi).astype(np.float64) if c["first"] else k["sigma"] * xi.astype(np.float64))
        body[p] = np.where(c["valid"][p].numpy().reshape(-1), xn, -np.inf)
    return out


@pytest.mark.parametrize("N,M,P", [(1, 1, 1), (5, 7, 3), (33, 255, 3)])
def test_ddim_restatement_passes_and_float64_subtraction_fails(N, M, P):
    n = 0
    for first in (False, True):
        for shift in (False, True):
            for noise in (False, True):
                for masked in (False, True):
                    n += 1
                    c = T.ddim_case(P, N, M, first, shift, noise, masked, 100 * N + 10 * P + n)
                    with np.errstate(invalid="ignore", over="ignore"):
                        T.ddim_check(c, ddim_restated(c))
                        if first and shift and N * M > 1 and c["t"] < 900:
                            with pytest.raises(AssertionError):
                                T.ddim_check(c, ddim_restated(c, "f64_sub"))
