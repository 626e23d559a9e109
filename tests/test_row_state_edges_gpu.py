"""The row and state kernels the denoise loops launch between their GEMMs (csrc/rowops.hip, csrc/stateops.hip), kernel by kernel, against plain
float64 statements written out below, at the shapes where their lane, slice and dtype arithmetic changes.  Needs a GPU.  The kernels are reached
through the diagnostics of include/diffreg_hip_debug.h (dr_debug_layernorm_f32, dr_debug_fourier_f32, dr_debug_pair_min_f64, dr_debug_ddim_f64,
dr_debug_state_map) and the two exported entries dr_vol_pe_f32 / dr_scatter_rows_f32.

Every output lives in a NaN-filled buffer with a margin on both sides: nothing outside [rows, C] may change, the padding between C and the leading
dimension included.  Every input's padding is NaN as well, so a lane that reads past its row poisons the row.

The bars
  LayerNorm      max |y - y64| over the call <= 2 x the same of torch.nn.functional.layer_norm in float32 on the same input; a row may always be
                 4 float32 ulps of its max |y64| off (torch is exact on constant rows); rowmax == max |y| of the kernel's own row, exactly.
  sin / cos      the angle (2^l p, or (p - o) / voxel * f) is formed exactly as the kernel states it in float32; the reference is float64 sin / cos
                 of that float32 angle; |dev - ref| <= max(4 x 2^-24, 2 x the deviation of torch's float32 sin / cos on the same angles).
  warp           R p + t in float32 in the kernel's stated order is bit exact; the centring may use a mean one float32 ulp off.
  pair_min, scatter_rows, the conversions     exact.
  ddim           1e-9 absolute on x_next, the bar tests/test_teacher_forced_gpu.py applies, against its ddim_expected.
  sigmoid        4 float64 ulps of torch.sigmoid's value.

Measured on the MI355X (printed by the tests; `python -m pytest -s`):
  LayerNorm, worst call of every form: device error / torch float32's error, and the device's error in float32 ulps of the row's max |y|
                         standard normal     mean 1e3, std 1e-2     constant row
    scalar form          1.75   3.2 ulps     1.04   31900 ulps      1.00   0.5 ulps
    float4, NV = 1       1.01   2.1          1.06   15648           1.00   0.5
    float4, NV = 2       1.76   2.7          1.05   16957           1.00   0.5
    float4, NV = 3       1.58   2.7          0.99   15862           1.00   0.5
    (the 1e4 ulps of the second kind are the float32 mean's own half ulp of 1e3 times rstd = 100: torch's figure is the same.  Before the mean's
    second pass in csrc/rowops.hip the kernel was 2 .. 10 x torch's error there, and 1e-4 instead of 0 on constant rows.)
  sin / cos, worst |dev - float64| and torch float32's on the same angles: Fourier 2-D 6.2e-8 / 3.6e-8, Fourier 3-D 6.8e-8 / 3.6e-8, vol_pe
    6.8e-8 / 3.6e-8 (bar 2.4e-7); ddim: x_next at most 3.6e-15 from the reference's arithmetic (bar 1e-9).
  pair_min slice geometry asserted below: 512 x 513 -> G = 64 slices of per = 4352, slices 61..63 empty, the last non-empty one (60) holds 1536
  entries; 1 x 61441 -> G = 16, per = 4096, slice 15 holds one entry; 128 x 128 -> G = 4, per = 4096 (the threshold itself).

tests/test_row_state_edges_cpu.py holds the bars to account without a GPU: restatements of the kernels on the host pass them, and restatements
with one deliberate error each (lane predicate c <= C4, one-pass variance, last slice skipped, sin and cos swapped, first-step subtraction in
float64) fail them at the shapes named there."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import diffreg_oracle as orc
from tests.conftest import ROOT
from tests.test_teacher_forced_gpu import ddim_expected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 64                       # elements of NaN on either side of every buffer (256 bytes of float32: keeps the 16-byte alignment)
NAN = float("nan")
F32_EPS = 2.0 ** -24
DDIM_TOL = 1e-9                   # tests/test_teacher_forced_gpu.py: the device's next state against ddim_expected on its own x_start


def codes():
    """the return codes, read from the public header"""
    text = open(os.path.join(ROOT, "include", "diffreg_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(DR_[A-Z_]+)\s+\(?(-?\d+)\)?", text)}


@pytest.fixture(scope="module")
def lib():
    from diffreg_hip import lib as L
    L.ensure_init()
    return L


def at(t, off=0):
    """device pointer of element `off` of a tensor"""
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


# ---- sentinel buffers ------------------------------------------------------------------------------------------------------------------------
def framed(body, ld=None, off=0, dtype=None):
    """host buffer [MARGIN | off | rows x ld | MARGIN] of NaN holding `body` ([rows, C], C <= ld) -> (flat tensor, index of element [0, 0])"""
    body = torch.as_tensor(body)
    rows, C = body.shape
    ld = C if ld is None else ld
    raw = torch.full((MARGIN + off + rows * ld + MARGIN,), NAN, dtype=dtype or body.dtype)
    raw[MARGIN + off:MARGIN + off + rows * ld].view(rows, ld)[:, :C] = body
    return raw, MARGIN + off


def blank(rows, C, ld=None, off=0, dtype=torch.float32):
    ld = C if ld is None else ld
    return torch.full((MARGIN + off + rows * ld + MARGIN,), NAN, dtype=dtype), MARGIN + off


def unframed(raw, start, rows, C, ld=None, what=""):
    """-> the [rows, C] body of a (host copy of a) framed buffer, after asserting that every element outside it is still NaN"""
    raw = torch.as_tensor(raw).cpu()
    ld = C if ld is None else ld
    body = raw[start:start + rows * ld].view(rows, ld)
    assert bool(torch.isnan(raw[:start]).all()), (what, "written in front of the buffer")
    assert bool(torch.isnan(raw[start + rows * ld:]).all()), (what, "written behind the buffer")
    assert bool(torch.isnan(body[:, C:]).all()), (what, "written into the padding between C and the leading dimension")
    return body[:, :C].clone()


def same_bits(a, b):
    a, b = torch.as_tensor(a).contiguous(), torch.as_tensor(b).contiguous()
    iv = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(iv), b.view(iv))


# ==============================================================================================================================================
# 1. LayerNorm with residual
# ==============================================================================================================================================
LN_WIDTHS = [1, 4, 63, 65, 252, 256, 260, 430, 432, 508, 512, 516, 528, 764, 768, 772, 1020, 1024]
LN_ROWS = [1, 3, 4, 5, 131]                    # four rows per workgroup
LN_RES = ["none", "pre", "post"]
LN_LAYOUTS = ["contiguous", "ld+4", "ld+1", "offset1"]      # the last two must take the scalar form
LN_KINDS = ["normal", "offset", "const"]       # standard normal; mean 1e3 with std 1e-2; a constant row
LN_PRODUCT_WIDTHS = [260, 516, 772]


def ln_layout(C, layout):
    """-> (leading dimension, offset of the base pointer in floats)"""
    return {"contiguous": (C, 0), "ld+4": (C + 4, 0), "ld+1": (C + 1, 0), "offset1": (C, 1)}[layout]


def ln_form(C, layout):
    """the kernel form the launch rule of csrc/rowops.hip chooses: 0 the scalar form, NV = 1 / 2 / 3 the float4 form with NV loads per lane"""
    ld, off = ln_layout(C, layout)
    if C % 4 or ld % 4 or off % 4 or C > 768:
        return 0
    return (C + 255) // 256


def ln_rotation(k):
    """the (rows, residual, layout) choices the k-th width of LN_WIDTHS is run with: one per row count, residual and layout rotated against it so
    that every choice meets every kernel form (asserted by tests/test_row_state_edges_cpu.py)"""
    return [(LN_ROWS[j], LN_RES[(k + j) % 3], LN_LAYOUTS[(k // 2 + j) % 4]) for j in range(5)]


def ln_case(rows, C, res_mode, layout, kind, seed):
    """host buffers and both references of one LayerNorm call"""
    g = gen(seed)
    if kind == "normal":
        x = torch.randn(rows, C, generator=g)
    elif kind == "offset":
        x = 1e3 + 1e-2 * torch.randn(rows, C, generator=g)
    else:
        x = (0.5 + torch.rand(rows, 1, generator=g)).expand(rows, C).contiguous()
    gamma, beta = 1.0 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    res = None
    if res_mode != "none":
        res = torch.randn(rows, C, generator=g)
        if kind == "const" and res_mode == "post":            # the normalised row x + res is the constant one
            res = torch.rand(rows, 1, generator=g).expand(rows, C).contiguous()
    ld, off = ln_layout(C, layout)

    def ref(dt):
        xx, rr = x.to(dt), None if res is None else res.to(dt)
        if res_mode == "post":
            return orc.layer_norm(xx + rr, gamma.to(dt), beta.to(dt))
        y = orc.layer_norm(xx, gamma.to(dt), beta.to(dt))
        return y if rr is None else y + rr
    c = dict(rows=rows, C=C, res_mode=res_mode, layout=layout, kind=kind, ld=ld, off=off, gamma=gamma, beta=beta, y64=ref(torch.float64), y32=ref(torch.float32))
    c["x_raw"], c["start"] = framed(x, ld, off)
    c["res_raw"] = None if res is None else framed(res, ld, off)[0]
    return c


def ln_check(c, out_raw, rowmax_raw=None):
    """the LayerNorm bar on a framed output (the device's, or a host restatement's) -> (worst row's error / torch float32's error, worst error in
    float32 ulps of max |y|)"""
    rows, C = c["rows"], c["C"]
    what = "LayerNorm C=%d rows=%d %s %s %s" % (C, rows, c["res_mode"], c["layout"], c["kind"])
    y = unframed(out_raw, c["start"], rows, C, c["ld"], what)
    assert bool(torch.isfinite(y).all()), (what, "non-finite output")
    y64 = c["y64"]
    e_dev = (y.double() - y64).abs().amax(1)
    e_t32 = (c["y32"].double() - y64).abs().amax(1)
    ulp = torch.from_numpy(np.spacing(y64.abs().amax(1).float().numpy())).double()
    bar = torch.clamp(4.0 * ulp, min=2.0 * float(e_t32.max()))       # twice torch's maximum error over the call; per row never below 4 ulps
    worst = int((e_dev - bar).argmax())
    assert bool((e_dev <= bar).all()), (what, "row %d: device %.3e from float64, torch float32 %.3e at worst, bar %.3e" % (worst, e_dev[worst], e_t32.max(), bar[worst]))
    if rowmax_raw is not None:
        rm = unframed(rowmax_raw, MARGIN, 1, rows, what=what + " rowmax")[0]
        assert same_bits(rm, y.abs().amax(1)), (what, "rowmax is not max |y| of the row")
    return float(e_dev.max() / e_t32.max()) if float(e_t32.max()) > 0 else 0.0, float((e_dev / ulp).max())


def ln_device(lib, c, want_rowmax):
    rows, C, ld = c["rows"], c["C"], c["ld"]
    x, out = c["x_raw"].to(DEV), blank(rows, C, ld, c["off"])[0].to(DEV)
    res = None if c["res_raw"] is None else c["res_raw"].to(DEV)
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    rm = blank(1, rows)[0].to(DEV) if want_rowmax else None
    rc = lib.raw().dr_debug_layernorm_f32(rows, C, at(x, c["start"]), ld, at(gamma), at(beta), at(res, c["start"]) if res is not None else None, ld,
                                          1 if c["res_mode"] == "post" else 0, at(out, c["start"]), ld, at(rm, MARGIN) if want_rowmax else None, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu(), (rm.cpu() if want_rowmax else None)


def ln_run(lib, C, combos, seed, stats):
    for n, (rows, res_mode, layout) in enumerate(combos):
        for kind in LN_KINDS:
            c = ln_case(rows, C, res_mode, layout, kind, seed + 7 * n)
            want_rowmax = res_mode != "post"              # the post-add launch has no rowmax output
            out, rm = ln_device(lib, c, want_rowmax)
            ratio, ulps = ln_check(c, out, rm)
            s = stats.setdefault((ln_form(C, layout), kind), [0.0, 0.0])
            s[0], s[1] = max(s[0], ratio), max(s[1], ulps)


def ln_report(what, stats):
    for (form, kind), (ratio, ulps) in sorted(stats.items()):
        print("%s: form %s, %-6s rows: device / torch float32 error <= %.2f, device error <= %.1f float32 ulps of max|y|"
              % (what, "scalar" if form == 0 else "float4 NV=%d" % form, kind, ratio, ulps))


@pytest.mark.parametrize("C", LN_WIDTHS)
def test_layernorm_every_width(lib, C):
    stats = {}
    ln_run(lib, C, ln_rotation(LN_WIDTHS.index(C)), 1000 + C, stats)
    ln_report("LayerNorm C=%d" % C, stats)


@pytest.mark.parametrize("C", LN_PRODUCT_WIDTHS)
def test_layernorm_rows_residual_layout_product(lib, C):
    stats = {}
    ln_run(lib, C, [(r, m, l) for r in LN_ROWS for m in LN_RES for l in LN_LAYOUTS], 5000 + C, stats)
    ln_report("LayerNorm product C=%d" % C, stats)


def test_layernorm_refusals_write_nothing(lib):
    rc, k = lib.raw().dr_debug_layernorm_f32, codes()
    C, rows = 1025, 3                                       # buffers are large enough for the call that is refused
    x, out = torch.randn(rows * C + 8, device=DEV), blank(rows, C)[0].to(DEV)
    g, b, rm = torch.ones(C, device=DEV), torch.zeros(C, device=DEV), blank(1, rows)[0].to(DEV)
    o, r = at(out, MARGIN), at(rm, MARGIN)
    assert rc(rows, 1025, at(x), C, at(g), at(b), None, 0, 0, o, C, r, stream()) == k["DR_ENOSUP"]
    assert rc(rows, 1025, at(x), C, at(g), at(b), at(x), C, 1, o, C, None, stream()) == k["DR_ENOSUP"]
    assert rc(rows, 512, at(x), C, at(g), at(b), at(x), C, 1, o, C, r, stream()) == k["DR_EINVAL"]       # post-add with a rowmax output
    assert rc(rows, 512, at(x), C, at(g), at(b), None, 0, 1, o, C, None, stream()) == k["DR_EINVAL"]     # post-add without a residual
    assert rc(rows, 512, at(x), 511, at(g), at(b), None, 0, 0, o, C, None, stream()) == k["DR_EINVAL"]   # ldx < C
    assert rc(rows, 512, at(x), C, at(g), at(b), None, 0, 0, o, 511, None, stream()) == k["DR_EINVAL"]   # ldo < C
    assert rc(rows, 512, at(x), C, at(g), at(b), at(x), 511, 0, o, C, None, stream()) == k["DR_EINVAL"]  # ldres < C
    assert rc(-1, 512, at(x), C, at(g), at(b), None, 0, 0, o, C, None, stream()) == k["DR_EINVAL"]
    assert rc(rows, 0, at(x), C, at(g), at(b), None, 0, 0, o, C, None, stream()) == k["DR_EINVAL"]
    for hole in range(4):
        p = [at(x), at(g), at(b), o]
        p[hole] = None
        assert rc(rows, 512, p[0], C, p[1], p[2], None, 0, 0, p[3], C, None, stream()) == k["DR_EINVAL"]
    assert rc(0, 512, at(x), C, at(g), at(b), None, 0, 0, o, C, r, stream()) == 0                       # no rows: nothing to do
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(rm).all())


# ==============================================================================================================================================
# 2. Fourier embedding and the warp + centring in front of it; the volumetric rotary tables
# ==============================================================================================================================================
def warp_f32(p, R, t):
    """R p + t in float32 in the kernels' stated order: three products, added left to right, then + t (p [n, 3], R [3, 3], t [3])"""
    cols = []
    for a in range(3):
        acc = R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]
        acc = acc + R[a, 2] * p[:, 2]
        cols.append(acc + t[a])
    return torch.stack(cols, 1)


def sincos_bar(ang32, what, stats):
    """-> (float64 sin, float64 cos, bar) of float32 angles: the larger of 4 x 2^-24 and twice torch's own float32 deviation on these angles"""
    a64 = ang32.double()
    s64, c64 = torch.sin(a64), torch.cos(a64)
    dev_t = max(float((torch.sin(ang32).double() - s64).abs().max()), float((torch.cos(ang32).double() - c64).abs().max())) if ang32.numel() else 0.0
    stats["torch"] = max(stats.get("torch", 0.0), dev_t)
    return s64, c64, max(4.0 * F32_EPS, 2.0 * dev_t)


def fourier_check(emb_raw, p, D, L, ldo, stats=None):
    """the Fourier bar on a framed [rows, ldo] embedding of the float32 points p [rows, D] (the device's, or a host restatement's)"""
    stats = {} if stats is None else stats
    rows, W = p.shape[0], (2 * L + 1) * D
    what = "Fourier D=%d rows=%d L=%d ldo=%d" % (D, rows, L, ldo)
    emb = unframed(emb_raw, MARGIN, rows, ldo, what=what)           # the kernel owns all ldo columns: the padding ones are zeros
    assert same_bits(emb[:, :D], p), (what, "the pass-through columns are not the input")
    assert same_bits(emb[:, W:], torch.zeros(rows, ldo - W)), (what, "padding columns are not +0")
    if L == 0:
        return stats
    fac = (2.0 ** torch.arange(L, dtype=torch.float32)).view(1, L, 1)
    ang = fac * p.view(rows, 1, D)                                   # exact: a power of two times a float32
    s64, c64, bar = sincos_bar(ang, what, stats)
    got = emb[:, D:W].reshape(rows, L, 2, D).double()
    e = max(float((got[:, :, 0] - s64).abs().max()), float((got[:, :, 1] - c64).abs().max()))
    stats["dev"] = max(stats.get("dev", 0.0), e)
    assert e <= bar, (what, "sin / cos %.3e from float64, bar %.3e" % (e, bar))
    return stats


def centred_check(ws, pts, R, t, what):
    """warped_ws [n, 3] against the float32 warp minus the float32 of the float64 mean: bit exact for a mean at most one float32 ulp off"""
    emu = pts if R is None else warp_f32(pts, R, t)
    mean = emu.double().mean(0).float()
    for a in range(3):
        cands = [mean[a], torch.nextafter(mean[a], torch.tensor(math.inf)), torch.nextafter(mean[a], torch.tensor(-math.inf))]
        assert any(same_bits(ws[:, a], emu[:, a] - m) for m in cands), (what, "axis %d: not the float32 warp minus the pair's mean" % a)


def pose(g):
    """a rotation (float32 of a float64 orthonormal matrix) and a translation of pixel-range size"""
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    return q.float().contiguous(), (50.0 * torch.randn(3, generator=g)).contiguous()


@pytest.mark.parametrize("rows", [1, 255, 257])
@pytest.mark.parametrize("L", [1, 10])
def test_fourier2d(lib, rows, L):
    stats = {}
    for pad in (0, 2):
        ldo = (2 * L + 1) * 2 + pad
        p = 640.0 * torch.rand(rows, 2, generator=gen(rows * 31 + L))            # pixel range: level-9 angles reach 3e5
        emb = blank(rows, ldo)[0].to(DEV)
        pd = framed(p)[0].to(DEV)
        assert lib.raw().dr_debug_fourier_f32(2, 1, rows, at(pd, MARGIN), None, None, L, at(emb, MARGIN), ldo, None, stream()) == 0
        torch.cuda.synchronize()
        fourier_check(emb, p, 2, L, ldo, stats)
    print("Fourier 2-D rows=%d L=%d: sin / cos %.3e from float64, torch float32 %.3e" % (rows, L, stats.get("dev", 0.0), stats.get("torch", 0.0)))


@pytest.mark.parametrize("rpp", [1, 63, 256, 257, 1000])
@pytest.mark.parametrize("P", [1, 3])
def test_fourier3d_warp_and_centring(lib, P, rpp):
    L, stats = 10, {}
    for warped in (False, True):
        for ldo in (63, 64):
            g = gen(P * 1009 + rpp * 3 + ldo + int(warped))
            pts = 640.0 * torch.rand(P, rpp, 3, generator=g)
            poses = [pose(g) for _ in range(P)]
            Rd = torch.stack([q[0] for q in poses]).to(DEV) if warped else None
            td = torch.stack([q[1] for q in poses]).to(DEV) if warped else None
            n = P * rpp
            emb, ws = blank(n, ldo)[0].to(DEV), blank(n, 3)[0].to(DEV)
            pd = framed(pts.view(n, 3))[0].to(DEV)
            rc = lib.raw().dr_debug_fourier_f32(3, P, rpp, at(pd, MARGIN), at(Rd) if warped else None, at(td) if warped else None, L,
                                                at(emb, MARGIN), ldo, at(ws, MARGIN), stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            what = "Fourier 3-D P=%d rows_per_pair=%d ldo=%d warped=%s" % (P, rpp, ldo, warped)
            w = unframed(ws, MARGIN, n, 3, what=what)
            for pi in range(P):
                centred_check(w[pi * rpp:(pi + 1) * rpp], pts[pi], poses[pi][0] if warped else None, poses[pi][1] if warped else None, what)
            fourier_check(emb, w, 3, L, ldo, stats)                  # the embedding of the device's own centred points
    print("Fourier 3-D P=%d rows_per_pair=%d: sin / cos %.3e from float64, torch float32 %.3e" % (P, rpp, stats["dev"], stats["torch"]))


def test_fourier_refusals_write_nothing(lib):
    rc, k = lib.raw().dr_debug_fourier_f32, codes()
    rows, L = 5, 10
    p, emb, ws = torch.rand(rows * 3 + 8, device=DEV), blank(rows, 64)[0].to(DEV), blank(rows, 3)[0].to(DEV)
    Rt = torch.eye(3, device=DEV).contiguous()
    e, w = at(emb, MARGIN), at(ws, MARGIN)
    assert rc(3, 1, rows, at(p), None, None, L, e, 62, w, stream()) == k["DR_EINVAL"]            # ldo one short
    assert rc(2, 1, rows, at(p), None, None, L, e, 41, None, stream()) == k["DR_EINVAL"]
    assert rc(4, 1, rows, at(p), None, None, L, e, 84, w, stream()) == k["DR_EINVAL"]            # D
    assert rc(1, 1, rows, at(p), None, None, L, e, 64, w, stream()) == k["DR_EINVAL"]
    assert rc(3, 1, rows, at(p), at(Rt), None, L, e, 64, w, stream()) == k["DR_EINVAL"]          # R without t
    assert rc(3, 1, rows, at(p), None, None, L, e, 64, None, stream()) == k["DR_EINVAL"]         # no place for the warped points
    assert rc(3, 1, rows, None, None, None, L, e, 64, w, stream()) == k["DR_EINVAL"]
    assert rc(3, 1, rows, at(p), None, None, L, None, 64, w, stream()) == k["DR_EINVAL"]
    assert rc(3, -1, rows, at(p), None, None, L, e, 64, w, stream()) == k["DR_EINVAL"]
    assert rc(3, 1, -1, at(p), None, None, L, e, 64, w, stream()) == k["DR_EINVAL"]
    assert rc(3, 1, rows, at(p), None, None, -1, e, 64, w, stream()) == k["DR_EINVAL"]
    assert rc(3, 0, rows, at(p), None, None, L, e, 64, w, stream()) == 0 and rc(2, 1, 0, at(p), None, None, L, e, 64, None, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(emb).all()) and bool(torch.isnan(ws).all())


VOL_ORIGIN, VOL_VOXEL = (-1.5, 0.25, 3.0), 0.08


def vol_freq(C):
    d = C // 3
    return torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * (-math.log(10000.0) / d))


@pytest.mark.parametrize("C", [6, 132, 432, 528])
@pytest.mark.parametrize("rows", [1, 7, 257])
def test_vol_pe(lib, rows, C):
    half, nf, stats = C // 2, C // 6, {}
    freq = vol_freq(C)
    for rpp in sorted({1, 3, 100, rows}):                   # pairs of 1 / 3 / 100 rows (a last pair that is cut short) and one pair of all rows
        for warped in (False, True):
            g = gen(rows * 7 + C + rpp + int(warped))
            xyz = 2.0 * torch.randn(rows, 3, generator=g)
            npair = (rows + rpp - 1) // rpp
            poses = [pose(g) for _ in range(npair)]
            poses = [(q[0], 0.02 * q[1]) for q in poses]                          # translations of scene size
            cosd, sind = blank(rows, half)[0].to(DEV), blank(rows, half)[0].to(DEV)
            xd, fd = framed(xyz)[0].to(DEV), framed(freq.view(1, nf))[0].to(DEV)
            Rd = torch.stack([q[0] for q in poses]).to(DEV) if warped else None
            td = torch.stack([q[1] for q in poses]).to(DEV) if warped else None
            rc = lib.raw().dr_vol_pe_f32(rows, rpp, C, at(xd, MARGIN), at(Rd) if warped else None, at(td) if warped else None, VOL_ORIGIN[0],
                                         VOL_ORIGIN[1], VOL_ORIGIN[2], VOL_VOXEL, at(fd, MARGIN), at(cosd, MARGIN), at(sind, MARGIN), stream())
            assert rc == 0, rc
            torch.cuda.synchronize()
            what = "vol_pe rows=%d C=%d rows_per_pair=%d warped=%s" % (rows, C, rpp, warped)
            p = xyz if not warped else torch.cat([warp_f32(xyz[i * rpp:(i + 1) * rpp], *poses[i]) for i in range(npair)])
            vox = (p - torch.tensor(VOL_ORIGIN, dtype=torch.float32)) / torch.tensor(VOL_VOXEL, dtype=torch.float32)
            ang = (vox.view(rows, 3, 1) * freq.view(1, 1, nf)).reshape(rows, half)        # entry (axis a, frequency k) at a * (C / 6) + k
            s64, c64, bar = sincos_bar(ang, what, stats)
            ec = float((unframed(cosd, MARGIN, rows, half, what=what).double() - c64).abs().max())
            es = float((unframed(sind, MARGIN, rows, half, what=what).double() - s64).abs().max())
            stats["dev"] = max(stats.get("dev", 0.0), ec, es)
            assert ec <= bar and es <= bar, (what, ec, es, bar)
    print("vol_pe rows=%d C=%d: sin / cos %.3e from float64, torch float32 %.3e" % (rows, C, stats["dev"], stats["torch"]))


def test_vol_pe_refuses_a_width_off_six(lib):
    rows = 4
    xyz, fr = torch.randn(rows, 3, device=DEV), torch.ones(8, device=DEV)
    cosd, sind = blank(rows, 8)[0].to(DEV), blank(rows, 8)[0].to(DEV)
    rc = lib.raw().dr_vol_pe_f32(rows, rows, 8, at(xyz), None, None, 0.0, 0.0, 0.0, 0.08, at(fr), at(cosd, MARGIN), at(sind, MARGIN), stream())
    assert rc == codes()["DR_ENOSUP"]
    torch.cuda.synchronize()
    assert bool(torch.isnan(cosd).all()) and bool(torch.isnan(sind).all())


# ==============================================================================================================================================
# 3. scatter_rows
# ==============================================================================================================================================
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def scatter_expected(src, sidx, didx, n_dst, C):
    """dst[didx[i]] = src[sidx[i]] under torch's index rule: negative indices wrap once, anything else out of range is skipped and flagged"""
    n_src = src.shape[0]
    dst, flag = torch.full((n_dst, C), NAN), 0
    for s, d in zip(sidx.tolist(), didx.tolist()):
        s, d = (s + n_src if s < 0 else s), (d + n_dst if d < 0 else d)
        if 0 <= s < n_src and 0 <= d < n_dst:
            dst[d] = src[s]
        else:
            flag = 1
    return dst, flag


def scatter_device(lib, src, sidx, didx, n_dst, C, with_status=True):
    n = sidx.numel()
    dst = blank(n_dst, C)[0].to(DEV)
    st = torch.full((MARGIN * 2 + 1,), 0, dtype=torch.int32, device=DEV)
    sd, si, di = src.to(DEV).contiguous(), sidx.to(DEV), didx.to(DEV)
    if n == 0:
        si = di = torch.zeros(1, dtype=torch.int64, device=DEV)       # the entry wants non-NULL index pointers even when it reads none
    rc = lib.raw().dr_scatter_rows_f32(n, C, at(sd), src.shape[0], at(si), at(di), at(dst, MARGIN), n_dst, at(st, MARGIN) if with_status else None,
                                       stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    stc = st.cpu()
    assert int(stc.abs().sum()) == int(stc[MARGIN]), "status written outside its word"
    return dst, int(stc[MARGIN])


@pytest.mark.parametrize("C", [1, 63, 64, 65, 432])
def test_scatter_rows(lib, C):
    for n in (0, 1, 3, 4, 5, 1000):
        g = gen(C * 13 + n)
        n_src, n_dst = n + 3, n + 9
        src = torch.randn(n_src, C, generator=g)
        sidx = torch.randint(0, n_src, (n,), generator=g)
        didx = (1 + torch.randperm(n_dst - 2, generator=g))[:n]       # distinct destination rows out of 1 .. n_dst - 2; the others keep the sentinel
        sidx[1::3] -= n_src                                           # negative indices in [-rows, -1] wrap once
        didx[::2] -= n_dst
        if n >= 5:
            sidx[0], didx[0] = -n_src, -n_dst                         # the lowest index that still wraps (row 0) ...
            sidx[2], didx[2] = n_src - 1, n_dst - 1                   # ... and the highest that is in range
            sidx[4] = sidx[3] + n_src if sidx[3] < 0 else sidx[3] - n_src    # a duplicate destination, from the same source row: the other
            didx[4] = didx[3] + n_dst if didx[3] < 0 else didx[3] - n_dst    # spelling of the same two indices
        what = "scatter_rows C=%d n=%d" % (C, n)
        exp, flag = scatter_expected(src, sidx, didx, n_dst, C)
        assert flag == 0
        dst, st = scatter_device(lib, src, sidx, didx, n_dst, C)
        assert st == 0 and same_bits(unframed(dst, MARGIN, n_dst, C, what=what), exp), what
        if n < 4:
            continue
        # indices out of range: skipped and flagged, every other row still lands -- with and without a status word
        bad = [("src", [(1, n_src)]), ("src", [(n - 1, -n_src - 1)]), ("src", [(0, I64_MAX), (3, I64_MIN)]),
               ("dst", [(0, n_dst)]), ("dst", [(n - 1, -n_dst - 1)]), ("dst", [(2, I64_MIN), (3, I64_MAX)])]
        for side, edits in bad:
            s2, d2 = sidx.clone(), didx.clone()
            for i, v in edits:
                (s2 if side == "src" else d2)[i] = v
            exp, flag = scatter_expected(src, s2, d2, n_dst, C)
            assert flag == 1
            for with_status in (True, False):
                dst, st = scatter_device(lib, src, s2, d2, n_dst, C, with_status)
                assert st == (1 if with_status else 0) and same_bits(unframed(dst, MARGIN, n_dst, C, what=what), exp), (what, side, edits)


# ==============================================================================================================================================
# 4. pair_min: one workgroup per pair, and G slices per pair with the last arrival reducing them
# ==============================================================================================================================================
PM_G, PM_SLICE, PM_SPLIT_MIN_NM, PM_SPLIT_MAX_P = 64, 4096, 16384, 32
PM_SPLIT_SHAPES = [(128, 128), (127, 129 + 1), (241, 255), (512, 513), (600, 700)]


def pm_geometry(NM):
    """the slice rule of csrc/stateops.hip: G = min(64, ceil(NM / 4096)) slices of `per` entries, per = ceil(NM / G) rounded up to 256
    -> (G, per, index of the last non-empty slice, its length)"""
    G = min(PM_G, (NM + PM_SLICE - 1) // PM_SLICE)
    per = ((NM + G - 1) // G + 255) // 256 * 256
    last = (NM - 1) // per
    return G, per, last, NM - last * per


def pm_positions(NM):
    """where the minimum is planted in turn: both ends, both sides of the first slice boundary, the first entry of the last slice of the rule (of
    the last non-empty one where that slice is empty), and the last entry's slice start"""
    G, per, last, _ = pm_geometry(NM)
    return sorted({0, NM - 1, min(per - 1, NM - 1), min(per, NM - 1), min((G - 1) * per, last * per), last * per})


def pm_check(out_raw, P, expected, what):
    """the pair_min bar: a minimum has no rounding, so the framed [P] output equals the float64 reference bit for bit"""
    got = unframed(out_raw, MARGIN, 1, P, what=what)[0]
    assert same_bits(got, expected), (what, got.tolist()[:4], expected.tolist()[:4])


def pm_scratch(lib, P):
    """-> (framed byte buffer, start, bytes): the scratch of P pairs with zeroed arrival counters between two bands of 0xA5"""
    nb = int(lib.raw().dr_debug_pair_min_scratch_bytes(P))
    raw = torch.full((256 + nb + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    raw[256 + nb - 64 * P:256 + nb] = 0
    return raw, 256, nb


def pm_scratch_check(raw, start, nb, P, what):
    h = raw.cpu()
    assert bool((h[:start] == 0xA5).all()) and bool((h[start + nb:] == 0xA5).all()), (what, "written outside the scratch")
    assert not bool(h[start + nb - 64 * P:start + nb].any()), (what, "the arrival counters are not left at zero")


def pm_call(lib, x, P, N, M, sm=None, tm=None, scratch=None):
    out = blank(1, P, dtype=torch.float64)[0].to(DEV)
    rc = lib.raw().dr_debug_pair_min_f64(P, N, M, at(x), at(sm) if sm is not None else None, at(tm) if tm is not None else None, at(out, MARGIN),
                                         at(scratch[0], scratch[1]) if scratch is not None else None, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def pm_state(P, NM, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.rand(P, NM, generator=g, device=DEV, dtype=torch.float64) + 1.0          # every entry in [1, 2): a planted 0.5 / 0.25 is the minimum


def test_pair_min_slice_geometry():
    """the shapes below hit what they are chosen for (pure arithmetic on the documented rule)"""
    G, per, last, n_last = pm_geometry(512 * 513)
    assert (G, per, last, n_last) == (64, 4352, 60, 1536) and last < G - 1                 # slices 61..63 start beyond NM: empty
    assert pm_geometry(61441) == (16, 4096, 15, 1)                                        # a last slice of one entry
    assert pm_geometry(128 * 128) == (4, 4096, 3, 4096) and 128 * 128 == PM_SPLIT_MIN_NM   # the threshold itself, slices exactly full
    assert pm_geometry(600 * 700)[:2] == (64, 6656) and pm_geometry(127 * 130)[0] == 5 and pm_geometry(241 * 255)[0] == 16
    assert 60 * 4352 in pm_positions(512 * 513) and 61440 in pm_positions(61441)


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("NM", [1, 63, 1023, 1025, 16383])
def test_pair_min_one_workgroup(lib, NM, P):
    x = pm_state(P, NM, NM + P)
    base = x.cpu().min(1).values
    pm_check(pm_call(lib, x, P, 1, NM), P, base, "pair_min NM=%d P=%d" % (NM, P))
    for k, pos in enumerate(sorted({0, NM - 1, NM // 2, min(1023, NM - 1), min(1024, NM - 1)})):
        y, exp = x.clone(), base.clone()
        y[k % P, pos] = exp[k % P] = 0.5
        pm_check(pm_call(lib, y, P, 1, NM), P, exp, "pair_min NM=%d P=%d, minimum at %d" % (NM, P, pos))


@pytest.mark.parametrize("P", [1, 2, 32])
@pytest.mark.parametrize("N,M", PM_SPLIT_SHAPES + [(1, 61441)])
def test_pair_min_split(lib, N, M, P):
    NM = N * M
    assert NM >= PM_SPLIT_MIN_NM and P <= PM_SPLIT_MAX_P
    x = pm_state(P, NM, NM + P)
    base = x.cpu().min(1).values
    scratch = pm_scratch(lib, P)
    what = "pair_min split %d x %d P=%d" % (N, M, P)
    pm_check(pm_call(lib, x, P, N, M, scratch=scratch), P, base, what)
    pm_scratch_check(*scratch, P, what)
    for k, pos in enumerate(pm_positions(NM)):
        pair = k % P
        old = float(x[pair, pos])
        x[pair, pos] = 0.5                                            # consecutive calls on the same scratch, different data each time
        exp = base.clone()
        exp[pair] = 0.5
        pm_check(pm_call(lib, x, P, N, M, scratch=scratch), P, exp, what + ", minimum at %d" % pos)
        pm_check(pm_call(lib, x, P, N, M), P, exp, what + ", minimum at %d, one workgroup" % pos)
        x[pair, pos] = old
    pm_scratch_check(*scratch, P, what)


def test_pair_min_beyond_32_pairs_takes_one_workgroup_with_scratch(lib):
    P, N, M = 33, 128, 128
    x = pm_state(P, N * M, 33)
    x[32, N * M - 1] = 0.5
    scratch = pm_scratch(lib, P)
    pm_check(pm_call(lib, x, P, N, M, scratch=scratch), P, x.cpu().min(1).values, "pair_min P=33 with scratch")
    h = scratch[0].cpu()
    assert bool((h[256:256 + scratch[2] - 64 * P] == 0xA5).all()), "the one-workgroup form wrote slice minima"
    pm_scratch_check(*scratch, P, "pair_min P=33")


@pytest.mark.parametrize("N,M,P", [(5, 13, 3), (127, 129 + 1, 2), (512, 513, 2)])
def test_pair_min_masks(lib, N, M, P):
    """the global minimum sits at a masked-out row, then at a masked-out column: the answer is the minimum inside the masks; a pair with nothing
    inside its masks gives +inf (the contract tests/test_sinkhorn_gpu.py::test_empty_pair_does_not_poison_batch relies on)"""
    NM = N * M
    x = pm_state(P, NM, NM).view(P, N, M)
    sm, tm = torch.ones(P, N, dtype=torch.bool), torch.ones(P, M, dtype=torch.bool)
    sm[:, N - 2:] = False
    tm[:, M - 3:] = False
    sm[0, 1] = False                                                  # a hole inside the valid block as well
    tm[0, 2] = False
    if P > 1:
        sm[P - 1] = False                                             # the last pair: no valid row
    x[0, N - 1, 0] = 0.25                                             # masked-out row
    x[0, 1, 5] = 0.25
    x[0, 3, M - 1] = 0.125                                            # masked-out column
    x[0, 0, 2] = 0.125
    x[0, 2, 1] = 0.75                                                 # the masked minimum
    xh = x.cpu()
    exp = xh.masked_fill(~(sm[:, :, None] & tm[:, None, :]), math.inf).view(P, -1).min(1).values
    assert float(exp[0]) == 0.75 and (P == 1 or float(exp[P - 1]) == math.inf)
    smd, tmd = sm.to(DEV).view(torch.uint8), tm.to(DEV).view(torch.uint8)
    what = "pair_min masks %d x %d P=%d" % (N, M, P)
    pm_check(pm_call(lib, x, P, N, M, smd, tmd), P, exp, what + ", one workgroup")
    if NM >= PM_SPLIT_MIN_NM:
        scratch = pm_scratch(lib, P)
        pm_check(pm_call(lib, x, P, N, M, smd, tmd, scratch), P, exp, what + ", split")
        pm_check(pm_call(lib, x, P, N, M, scratch=scratch), P, xh.view(P, -1).min(1).values, what + ", split, no masks, same scratch")
        pm_scratch_check(*scratch, P, what)


def test_pair_min_refusals_write_nothing(lib):
    rc, k = lib.raw().dr_debug_pair_min_f64, codes()
    x, out = pm_state(2, 64, 1), blank(1, 2, dtype=torch.float64)[0].to(DEV)
    m = torch.ones(2, 8, dtype=torch.uint8, device=DEV)
    o = at(out, MARGIN)
    assert rc(2, 8, 0, at(x), None, None, o, None, stream()) == k["DR_EINVAL"]                     # M < 1
    assert rc(2, 0, 8, at(x), None, None, o, None, stream()) == k["DR_EINVAL"]
    assert rc(-1, 8, 8, at(x), None, None, o, None, stream()) == k["DR_EINVAL"]
    assert rc(2, 8, 8, None, None, None, o, None, stream()) == k["DR_EINVAL"]
    assert rc(2, 8, 8, at(x), None, None, None, None, stream()) == k["DR_EINVAL"]
    assert rc(2, 8, 8, at(x), at(m), None, o, None, stream()) == k["DR_EINVAL"]                    # one mask without the other
    assert rc(0, 8, 8, at(x), None, None, o, None, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ==============================================================================================================================================
# 5. ddim, the conversions and the sigmoid
# ==============================================================================================================================================
DDIM_TIMES = orc.time_pairs(20)


def ddim_coefficients_host(t, tn):
    """the five coefficients as the loops compute them on the host (csrc/loop_common.h) from the float64 schedule"""
    ac = orc.diffusion_schedule()[0]
    a, an = float(ac[t]), float(ac[tn])
    sigma = math.sqrt((1.0 - a / an) * (1.0 - an) / (1.0 - a))
    return dict(sra=math.sqrt(1.0 / a), srm1=math.sqrt(1.0 / a - 1.0), sigma=sigma, c=math.sqrt(1.0 - an - sigma * sigma),
                sqrt_an=float(np.float32(math.sqrt(an))))


def ddim_case(P, N, M, first, shift, noise, masked, seed):
    """one DDIM update: the state entering the step (float32 values on the first step, quirk Q2), x_start, xi, ragged masks, and the reference's
    next state per pair (ddim_expected, extended by sigma * xi in the state's dtype as the kernel's header states)"""
    g = gen(seed)
    t, tn = DDIM_TIMES[seed % 20]         # any step of the 20-step schedule, with or without the first step's float32 bookkeeping: at (999, 949)
    #                                       itself c is 1e-4, which hides that bookkeeping below the bar
    x = 3.0 * torch.randn(P, N, M, generator=g, dtype=torch.float32 if first else torch.float64)
    x0 = torch.rand(P, N, M, generator=g)
    xi = torch.randn(P, N, M, generator=g) if noise else None
    sm, tm = torch.ones(P, N, dtype=torch.bool), torch.ones(P, M, dtype=torch.bool)
    if masked:
        for p in range(P):
            sm[p, N - (p + 1) % N:] = False                      # ragged: pair p keeps N - (p + 1) % N rows and M - (2 p + 1) % M columns
            tm[p, M - (2 * p + 1) % M:] = False
        if N > 2:
            sm[0, 1] = False
    valid = sm[:, :, None] & tm[:, None, :]
    sigma = orc.ddim_coefficients(orc.diffusion_schedule()[0], t, tn)[0]
    exp, mins = [], []
    for p in range(P):
        x_in = x[p].masked_fill(~valid[p], math.inf) if shift else x[p]          # the shift is the minimum inside the masks
        mins.append(float(x_in.min()))
        e = ddim_expected(x_in, x0[p], t, tn, shift, first)
        if noise:
            e = e + sigma * xi[p].to(x.dtype)
        exp.append(e.double())
    return dict(P=P, N=N, M=M, first=first, t=t, tn=tn, x=x.double(), x0=x0, xi=xi, sm=sm if masked else None, tm=tm if masked else None,
                shift=torch.tensor(mins, dtype=torch.float64) if shift else None, valid=valid, expected=torch.stack(exp))


def ddim_check(c, x_raw):
    """the DDIM bar on a framed [P, N M] next state (the device's, or a host restatement's)"""
    P, NM = c["P"], c["N"] * c["M"]
    what = "ddim %d x %d P=%d first=%s shift=%s noise=%s masks=%s" % (c["N"], c["M"], P, c["first"], c["shift"] is not None, c["xi"] is not None, c["sm"] is not None)
    got = unframed(x_raw, MARGIN, P, NM, what=what).view(P, c["N"], c["M"])
    valid = c["valid"]
    assert bool((got[~valid] == -math.inf).all()), (what, "a masked entry is not -inf")
    assert bool(torch.isfinite(got[valid]).all()), (what, "an unmasked entry is not finite")
    e = float((got[valid] - c["expected"][valid]).abs().max()) if bool(valid.any()) else 0.0
    assert e <= DDIM_TOL, (what, e)
    return e


def ddim_device(lib, c):
    from diffreg_hip.lib import DebugDdimArgs
    P, NM = c["P"], c["N"] * c["M"]
    xd = framed(c["x"].view(P, NM))[0].to(DEV)
    keep = [c["x0"].to(DEV).contiguous()]
    a = DebugDdimArgs()
    a.x, a.x0 = xd.data_ptr() + MARGIN * 8, keep[0].data_ptr()
    for name, key, conv in (("shift", "shift", lambda v: v), ("noise", "xi", lambda v: v), ("src_mask", "sm", lambda v: v.view(torch.uint8)),
                            ("tgt_mask", "tm", lambda v: v.view(torch.uint8))):
        if c[key] is not None:
            keep.append(conv(c[key].contiguous()).to(DEV))
            setattr(a, name, keep[-1].data_ptr())
    a.N, a.M, a.first_step = c["N"], c["M"], 1 if c["first"] else 0
    for k, v in ddim_coefficients_host(c["t"], c["tn"]).items():
        setattr(a, k, v)
    rc = lib.raw().dr_debug_ddim_f64(ctypes.byref(a), P, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return xd


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("N,M", [(1, 1), (5, 7), (16, 17), (33, 255)])
def test_ddim(lib, N, M, P):
    worst, n = 0.0, 0
    for first in (False, True):
        for shift in (False, True):
            for noise in (False, True):
                for masked in (False, True):
                    n += 1
                    c = ddim_case(P, N, M, first, shift, noise, masked, 100 * N + 10 * P + n)
                    worst = max(worst, ddim_check(c, ddim_device(lib, c)))
    print("ddim %d x %d P=%d: x_next at most %.3e from the reference's arithmetic" % (N, M, P, worst))


def test_ddim_refusals_write_nothing(lib):
    from diffreg_hip.lib import DebugDdimArgs
    rc, k = lib.raw().dr_debug_ddim_f64, codes()
    x, x0 = blank(2, 12, dtype=torch.float64)[0].to(DEV), torch.rand(24, device=DEV)
    m = torch.ones(8, dtype=torch.uint8, device=DEV)

    def args(**kw):
        a = DebugDdimArgs()
        a.x, a.x0, a.N, a.M, a.first_step, a.sra, a.srm1, a.c, a.sigma, a.sqrt_an = x.data_ptr() + MARGIN * 8, x0.data_ptr(), 3, 4, 0, 1.0, 1.0, 1.0, 0.0, 1.0
        for name, v in kw.items():
            setattr(a, name, v)
        return ctypes.byref(a)
    assert rc(None, 2, stream()) == k["DR_EINVAL"]
    assert rc(args(), -1, stream()) == k["DR_EINVAL"]
    assert rc(args(N=0), 2, stream()) == k["DR_EINVAL"] and rc(args(M=0), 2, stream()) == k["DR_EINVAL"]
    assert rc(args(x=None), 2, stream()) == k["DR_EINVAL"] and rc(args(x0=None), 2, stream()) == k["DR_EINVAL"]
    assert rc(args(src_mask=m.data_ptr()), 2, stream()) == k["DR_EINVAL"]                           # one mask without the other
    assert rc(args(), 0, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all())


MAP_SIZES = [0, 1, 255, 256, 257, 100003]
F32_MAX = float(np.finfo(np.float32).max)


def map_device(lib, kind, x, out_dtype):
    n = x.numel()
    xd, out = framed(x.view(1, n))[0].to(DEV), blank(1, n, dtype=out_dtype)[0].to(DEV)
    rc = lib.raw().dr_debug_state_map(kind, at(xd, MARGIN), at(out, MARGIN), n, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return unframed(out, MARGIN, 1, n, what="state map %d n=%d" % (kind, n))[0]


def with_specials(x, specials):
    """the first entries AND the last ones (the tail block of the launch) are replaced by as many of `specials` as fit"""
    s = torch.tensor(specials, dtype=x.dtype)
    k = min(x.numel(), s.numel())
    x[:k] = s[:k]
    if x.numel() >= 2 * s.numel():
        x[-s.numel():] = s
    return x


@pytest.mark.parametrize("n", MAP_SIZES)
def test_conversions(lib, n):
    g = gen(n)
    x32 = with_specials(torch.randn(n, generator=g) * 10.0 ** torch.randint(-30, 30, (n,), generator=g).float(),
                        [0.0, -0.0, math.inf, -math.inf, F32_MAX, -F32_MAX, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38])
    assert same_bits(map_device(lib, 0, x32, torch.float64), x32.double())                  # exact widening
    half_ulp_over = F32_MAX + 2.0 ** 103                                                  # the tie between the largest float32 and 2^128: to even = inf
    x64 = with_specials(torch.randn(n, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-50, 39, (n,), generator=g).double(),
                        [0.0, -0.0, math.inf, -math.inf, 1e39, -1e39, half_ulp_over, -half_ulp_over, math.nextafter(half_ulp_over, 0.0), F32_MAX,
                         1e-40, -1e-40, 1e-46, -1e-46, 2.0 ** -150, -(2.0 ** -150), math.nextafter(2.0 ** -150, 1.0), 2.0 ** -149 * 1.5, 2.0 ** -149 * 2.5,
                         1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -52, 1.0 + 3 * 2.0 ** -24, 5e-324, 1.7976931348623157e308])
    ref = x64.float()                                                                     # torch's cast: round to nearest even
    if n >= 24:
        assert ref[6] == math.inf and ref[8] == F32_MAX and ref[14] == 0.0 and ref[16] == 2.0 ** -149 and ref[17] == 2.0 ** -148 and ref[18] == 2.0 ** -148
        assert bool((ref[1].view(torch.int32) == -2 ** 31)) and ref[19] == 1.0 and ref[20] > 1.0 and ref[21] == 1.0 + 2.0 ** -22
    assert same_bits(map_device(lib, 1, x64, torch.float32), ref)


@pytest.mark.parametrize("n", MAP_SIZES)
def test_sigmoid(lib, n):
    x = with_specials(10.0 * torch.randn(n, generator=gen(n + 1), dtype=torch.float64),
                      [0.0, -0.0, math.inf, -math.inf, 745.0, -745.0, 5e-324, -5e-324, 2.2250738585072014e-308, -1e-310, 36.7, -36.7, 709.0, -709.0])
    got, ref = map_device(lib, 2, x, torch.float64), torch.sigmoid(x)
    bar = 4.0 * torch.from_numpy(np.spacing(ref.numpy()))                                  # one ulp for exp, half each for the add and the divide, headroom
    assert bool(((got - ref).abs() <= bar).all()), ("sigmoid n=%d" % n, float(((got - ref).abs() / bar).max()))
    assert bool((got[x == -math.inf] == 0.0).all()) and bool((got[x == math.inf] == 1.0).all())
    assert bool(((got >= 0.0) & (got <= 1.0)).all())


def test_state_map_refusals(lib):
    rc, k = lib.raw().dr_debug_state_map, codes()
    x, out = torch.rand(16, device=DEV), blank(1, 16, dtype=torch.float64)[0].to(DEV)
    o = at(out, MARGIN)
    assert rc(3, at(x), o, 16, stream()) == k["DR_EINVAL"] and rc(-1, at(x), o, 16, stream()) == k["DR_EINVAL"]
    assert rc(0, at(x), o, -1, stream()) == k["DR_EINVAL"]
    assert rc(0, None, o, 16, stream()) == k["DR_EINVAL"] and rc(0, at(x), None, 16, stream()) == k["DR_EINVAL"]
    assert rc(0, None, None, 0, stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
