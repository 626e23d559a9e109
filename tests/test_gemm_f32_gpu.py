"""The fp32 GEMM family (csrc/gemm.hip, launch_gemm) under every geometry the library can select, against float64.

Geometries: "auto" (the library's own rule), 0 (32 x 32 tiles, k split over 4 waves and reduced through LDS, 128-k chunks), 9 (64 x 64
tiles, single LDS buffer, 32-k chunks), 11 / 12 (the register-only latency form with 8 / 16 waves: K <= 448 / 896).

Two kinds of operand:
  exact  -- small integers (A, W, bias, addend in [-8, 8]) and power-of-two scales: every product is exact in fp32 and every partial sum
            stays below 2^24 for K <= 4 096, so the result is exact in ANY summation order and must equal the float64 reference bit for bit.
            This is what catches a missing / doubled / misplaced k-group, tile row or column, or an epilogue on the wrong column.
  random -- normal floats with rows scaled over six orders of magnitude: each entry is bounded against float64 relative to
            S[r, c] = (|A| @ |W|^T)[r, c] (plus the epilogue's terms), not max |ref|, so a small row keeps its own accuracy.

The epilogue order the kernels implement (both the staged and the latency form):  out = scale * relu(rot(acc) + bias) + addend."""
import ctypes

import pytest
import torch

from tests.helpers import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
DR_OK, DR_EINVAL, DR_ENOSUP = 0, -1, -3
EPI_RELU, EPI_ROTARY = 1, 2
GEOMS = ["auto", 0, 9, 11, 12]
KMAX = {11: 448, 12: 896}           # the latency form's k range: 8 waves x NW x 7 groups of 8
TOL = 1e-6                          # x S: a k-ordered fp32 chain is ~1.5e-7 S at K <= 1 024, ~3.5e-7 S at K = 4 096


def lib():
    from diffreg_hip import lib as _lib
    return _lib


def fits(geom, K):
    return K <= KMAX.get(geom, 1 << 30)


@pytest.fixture
def force():
    """force(geom): select a geometry for the rest of the test; the library is back on its own rule afterwards"""
    L = lib()
    L.ensure_init()
    yield lambda g: L.raw().dr_debug_gemm_config(-1 if g == "auto" else g)
    L.raw().dr_debug_gemm_config(-1)


# ------------------------------------------------------------------------------------------------------------------------------------
# a problem, its operands and its float64 reference
# ------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """one GEMM problem with its own operands on the device.  out lives in a NaN-filled [nb, out_rows, ldo] buffer between guard bands, at
    column offset `coloff` (the q|k|v layout); A (and A2) are wider than their segments when lda > K1 (lda2 > K - K1).  nbatch > 1: A and
    out are strided per instance, W too unless shared_w (stride 0); A2, bias, addend and the rotary tables are shared by all instances."""

    def __init__(self, rows, ncols, K, *, seed, exact, K1=None, lda=None, lda2=None, ldo=None, coloff=0, relu=False, bias=False,
                 addend=False, rot_C=0, scale=1.0, row_mag=False, extra_rows=3, nbatch=0, shared_w=False):
        g = torch.Generator().manual_seed(seed)
        two = K1 is not None
        K1 = K1 if two else K
        lda = lda or K1
        lda2 = lda2 or (K - K1)
        ldo = ldo or (coloff + ncols)
        assert coloff + ncols <= ldo
        nb = max(nbatch, 1)

        def draw(*shape):
            if exact:
                return torch.randint(-8, 9, shape, generator=g).float()
            return torch.randn(*shape, generator=g)
        ra = max(rows, 1)                   # rows = 0 still passes real (unread) operands: the entry refuses NULL
        A = draw(nb, ra, lda)
        A2 = draw(ra, lda2) if two else None
        W = draw(1 if shared_w else nb, ncols, K)
        if row_mag and rows:
            mag = 10.0 ** (torch.arange(ra) % 7 - 3).float()[:, None]
            A *= mag
            if two:
                A2 *= mag
        self.rows, self.ncols, self.K, self.K1, self.lda, self.lda2, self.ldo, self.coloff = rows, ncols, K, K1, lda, lda2, ldo, coloff
        self.epi = (EPI_RELU if relu else 0) | (EPI_ROTARY if rot_C else 0)
        self.rot_C, self.scale, self.two, self.nbatch, self.nb, self.shared_w = rot_C, scale, two, nbatch, nb, shared_w
        self.A, self.A2, self.W = A.to(DEV), (A2.to(DEV) if two else None), W.to(DEV)
        self.bias = draw(ncols).to(DEV) if bias else None
        self.addend = draw(ra, ldo).to(DEV) if addend else None
        self.cos = self.sin = None
        if rot_C:
            ang = torch.rand(ra, rot_C // 2, generator=g, dtype=torch.float64) * 6.3
            self.cos, self.sin = ang.cos().float().to(DEV), ang.sin().float().to(DEV)
        self.out_rows = rows + extra_rows
        self.buf, self.guard = guarded((nb, self.out_rows, ldo), torch.float32, DEV, fill=NAN)

    def problem(self):
        return lib().gemm_problem(self.A, self.W, self.buf[:, :, self.coloff:], self.rows, self.ncols, self.K, self.lda, self.ldo,
                                  A2=self.A2, K1=self.K1 if self.two else 0, lda2=self.lda2 if self.two else 0, bias=self.bias,
                                  addend=None if self.addend is None else self.addend[:, self.coloff:], epilogue=self.epi, cos=self.cos, sin=self.sin, rot_C=self.rot_C, scale=self.scale,
                                  nbatch=self.nbatch, stride_a=self.A.shape[1] * self.lda, stride_w=0 if self.shared_w else self.ncols * self.K,
                                  stride_o=self.out_rows * self.ldo)

    def reset(self):
        self.buf.fill_(NAN)

    def got(self):
        return self.buf[:, :self.rows, self.coloff:self.coloff + self.ncols]

    def reference(self):
        """-> (float64 reference [nb, rows, ncols], float64 error scale E: |error| <= TOL E is the bound of the random kind)"""
        A = self.A[:, :self.rows, :self.K1].double()
        if self.two:
            A = torch.cat([A, self.A2[:self.rows, :self.K - self.K1].double().expand(self.nb, -1, -1)], 2)
        W = self.W.double().transpose(1, 2)
        acc, S = A @ W, A.abs() @ W.abs()
        if self.rot_C:
            c = torch.arange(self.ncols, device=DEV)
            h = (c % self.rot_C) // 2
            cs, sn = self.cos[:self.rows].double()[:, h], self.sin[:self.rows].double()[:, h]
            partner = c ^ 1
            sign = torch.where(c % 2 == 1, 1.0, -1.0).double()
            acc = acc * cs + sign * acc[..., partner] * sn
            S = S * cs.abs() + S[..., partner] * sn.abs()
        if self.bias is not None:
            acc = acc + self.bias.double()
            S = S + self.bias.double().abs()
        if self.epi & EPI_RELU:
            acc = acc.clamp_min(0.0)
        acc, S = acc * self.scale, S * abs(self.scale)
        if self.addend is not None:
            ad = self.addend[:self.rows, self.coloff:self.coloff + self.ncols].double()
            acc, S = acc + ad, S + ad.abs()
        return acc, S

    def assert_untouched_outside(self):
        """rows past `rows`, the columns left of the offset and the gap columns up to ldo still hold their NaN; nothing beyond the buffer"""
        self.guard()
        inside = torch.zeros(self.nb, self.out_rows, self.ldo, dtype=torch.bool, device=DEV)
        inside[:, :self.rows, self.coloff:self.coloff + self.ncols] = True
        assert bool(torch.isnan(self.buf[~inside]).all()), "a write outside rows x ncols"

    def assert_exact(self, tag=""):
        ref = self.reference()[0].float()
        got = self.got()
        bad = (got != ref).nonzero()
        assert bad.shape[0] == 0, ("%s: %d entries differ from the exact result, first at %s: got %r, want %r"
                                   % (tag, bad.shape[0], bad[0].tolist(), got[tuple(bad[0])].item(), ref[tuple(bad[0])].item()))
        assert torch.equal(got, ref)
        self.assert_untouched_outside()

    def assert_bound(self, tag="", good=None):
        """every entry (of `good` [rows, ncols], default all) finite and within TOL E of float64"""
        ref, S = self.reference()
        got = self.got().double()
        good = torch.ones(self.rows, self.ncols, dtype=torch.bool, device=DEV) if good is None else good
        good = good.expand(self.nb, -1, -1)
        assert bool(torch.isfinite(got[good]).all()), tag + ": non-finite entries"
        err = ((got - ref).abs() - TOL * S)[good]
        if err.numel():
            worst = int(err.argmax())
            assert float(err.max()) <= 0.0, ("%s: an entry exceeds %.0e S: got %r, want %r, S %r" % (
                tag, TOL, got[good][worst].item(), ref[good][worst].item(), S[good][worst].item()))
        self.assert_untouched_outside()


def launch(cases, checked=True):
    return lib().debug_gemm([c.problem() for c in cases], cases[0].W, checked=checked)


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) exact operands: bit-exact at every tile / chunk / k-group / latency-form boundary
# ------------------------------------------------------------------------------------------------------------------------------------
ROWS = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
KS = [4, 28, 32, 36, 60, 64, 68, 124, 128, 132, 444, 448, 452, 892, 896, 900, 1532, 4096]
# K <= 448 (12 values) meets every rows and every ncols value, so even geometry 11 sees each boundary in all three dimensions.
# Boundaries crossed on both sides, per geometry:
#   rows / ncols  31|32|33, 63|64|65, 127|128|129, 257: the 32-wide tiles of 0, 11, 12 and the 64-wide tiles of 9 (all geometries)
#   K 4, 28|32|36, 60|64|68: 8-k groups (all), the 32-k chunk of 9 and the 32 k per wave and chunk of 0's 4-way split
#   K 124|128|132, 1532, 4096: the 128-k chunk of 0 (and several chunks of 9)
#   K 444|448|452: the end of 11's range (452 refused: test_forced_latency_form_beyond_its_range_is_refused); 892|896|900 likewise for 12
EXACT_SHAPES = [(ROWS[i % 11], ROWS[(i * 5 + 3) % 11], K) for i, K in enumerate(KS)]
EXACT_CASES = [(s, g) for s in EXACT_SHAPES for g in GEOMS if fits(g, s[2])]


@pytest.mark.parametrize("shape,geom", EXACT_CASES, ids=["%dx%dx%d-%s" % (s + (g,)) for s, g in EXACT_CASES])
def test_exact_integer_operands(shape, geom, force):
    """plain (lda = K, ldo = ncols) and the full epilogue (bias, ReLU, scale 0.5, addend) with lda > K, ldo > ncols: bit-exact, and
    nothing written outside rows x ncols"""
    force(geom)
    rows, ncols, K = shape
    plain = Case(rows, ncols, K, seed=rows * 7 + ncols * 131 + K, exact=True)
    launch([plain])
    plain.assert_exact("plain")
    full = Case(rows, ncols, K, seed=rows + ncols * 17 + K * 3, exact=True, lda=K + 8, ldo=ncols + 5, relu=True, bias=True, addend=True,
                scale=0.5)
    launch([full])
    full.assert_exact("bias + relu + scale + addend")
    up = Case(rows, ncols, K, seed=K * 11 + 5, exact=True, bias=True, scale=2.0)     # no ReLU: negative entries keep their value
    launch([up])
    up.assert_exact("bias + scale 2")


# K1 at, just before and just after the 128-k chunk (geometry 0), the 32-k chunk (9) and an 8-k group (all); the second segment ends at
# or around a boundary too.  lda / lda2 wider than the segments.
TWO_SEG = [(65, 33, 28, 64), (33, 65, 32, 96), (129, 64, 36, 100), (64, 129, 8, 44), (31, 127, 12, 60), (63, 31, 124, 256),
           (127, 63, 128, 256), (257, 32, 132, 264), (32, 257, 4, 448), (1, 65, 444, 448), (96, 65, 440, 892), (40, 70, 896, 900),
           (33, 64, 1024, 1532)]
TWO_CASES = [(s, g) for s in TWO_SEG for g in GEOMS if fits(g, s[3])]


@pytest.mark.parametrize("shape,geom", TWO_CASES, ids=["%dx%dx%d|%d-%s" % (s[:3] + (s[3] - s[2], g)) for s, g in TWO_CASES])
def test_exact_two_segment_a(shape, geom, force):
    """A = [A | A2] along k (mlp0 on [x | msg]; grad_y = g_k Wk + g_v Wv): the segment boundary K1 must neither drop nor repeat a k"""
    force(geom)
    rows, ncols, K1, K = shape
    c = Case(rows, ncols, K, seed=K1 * 13 + K, exact=True, K1=K1, lda=K1 + 4, lda2=K - K1 + 12)
    launch([c])
    c.assert_exact("two segments")
    c = Case(rows, ncols, K, seed=K1 * 17 + K, exact=True, K1=K1, lda=K1 + 12, lda2=K - K1 + 4, ldo=ncols + 3, relu=True, bias=True,
             addend=True, scale=0.25)
    launch([c])
    c.assert_exact("two segments + epilogue")


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) random floats: per-entry bound against float64 at the production shapes, every applicable geometry
# ------------------------------------------------------------------------------------------------------------------------------------
RANDOM_SHAPES = [
    (300, 432, 432), (300, 528, 528), (300, 256, 256), (300, 64, 64),          # 3DMatch / 4DMatch / 2D-3D widths
    (564, 629, 432), (564, 629, 864),                                          # single pair: similarity, mlp2
    (3072, 256, 256),                                                          # 2D-3D loop projections
    (256, 256, 96), (256, 256, 1024), (256, 256, 1532), (256, 256, 4096),      # weight gradients C x C x R4
    (1530, 256, 1024), (1024, 256, 1532),                                      # circle-loss backward
]


@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=["%dx%dx%d" % s for s in RANDOM_SHAPES])
def test_random_floats_every_geometry(shape, force):
    """rows over six orders of magnitude; plain, and bias + ReLU + scale + addend with lda > K and ldo > ncols: every entry within 1e-6 S
    of float64 under auto and every geometry whose range holds K (so they also agree with each other)"""
    rows, ncols, K = shape
    plain = Case(rows, ncols, K, seed=K + ncols, exact=False, row_mag=True)
    full = Case(rows, ncols, K, seed=K * 3 + ncols, exact=False, row_mag=True, lda=K + 4, ldo=ncols + 2, relu=True, bias=True,
                addend=True, scale=0.125)
    for geom in GEOMS:
        if not fits(geom, K):
            continue
        force(geom)
        for c, tag in ((plain, "plain"), (full, "epilogue")):
            c.reset()
            launch([c])
            c.assert_bound("%s, geometry %s" % (tag, geom))


ROT_CASES = [(96, 432, 432, 432, 0), (300, 256, 256, 256, 256), (33, 128, 64, 64, 64), (257, 64, 128, 64, 0), (1193, 432, 432, 432, 432)]


@pytest.mark.parametrize("rows,ncols,K,rot_C,coloff", ROT_CASES, ids=["%dx%dx%d-rot%d-off%d" % s for s in ROT_CASES])
def test_rotary_epilogue(rows, ncols, K, rot_C, coloff, force):
    """rotary on q / k written into a q|k|v buffer (ldo = 3C, column offset 0 or C), and rot_C < ncols (a fused q|k, ncols = 2 rot_C):
    rotary, then bias, ReLU, scale, addend -- in the staged and in the latency epilogue"""
    plain = Case(rows, ncols, K, seed=rows + K, exact=False, row_mag=True, rot_C=rot_C, coloff=coloff, ldo=3 * max(ncols, rot_C))
    full = Case(rows, ncols, K, seed=rows + 2 * K, exact=False, row_mag=True, rot_C=rot_C, coloff=coloff, ldo=3 * max(ncols, rot_C),
                relu=True, bias=True, addend=True, scale=0.5)
    for geom in GEOMS:
        if not fits(geom, K):
            continue
        force(geom)
        for c, tag in ((plain, "rotary"), (full, "rotary + epilogue")):
            c.reset()
            launch([c])
            c.assert_bound("%s, geometry %s" % (tag, geom))


# ------------------------------------------------------------------------------------------------------------------------------------
# strided batches
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("nbatch,rows,ncols,K", [(1, 65, 33, 30), (2, 33, 64, 130), (128, 31, 17, 66), (257, 9, 40, 28)])
def test_bmm_nt_batches(nbatch, rows, ncols, K, geom, force):
    """lib.bmm_nt (dr_gemm_nt_batched_f32; K not a multiple of 4 is zero-padded by the wrapper): every batch bit-exact"""
    force(geom)
    g = torch.Generator().manual_seed(nbatch * 1000 + K)
    a = torch.randint(-8, 9, (nbatch, rows, K), generator=g).float()
    b = torch.randint(-8, 9, (nbatch, ncols, K), generator=g).float()
    ref = (a.double() @ b.double().transpose(1, 2) * 0.5).float()
    got = lib().bmm_nt(a.to(DEV), b.to(DEV), scale=0.5)
    assert torch.equal(got.cpu(), ref)


BATCHED = [(2, 64, 65, 128, False), (5, 33, 31, 36, True), (130, 17, 32, 452, True), (3, 129, 33, 900, False)]
BATCHED_CASES = [(b, g) for b in BATCHED for g in GEOMS if fits(g, b[3])]


@pytest.mark.parametrize("case,geom", BATCHED_CASES, ids=["b%d-%dx%dx%d-%s-%s" % (b[:4] + ("w0" if b[4] else "wz", g)) for b, g in BATCHED_CASES])
def test_batched_strides_and_gaps(case, geom, force):
    """dr_gemm_nt_batched_f32 with stride_o > rows ncols (the gaps between instances untouched) and stride_w = 0 (one weight for all)"""
    nbatch, rows, ncols, K, shared_w = case
    force(geom)
    L = lib()
    g = torch.Generator().manual_seed(nbatch + rows + K)
    sA, sO = rows * K + 8, rows * ncols + 37
    A = torch.randint(-8, 9, (nbatch * sA,), generator=g).float().to(DEV)
    W = torch.randint(-8, 9, (1 if shared_w else nbatch, ncols * K), generator=g).float().to(DEV)
    out, chk = guarded((nbatch * sO,), torch.float32, DEV, fill=NAN)
    rc = L.raw().dr_gemm_nt_batched_f32(nbatch, rows, ncols, K, L.ptr(A), sA, L.ptr(W), 0 if shared_w else ncols * K, L.ptr(out), sO,
                                        2.0, L.stream_of(A))
    assert rc == DR_OK
    chk()
    inside = torch.zeros(nbatch * sO, dtype=torch.bool, device=DEV)
    for z in range(nbatch):
        a = A[z * sA:z * sA + rows * K].view(rows, K).double()
        w = W[0 if shared_w else z].view(ncols, K).double()
        o = out[z * sO:z * sO + rows * ncols].view(rows, ncols)
        assert torch.equal(o, (a @ w.t() * 2.0).float()), "instance %d" % z
        inside[z * sO:z * sO + rows * ncols] = True
    assert bool(torch.isnan(out[~inside]).all()), "a write into the gap between instances"


# ------------------------------------------------------------------------------------------------------------------------------------
# grouped launches: 2..4 different problems in one grid
# ------------------------------------------------------------------------------------------------------------------------------------
def group_cases(kind):
    if kind == "small":             # max K 444: every geometry
        return [Case(33, 31, 36, seed=1, exact=False, relu=True, bias=True),
                Case(1, 128, 444, seed=2, exact=False, rot_C=128, coloff=3, ldo=131),
                Case(0, 32, 32, seed=3, exact=False, addend=True),
                Case(70, 64, 128, seed=4, exact=False, K1=64, lda=68, lda2=72, addend=True, scale=0.5)]
    if kind == "mixed":             # max K 512; one of them a strided batch with a shared weight
        return [Case(96, 256, 256, seed=6, exact=False, relu=True, bias=True), Case(200, 64, 512, seed=7, exact=False, K1=256, addend=True),
                Case(40, 33, 68, seed=5, exact=False, nbatch=3, shared_w=True, extra_rows=1), Case(0, 64, 64, seed=8, exact=False)]
    # the 2D-3D training's backward (train_fusion.hip): R x C activation gradients with K = C and K = 2C (two segments) next to C x C weight
    # gradients contracted over the R4 tokens
    return [Case(1024, 64, 64, seed=9, exact=False, row_mag=True), Case(1024, 64, 128, seed=10, exact=False, K1=64, addend=True),
            Case(64, 64, 1024, seed=11, exact=False, row_mag=True), Case(64, 64, 1532, seed=12, exact=False, nbatch=2)]


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("kind", ["small", "mixed", "train"])
def test_grouped_launch(kind, geom, force):
    """2..4 different problems (rows, ncols, K, epilogues, nbatch; one with rows = 0) in one grid, every problem within the random-operand
    bound; under a forced geometry each is also bit-identical to the same problem launched alone (nothing couples problems -- auto may pick
    another geometry for a problem alone, since it decides from the group's largest K and total tiles).  A latency form that cannot hold
    the group's largest K refuses the whole group."""
    cases = group_cases(kind)
    force(geom)
    if not fits(geom, max(c.K for c in cases)):
        assert launch(cases, checked=False) == DR_ENOSUP
        for c in cases:
            c.assert_untouched_outside()
        return
    launch(cases)
    grouped = []
    for i, c in enumerate(cases):
        c.assert_bound("problem %d of the group, geometry %s" % (i, geom))
        grouped.append(c.buf.clone())
    if geom == "auto":
        return
    for i, c in enumerate(cases):
        c.reset()
        launch([c])
        assert torch.equal(c.buf.nan_to_num(-7.0), grouped[i].nan_to_num(-7.0)), "problem %d alone != in the group" % i


# ------------------------------------------------------------------------------------------------------------------------------------
# no-ops, refusals, degenerate values
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_noops_leave_the_output_alone(geom, force):
    """rows = 0 (internal form and dr_linear_f32) and nbatch = 0 return DR_OK and write nothing"""
    force(geom)
    L = lib()
    c = Case(0, 64, 64, seed=1, exact=True, addend=True, bias=True, relu=True)
    assert launch([c], checked=False) == DR_OK
    c.assert_untouched_outside()
    x = torch.zeros(4, 64, device=DEV)
    W = torch.ones(32, 64, device=DEV)
    out, chk = guarded((4, 32), torch.float32, DEV, fill=NAN)
    assert L.raw().dr_linear_f32(0, 32, 64, L.ptr(x), L.ptr(W), L.ptr(out), 0, None, None, 0, 1.0, L.stream_of(x)) == DR_OK
    assert L.raw().dr_gemm_nt_batched_f32(0, 4, 32, 64, L.ptr(x), 256, L.ptr(W), 0, L.ptr(out), 128, 1.0, L.stream_of(x)) == DR_OK
    assert L.raw().dr_gemm_nt_batched_f32(2, 0, 32, 64, L.ptr(x), 256, L.ptr(W), 0, L.ptr(out), 128, 1.0, L.stream_of(x)) == DR_OK
    chk()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("geom,K", [(11, 452), (12, 900), (11, 900), (12, 4096)])
def test_forced_latency_form_beyond_its_range_is_refused(geom, K, force):
    """the latency form holds 8 NW 7 k of a row in registers: forced beyond that it returns DR_ENOSUP and launches nothing (it used to drop
    every k past the limit and report DR_OK)"""
    force(geom)
    c = Case(64, 64, K, seed=K, exact=True)
    assert launch([c], checked=False) == DR_ENOSUP
    c.assert_untouched_outside()
    assert bool(torch.isnan(c.got()).all())
    lim = Case(64, 64, KMAX[geom], seed=K + 1, exact=True)         # at the limit it runs, exactly
    launch([lim])
    lim.assert_exact("K at the limit")


def test_env_selected_latency_form_beyond_its_range_is_refused(force, monkeypatch):
    """DR_GEMM_CFG (read only under dr_debug_enable_env) replaces the staged geometry of a large launch: a latency form that cannot hold K
    is refused the same way"""
    L = lib()
    force("auto")
    monkeypatch.setenv("DR_GEMM_CFG", "11")
    L.raw().dr_debug_enable_env(1)
    try:
        c = Case(1024, 512, 900, seed=3, exact=True, extra_rows=1)     # 128 tiles of 64 x 64 and K > 896: geometry 9 by the rule
        rc = launch([c], checked=False)
    finally:
        L.raw().dr_debug_enable_env(0)
    assert rc == DR_ENOSUP
    c.assert_untouched_outside()
    c.reset()
    launch([c])                                                        # knobs off again: the rule's own geometry, exact
    c.assert_exact("after the knob")


@pytest.mark.parametrize("geom", [1, 2, 3, 10, 13])
def test_unknown_geometries_are_refused(geom, force):
    """geometries 1 and 2 (128 x 64 / 64 x 64 double-buffered tiles) were never selected by the library and are gone: forcing one is
    DR_EINVAL, like any other unknown number"""
    force(geom)
    c = Case(64, 64, 64, seed=geom, exact=True)
    assert launch([c], checked=False) == DR_EINVAL
    c.assert_untouched_outside()


def test_debug_entry_validates_its_arguments(force):
    """dr_debug_gemm_f32: n outside 1..4 and malformed problems are DR_EINVAL; misaligned operands DR_ENOSUP, before anything launches"""
    force("auto")
    L = lib()
    c = Case(64, 64, 64, seed=1, exact=True, K1=32, lda=36, lda2=32)
    s = L.stream_of(c.W)
    arr = (L.DebugGemmProblem * 5)(*([c.problem()] * 5))
    assert L.raw().dr_debug_gemm_f32(arr, 0, s) == DR_EINVAL
    assert L.raw().dr_debug_gemm_f32(arr, 5, s) == DR_EINVAL
    assert L.raw().dr_debug_gemm_f32(None, 1, s) == DR_EINVAL

    def rc(**kw):
        p = c.problem()
        for k, v in kw.items():
            setattr(p, k, v)
        return L.raw().dr_debug_gemm_f32(ctypes.byref(p), 1, s)
    assert rc(K1=0) == DR_EINVAL and rc(K1=64) == DR_EINVAL                # a second segment must be non-empty
    assert rc(lda=28) == DR_EINVAL and rc(lda2=28) == DR_EINVAL and rc(ldo=63) == DR_EINVAL
    assert rc(ncols=0) == DR_EINVAL and rc(rows=-1) == DR_EINVAL and rc(nbatch=-1) == DR_EINVAL
    assert rc(epilogue=EPI_ROTARY) == DR_EINVAL and rc(epilogue=4) == DR_EINVAL
    assert rc(K1=34) == DR_ENOSUP and rc(lda=34) == DR_ENOSUP             # the segment boundary / lda not a multiple of 4
    assert rc(A=c.A.data_ptr() + 4) == DR_ENOSUP                           # A not 16-byte aligned
    c.assert_untouched_outside()
    assert bool(torch.isnan(c.got()).all())


DEGEN_CASES = [(g, K) for K in (132, 1532) for g in GEOMS if fits(g, K)]


@pytest.mark.parametrize("geom,K", DEGEN_CASES)
def test_degenerate_rows_and_columns_stay_put(geom, K, force):
    """zero rows, rows 1e-30 and 1e30 times the others, an inf in one row of A and a NaN in one column of W: only that row and that column
    may be non-finite, every other entry keeps its bound (nothing is shared across rows or columns of a tile)"""
    force(geom)
    rows, ncols = 130, 100
    c = Case(rows, ncols, K, seed=K, exact=False, bias=True, addend=True, ldo=ncols + 4)
    c.A[0, 3] = 0.0
    c.A[0, 10] *= 1e-30
    c.A[0, 11] *= 1e30
    c.A[0, 64, K // 2] = float("inf")
    c.W[0, 33, K - 1] = float("nan")
    launch([c])
    good = torch.ones(rows, ncols, dtype=torch.bool, device=DEV)
    good[64] = False
    good[:, 33] = False
    c.assert_bound("degenerate rows, geometry %s" % geom, good=good)
    got = c.got()[0]
    assert not bool(torch.isfinite(got[64]).any()) and not bool(torch.isfinite(got[:, 33]).any())
    zero = (c.bias + c.addend[3, :ncols])[good[3]]                      # a zero row: bias + addend, exactly
    assert torch.equal(got[3][good[3]], zero)
