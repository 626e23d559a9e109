"""Every forward attention form of csrc/attention.hip, one at a time, against float64 on the CPU at its tile edges: the 32-query kernel with 4 and
with 8 waves, the 128-query flash kernel on the f32-input MFMA and on split bf16 operands, the plane-image kernel with one and with two key groups
(three-product and single-product f16, with and without the XCD dealing), in every head-dim geometry the dispatcher instantiates.

Each case asserts WHICH form ran (dr_debug_attention_last_form, include/diffreg_hip_debug.h) before it compares numbers: a case that reached
another kernel fails.  The f32 forms are reached through dr_attention_f32, the flash ones forced with dr_debug_attention_config(1) and
dr_debug_attention_split(0 | 1) (restored to -1 behind every call), the plane forms by shape alone (workgroups against the CU count, Lk >= 128,
H P % 8).  No DR_* environment knob is read.

Reference: float64 softmax(q k^T / sqrt(d)) v per head from the definition (attn_reference of the primitives test for dr_attention_f32: key j is
dead for query l when q_mask[l] && !k_mask[j]; the plane entry as test_attention_on_plane_images: keys outside k_mask are dead, rows with q_mask
set are compared).  Inputs are float32 values cast up; v is scaled by 2 (f32 entry) or 3 (plane entry).  Every output lies between guard bands and
starts as NaN; every compared entry must be finite.

Bounds: largest absolute error over every compared entry / largest entry of the float64 reference
  * f32-product forms and the plane three-product form: < 1e-5 (ATTN_BOUND of the primitives test, the bound of test_attention_on_plane_images);
  * flash on split operands: < 1e-5 (measured on an MI355X over every case of this file: the largest quotient is below it, table in DESIGN.md);
  * plane single-product f16: between 1e-5 and 3e-3 (test_attention_on_plane_images_f16_entry; the lower end proves the mode was on).

Each case prints its figures ("[fig] ...") before it asserts; run with -s to see them.  The last test of the file needs the whole file to have run
in this process: it asserts that the getter has shown every form.  Needs a GPU."""
import ctypes
import functools

import pytest
import torch

from diffreg_hip import lib
from tests.helpers import guarded
from tests.test_train_primitives_gpu import ATTN_BOUND, attn_masks, attn_reference, fig, gen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NAN = float("nan")

# DR_ATTN_FORM_* of include/diffreg_hip_debug.h
Q32_W4, Q32_W8, FLASH_F32, FLASH_SPLIT, PLANES_KG1, PLANES_KG2 = 1, 2, 3, 4, 5, 6
FORM_MASK, FORM_F16, FORM_XCD, GEOM_SHIFT = 0xf, 0x10, 0x20, 8
FORM_NAME = {Q32_W4: "q32-w4", Q32_W8: "q32-w8", FLASH_F32: "flash-f32", FLASH_SPLIT: "flash-split", PLANES_KG1: "planes-kg1", PLANES_KG2: "planes-kg2"}

SPLIT_BOUND = 1e-5            # flash on split operands against float64: measured, see the module docstring
PLANES_BOUND = 1e-5
F16_LOW, F16_HIGH = 1e-5, 3e-3

SEEN = set()                  # every value the getter returned in this process
WORST = {}                    # (form name [+ f16], geometry) -> largest quotient


def geom_of(d):
    return 8 if d <= 64 else 14 if d <= 112 else 17 if d <= 136 else 20


def last_form():
    f = int(lib.raw().dr_debug_attention_last_form())
    SEEN.add(f)
    return f


def describe(f):
    return "%s%s%s geometry %d" % (FORM_NAME.get(f & FORM_MASK, "none"), " f16" if f & FORM_F16 else "", " xcd" if f & FORM_XCD else "", f >> GEOM_SHIFT)


def expect_form(got, form, d, f16=False, xcd=False):
    want = form | (FORM_F16 if f16 else 0) | (FORM_XCD if xcd else 0) | (geom_of(d) << GEOM_SHIFT)
    assert got == want, "ran %s, the case is about %s" % (describe(got), describe(want))


def quotient(got, ref, keep=None):
    """max |got - ref| over every compared entry / max |ref|; every compared entry finite"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if keep is not None:
        got, ref_c = got[keep.cpu()], ref[keep.cpu()]
    else:
        ref_c = ref
    assert bool(torch.isfinite(got).all()), "non-finite entries in the device result"
    return float((got - ref_c).abs().max()) / float(ref.abs().max())


def note(form, x):
    key = (FORM_NAME[form & FORM_MASK] + (" f16" if form & FORM_F16 else ""), form >> GEOM_SHIFT)
    WORST[key] = max(WORST.get(key, 0.0), x)


# ================================================================================================================================
# the float32 entry: dr_attention_f32
# ================================================================================================================================
@functools.lru_cache(maxsize=None)
def f32_inputs(B, L, S, H, d, qscale=1.0):
    g = gen(B, L, S, H, d, 5)
    C = H * d
    q, k = torch.randn(B, L, C, generator=g) * qscale, torch.randn(B, S, C, generator=g)
    v = torch.randn(B, S, C, generator=g) * 2
    return q, k, v


def f32_reference(q, k, v, H, qm, km):
    return attn_reference(q, k, v, torch.zeros_like(q), H, qm, km)[0]


FORCE = {"q32": (-1, -1), "flash": (1, 0), "split": (1, 1)}


class forced:
    """the flash forms through the debug setters; both back at -1 behind the call whatever happens"""
    def __init__(self, how):
        self.cfg = FORCE[how]

    def __enter__(self):
        lib.ensure_init()
        lib.raw().dr_debug_attention_config(self.cfg[0])
        lib.raw().dr_debug_attention_split(self.cfg[1])

    def __exit__(self, *exc):
        lib.raw().dr_debug_attention_config(-1)
        lib.raw().dr_debug_attention_split(-1)


def run_f32(how, q, k, v, H, qm, km):
    out, chk = guarded(q.shape, F32, DEV, fill=NAN)
    dv = lambda t_: None if t_ is None else t_.to(DEV)
    with forced(how):
        lib.attention(dv(q), dv(k), dv(v), H, dv(qm), dv(km), out=out)
        form = last_form()
    chk()
    return out, form


def check_f32(what, how, form, B, L, S, H, d, qm, km, qscale=1.0):
    q, k, v = f32_inputs(B, L, S, H, d, qscale)
    ref = f32_reference(q, k, v, H, qm, km)
    assert bool(torch.isfinite(ref).all())
    out, got = run_f32(how, q, k, v, H, qm, km)
    expect_form(got, form, d)
    e = quotient(out, ref)
    fig("%s %s B%d L%d S%d H%d d%d" % (what, describe(got), B, L, S, H, d), out=e)
    note(got, e)
    bound = SPLIT_BOUND if form == FLASH_SPLIT else ATTN_BOUND
    assert e < bound, (e, bound)


# ---- head dims: every geometry first with its smallest d, then up to its padded width and past the next one's start ----------------------------
HEAD_D = (4, 16, 60, 64, 68, 100, 108, 112, 116, 132, 136)
FLASH_D = [(how, H, d) for how in ("flash", "split") for d in HEAD_D for H in (1, 4)]


@pytest.mark.parametrize("how,H,d", FLASH_D, ids=["%s-H%d-d%d" % c for c in FLASH_D])
@pytest.mark.parametrize("masked", [False, True], ids=["full", "masked"])
def test_flash_head_dims(how, H, d, masked):
    """both flash kernels at head dims below, at and between the padded widths of the three geometries (columns d .. DP - 1 are zero-filled at the LDS
    store, the float4 loads clamped at nv4 - 1); L = 130 is two query blocks, the second with two rows.  Above d = 112 the split form does not exist:
    the dispatcher must run the f32 flash kernel, and the numbers are held there too."""
    B, L, S = 2, 130, 70
    qm, km = attn_masks(B, L, S, gen(B, L, S, 11)) if masked else (None, None)
    form = FLASH_SPLIT if how == "split" and d <= 112 else FLASH_F32
    check_f32("head dim", how, form, B, L, S, H, d, qm, km)


@pytest.mark.parametrize("d", [64, 108, 132])
def test_eight_wave_head_dims(d):
    """the 32-query kernel at S > 128 and at most 256 workgroups: 8 waves deal the 7 key tiles at d = 64 and 108; AttnGeom<17,5,8> needs 183 808 bytes
    of LDS (> 160 KiB), so d = 132 must run 4 waves"""
    check_f32("8-wave head dim", "q32", Q32_W4 if d == 132 else Q32_W8, 2, 130, 200, 4, d, None, None)


# ---- lengths -------------------------------------------------------------------------------------------------------------------------------------
LENGTHS = ((1, 1), (1, 200), (200, 1), (31, 33), (32, 32), (33, 31), (127, 129), (128, 128), (129, 127), (257, 65))
LEN_CFG = {"flash-d108": ("flash", FLASH_F32, 108), "flash-d64": ("flash", FLASH_F32, 64), "split-d108": ("split", FLASH_SPLIT, 108),
           "w8-d108": ("q32", Q32_W8, 108)}
LEN_CASES = [(c, L, S) for c in LEN_CFG for (L, S) in LENGTHS]


@pytest.mark.parametrize("cfg,L,S", LEN_CASES, ids=["%s-L%d-S%d" % c for c in LEN_CASES])
@pytest.mark.parametrize("masked", [False, True], ids=["full", "masked"])
def test_lengths(cfg, L, S, masked):
    """one query / one key, one below / at / one past the 32-key tile and the 128-query block, three query blocks.  The 8-wave form exists for
    S > 128 only: the other pairs must run 4 waves."""
    how, form, d = LEN_CFG[cfg]
    if form == Q32_W8 and S <= 128:
        form = Q32_W4
    B, H = 2, 4
    qm, km = attn_masks(B, L, S, gen(B, L, S, 13)) if masked else (None, None)
    check_f32("lengths", how, form, B, L, S, H, d, qm, km)


# ---- masks ---------------------------------------------------------------------------------------------------------------------------------------
MASK_S = 200                    # 7 key tiles, the last with 8 keys: 8 waves dealing them leave a wave without a tile, 4 waves deal two each but one


def mask_case(name, B, L, S):
    """-> (q_mask, k_mask).  b to e keep q_mask all ones, so that the dead keys are dead for every query."""
    assert S == MASK_S
    g = gen(B, L, S, 17)
    ones = torch.ones(B, L, dtype=torch.bool)
    km = torch.ones(B, S, dtype=torch.bool)
    last = (S - 1) // 32 * 32
    if name == "a":
        return attn_masks(B, L, S, g)
    if name == "f":                                                  # rows without q_mask see every key; they are compared too
        qm, km = attn_masks(B, L, S, g)
        qm[:, [0, 31, 32, L - 1]] = False
        for b in range(B):
            qm[b, (5 * b + 64) % L] = False
        return qm, km
    if name.startswith("b"):                                         # a dead first tile, two, every tile before the last
        km[:, :{"b32": 32, "b64": 64, "blast": last}[name]] = False
    elif name == "c":                                                # a dead middle tile
        km[:, 64:96] = False
    elif name == "d":                                                # dead tiles at the end (every ragged batch): keys 0 .. 4 alive
        km[:, 5:] = False
    else:                                                            # exactly one key alive (another one per batch element where there is room)
        km[:] = False
        for b in range(B):
            km[b, {"e-first": 5 + b % 20, "e-mid": 100 + b % 20, "e-last": S - 1}[name]] = True
    return ones, km


MASK_NAMES = ("a", "b32", "b64", "blast", "c", "d", "e-first", "e-mid", "e-last", "f")
# (B, L, H): the 4-wave form at S > 128 needs more than 256 32-query workgroups (22 x 4 x 3 = 264) and fewer than 256 flash ones (6 x 4 x 3 = 72)
MASK_CFG = {"w4-d108": ("q32", Q32_W4, 108, (3, 704, 4)), "w8-d108": ("q32", Q32_W8, 108, (2, 130, 4)),
            "flash-d108": ("flash", FLASH_F32, 108, (2, 130, 4)), "flash-d64": ("flash", FLASH_F32, 64, (2, 130, 4)),
            "split-d108": ("split", FLASH_SPLIT, 108, (2, 130, 4)), "split-d64": ("split", FLASH_SPLIT, 64, (2, 130, 4))}
MASK_CASES = [(c, m) for c in MASK_CFG for m in MASK_NAMES]


@pytest.mark.parametrize("cfg,mask", MASK_CASES, ids=["%s-%s" % c for c in MASK_CASES])
def test_masks(cfg, mask):
    """per batch element different masks; 32-key tiles that are entirely dead: first (the running maximum is -inf at the first rescale), middle (the
    state must not move), trailing; one live key; rows without q_mask.  In the 32-query kernel the waves whose dealt tiles are all dead reach the
    merge with m = -inf."""
    how, form, d, (B, L, H) = MASK_CFG[cfg]
    qm, km = mask_case(mask, B, L, MASK_S)
    check_f32("mask " + mask, how, form, B, L, MASK_S, H, d, qm, km)


@pytest.mark.parametrize("cfg", list(MASK_CFG))
def test_peaked_softmax(cfg):
    """q scaled by 3: logits of standard deviation 3, a softmax that a few keys dominate.  Every form stays inside its own bound here (DESIGN.md
    section 5o), so the case has no bound of its own."""
    how, form, d, (B, L, H) = MASK_CFG[cfg]
    qm, km = mask_case("a", B, L, MASK_S)
    check_f32("peaked", how, form, B, L, MASK_S, H, d, qm, km, qscale=3.0)


# ---- row stride, misaligned out ------------------------------------------------------------------------------------------------------------------
def raw_attention(B, H, L, S, d, q_ptr, k_ptr, v_ptr, ld, mq, mk, out_ptr, stream):
    return lib.raw().dr_attention_f32(B, H, L, S, d, q_ptr, k_ptr, v_ptr, ld, lib.ptr(mq), lib.ptr(mk), 1.0 / d ** 0.5, out_ptr, stream)


@pytest.mark.parametrize("how,form", [("flash", FLASH_F32), ("split", FLASH_SPLIT)])
def test_flash_row_stride_beyond_the_heads(how, form):
    """ld = 3 C as test_attention_row_stride_beyond_the_heads: q | k | v column slices of one buffer, out the middle third of a sentinel-filled one"""
    B, L, H, d = 2, 130, 4, 108
    S, C = L, H * d
    ld = 3 * C
    q, k, v = f32_inputs(B, L, S, H, d)
    qm, km = attn_masks(B, L, S, gen(B, L, S, 19))
    ref = f32_reference(q, k, v, H, qm, km)
    qkv = torch.cat([q, k, v], 2).reshape(B * L, ld).contiguous().to(DEV)
    SENT = 12345.0
    O, chk = guarded((B * L, ld), F32, DEV, fill=SENT)
    at = lambda t_, col: ctypes.c_void_p(t_.data_ptr() + 4 * col)
    mq, mk = lib.mask_u8(qm.to(DEV)), lib.mask_u8(km.to(DEV))
    with forced(how):
        lib.check(raw_attention(B, H, L, S, d, at(qkv, 0), at(qkv, C), at(qkv, 2 * C), ld, mq, mk, at(O, C), lib.stream_of(qkv)))
        got = last_form()
    chk()
    expect_form(got, form, d)
    e = quotient(O[:, C:2 * C].reshape(B, L, C), ref)
    fig("ld = 3 C %s" % describe(got), out=e)
    note(got, e)
    assert e < (SPLIT_BOUND if form == FLASH_SPLIT else ATTN_BOUND), e
    assert bool((O[:, :C] == SENT).all()) and bool((O[:, 2 * C:] == SENT).all()), "padding columns written"


def test_misaligned_out_falls_back_to_the_32_query_kernel():
    """ldo % 4 == 0 but `out` 4 bytes past a 16-byte boundary: the flash kernels store float4, so the dispatcher must run the 32-query kernel even
    when the flash form is forced.  Rows of C + 4 floats: q, k, v in columns 0 .. C - 1, out in columns 1 .. C of its own buffer."""
    B, L, S, H, d = 2, 130, 70, 4, 108
    C = H * d
    ld = C + 4
    q, k, v = f32_inputs(B, L, S, H, d)
    qm, km = attn_masks(B, L, S, gen(B, L, S, 23))
    ref = f32_reference(q, k, v, H, qm, km)
    wide = lambda t_: torch.nn.functional.pad(t_.reshape(-1, C), (0, 4)).contiguous().to(DEV)
    Q, K, V = wide(q), wide(k), wide(v)
    SENT = 12345.0
    O, chk = guarded((B * L, ld), F32, DEV, fill=SENT)
    assert O.data_ptr() % 16 == 0
    mq, mk = lib.mask_u8(qm.to(DEV)), lib.mask_u8(km.to(DEV))
    with forced("flash"):
        lib.check(raw_attention(B, H, L, S, d, lib.ptr(Q), lib.ptr(K), lib.ptr(V), ld, mq, mk, ctypes.c_void_p(O.data_ptr() + 4), lib.stream_of(Q)))
        got = last_form()
    chk()
    expect_form(got, Q32_W4, d)
    e = quotient(O[:, 1:C + 1].reshape(B, L, C), ref)
    fig("misaligned out %s" % describe(got), out=e)
    note(got, e)
    assert e < ATTN_BOUND, e
    assert bool((O[:, 0] == SENT).all()) and bool((O[:, C + 1:] == SENT).all()), "padding columns written"


# ================================================================================================================================
# the plane-image entry: dr_attention_planes / dr_attention_planes_f16
# ================================================================================================================================
IMG_FILL = 0x7e                 # two of these bytes are an fp16 NaN: an image unit the kernel did not write decodes as NaN


@functools.lru_cache(maxsize=None)
def plane_inputs(P, Lq, Lk, H, d, qscale=1.0):
    g = gen(P, Lq, Lk, H, d, 29)
    C = H * d
    return torch.randn(P, Lq, C, generator=g) * qscale, torch.randn(P, Lk, C, generator=g), torch.randn(P, Lk, C, generator=g) * 3


def plane_reference(q, k, v, H, km):
    """float64; keys outside k_mask are dead for every query (the rows with q_mask set are the ones compared)"""
    P, Lq, C = q.shape
    d = C // H
    qh, kh, vh = (z.double().view(P, -1, H, d).transpose(1, 2) for z in (q, k, v))
    logit = qh @ kh.transpose(-1, -2) / d ** 0.5
    if km is not None:
        logit = logit.masked_fill(~km[:, None, None, :], float("-inf"))
    return (torch.softmax(logit, -1) @ vh).transpose(1, 2).reshape(P, Lq, C)


def run_planes(q, k, v, H, qm, km, f16=False):
    """the images as lib.attention_planes builds them (head-padded columns, one k / v bound per segment); the out image and out bound between guard
    bands, starting as NaN -> (return code, out [P, Lq, H, dp] decoded, out bound [P Lq], form, raw out image)"""
    lib.ensure_init()
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    P, Lq, C = q.shape
    Lk, d = k.shape[1], C // H
    dp = (d + 15) // 16 * 16

    def pad(x):
        y = torch.zeros(x.shape[0] * x.shape[1], H * dp, device=DEV)
        y.view(-1, H, dp)[:, :, :d] = x.reshape(-1, H, d)
        return y
    qi, qb = lib.planes_from_f32(pad(q))
    ki, kb = lib.planes_from_f32_bounded(pad(k), k.abs().amax((1, 2)).repeat_interleave(Lk))
    vi, vb = lib.planes_from_f32_bounded(pad(v), v.abs().amax((1, 2)).repeat_interleave(Lk))
    oi, chk_i = guarded((lib.raw().dr_plane_image_bytes(P * Lq, H * dp),), torch.uint8, DEV, fill=IMG_FILL)
    ob, chk_b = guarded((P * Lq,), F32, DEV, fill=NAN)
    mq = lib.mask_u8(None if qm is None else qm.to(DEV))
    mk = lib.mask_u8(None if km is None else km.to(DEV))
    entry = lib.raw().dr_attention_planes_f16 if f16 else lib.raw().dr_attention_planes
    rc = entry(P, Lq, Lk, H, d, lib.ptr(qi), lib.ptr(qb), lib.ptr(ki), lib.ptr(kb), lib.ptr(vi), lib.ptr(vb), lib.ptr(mq), lib.ptr(mk), lib.ptr(oi),
               lib.ptr(ob), lib.stream_of(q))
    form = last_form()
    chk_i(); chk_b()
    o = lib.planes_to_f32(oi, ob, P * Lq, H * dp).view(P, Lq, H, dp) if rc == 0 else None
    return rc, o, ob, form, oi


def check_planes(what, form, P, Lq, Lk, H, d, qm, km, f16=False, xcd=False, qscale=1.0):
    q, k, v = plane_inputs(P, Lq, Lk, H, d, qscale)
    ref = plane_reference(q, k, v, H, km)
    assert bool(torch.isfinite(ref).all())
    rc, o, ob, got, _ = run_planes(q, k, v, H, qm, km, f16)
    lib.check(rc)
    expect_form(got, form, d, f16, xcd)
    keep = qm if qm is not None else torch.ones(P, Lq, dtype=torch.bool)
    e = quotient(o[:, :, :, :d].reshape(P, Lq, H * d), ref, keep)
    fig("%s %s P%d Lq%d Lk%d H%d d%d" % (what, describe(got), P, Lq, Lk, H, d), out=e)
    note(got, e)
    assert bool((o[:, :, :, d:] == 0).all()), "the head pad of the out image is not zero"
    assert bool((ob.cpu().view(P, Lq).double() >= ref.abs().amax(2))[keep].all()), "the out bound is no upper bound of its row"
    if f16:
        assert F16_LOW < e < F16_HIGH, e
    else:
        assert e < PLANES_BOUND, e


def plane_masks(P, Lq, Lk):
    """what test_attention_on_plane_images masks, per segment different"""
    qm, km = torch.ones(P, Lq, dtype=torch.bool), torch.ones(P, Lk, dtype=torch.bool)
    qm[:, Lq - 5:] = False
    km[:, Lk - 7:] = False
    km[0, :3] = False
    for p in range(P):
        km[p, 11 + 2 * p:Lk:13 + p] = False
        qm[p, (3 * p + 1) % Lq] = False
    return qm, km


KG1_SHAPE, KG2_SHAPE = (2, 96, 80, 4), (2, 96, 160, 4)          # Lk < 128: one key group; 8 workgroups and Lk >= 128: two
# every width at which attn_store_planes changes branch: the unit that ends at d (52 + 4, 60 + 4 | 100 + 4, 104 | 136), the one that straddles it
PLANE_D = (52, 60, 64, 100, 104, 108, 112, 132, 136)


@pytest.mark.parametrize("d", PLANE_D)
@pytest.mark.parametrize("kg", [1, 2])
@pytest.mark.parametrize("masked", [False, True], ids=["full", "masked"])
def test_planes_head_dims(d, kg, masked):
    P, Lq, Lk, H = KG1_SHAPE if kg == 1 else KG2_SHAPE
    qm, km = plane_masks(P, Lq, Lk) if masked else (None, None)
    check_planes("plane head dim", PLANES_KG1 if kg == 1 else PLANES_KG2, P, Lq, Lk, H, d, qm, km)


@pytest.mark.parametrize("Lk", [128, 129, 191, 192, 257])
@pytest.mark.parametrize("masked", [False, True], ids=["full", "masked"])
def test_planes_two_key_groups_key_lengths(Lk, masked):
    """an even and an odd number of key tiles (the group with one tile fewer keeps the other's barriers company), the last tile complete or not"""
    P, Lq, H, d = 2, 96, 4, 108
    qm, km = plane_masks(P, Lq, Lk) if masked else (None, None)
    check_planes("KG2 key length", PLANES_KG2, P, Lq, Lk, H, d, qm, km)


def test_planes_one_key_group_five_key_tiles():
    """one key group with at least four key tiles runs only past one workgroup per CU (the launcher compares the workgroup count with
    hipDeviceProp_t::multiProcessorCount, 256 on an MI355X; torch reports the same number): P = 65 segments x 4 heads x 1 query block = 260"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    P = 65 if cus < 260 else cus // 4 + 1
    check_planes("KG1 five tiles", PLANES_KG1, P, 32, 130, 4, 108, None, None)


@pytest.mark.parametrize("P,Lq,Lk,H,kg,xcd", [(2, 300, 160, 4, 2, True), (4, 129, 64, 2, 1, True), (2, 300, 160, 3, 2, False)],
                         ids=["kg2-xcd", "kg1-xcd", "kg2-H3-off"])
@pytest.mark.parametrize("masked", [False, True], ids=["full", "masked"])
def test_planes_xcd_dealing(P, Lq, Lk, H, kg, xcd, masked):
    """H P a multiple of 8 and more than one query block: the workgroup ids are dealt so that the query blocks of one (head, segment) share an XCD --
    a permutation of (query block, head, segment) that must reach every triple once; H = 3: off"""
    qm, km = plane_masks(P, Lq, Lk) if masked else (None, None)
    check_planes("XCD dealing", PLANES_KG1 if kg == 1 else PLANES_KG2, P, Lq, Lk, H, 108, qm, km, xcd=xcd)


@pytest.mark.parametrize("d", [64, 100, 136])
@pytest.mark.parametrize("kg", [1, 2])
def test_planes_f16_single_product(d, kg):
    P, Lq, Lk, H = KG1_SHAPE if kg == 1 else KG2_SHAPE
    check_planes("plane f16", PLANES_KG1 if kg == 1 else PLANES_KG2, P, Lq, Lk, H, d, None, None, f16=True)


# (P, Lq, H) at Lk = 200: 2 x 2 x 4 = 16 workgroups -> two key groups, H P = 8 and two query blocks -> dealt; 33 x 2 x 4 = 264 workgroups -> one key group
PLANE_MASK_CFG = {"kg1": (PLANES_KG1, (33, 130, 4), False), "kg2": (PLANES_KG2, (2, 130, 4), True)}
PLANE_MASK_NAMES = ("b32", "b64", "blast", "c", "d", "e-first", "e-mid", "e-last")
PLANE_MASK_CASES = [(c, m) for c in PLANE_MASK_CFG for m in PLANE_MASK_NAMES]


@pytest.mark.parametrize("cfg,mask", PLANE_MASK_CASES, ids=["%s-%s" % c for c in PLANE_MASK_CASES])
def test_planes_dead_tiles(cfg, mask):
    """the dead-tile masks of test_masks on the plane kernel: with two key groups, group 0 (tiles 0, 2, 4, 6) or group 1 (tiles 1, 3, 5) holds only dead
    tiles in several of them and reaches the group merge with m = -inf"""
    form, (P, Lq, H), xcd = PLANE_MASK_CFG[cfg]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if form == PLANES_KG1 and 2 * H * P <= cus:
        P = cus // (2 * H) + 1
    qm, km = mask_case(mask, P, Lq, MASK_S)
    check_planes("plane mask " + mask, form, P, Lq, MASK_S, H, 108, qm, km, xcd=xcd)


@pytest.mark.parametrize("cfg", ["kg1", "kg2", "kg1-f16", "kg2-f16"])
def test_planes_peaked_softmax(cfg):
    kg, f16 = cfg[:3], cfg.endswith("f16")
    P, Lq, Lk, H = KG1_SHAPE if kg == "kg1" else KG2_SHAPE
    qm, km = plane_masks(P, Lq, Lk)
    check_planes("plane peaked", PLANES_KG1 if kg == "kg1" else PLANES_KG2, P, Lq, Lk, H, 108, qm, km, f16=f16, qscale=3.0)


@pytest.mark.parametrize("d", [68, 116])
def test_planes_refuse_a_head_dim_off_the_bucket_width(d):
    """ceil16(68) = 80 is not the 112 of its bucket, ceil16(116) = 128 not 144: DR_EINVAL, nothing launched, nothing written"""
    P, Lq, Lk, H = KG1_SHAPE
    q, k, v = plane_inputs(P, Lq, Lk, H, d)
    rc, _, ob, got, oi = run_planes(q, k, v, H, None, None)
    assert rc == -1 and lib.raw().dr_strerror(rc) == b"invalid argument", rc
    assert got == 0, describe(got)
    assert bool((oi == IMG_FILL).all()) and bool(torch.isnan(ob).all()), "a refused call wrote its outputs"


# ================================================================================================================================
def test_every_form_was_seen():
    """the getter has shown every form in this process (needs the tests above to have run): prints the largest quotient per form and geometry"""
    for (name, geom), x in sorted(WORST.items()):
        print("[fig] worst %-14s geometry %2d: %.3e" % (name, geom, x))
    seen = {(f & FORM_MASK, f >> GEOM_SHIFT, bool(f & FORM_F16)) for f in SEEN}
    need = [(Q32_W4, 14, False), (Q32_W8, 14, False), (FLASH_F32, 8, False), (FLASH_F32, 14, False), (FLASH_F32, 17, False), (FLASH_SPLIT, 8, False),
            (FLASH_SPLIT, 14, False), (PLANES_KG1, 14, False), (PLANES_KG2, 14, False), (PLANES_KG1, 14, True), (PLANES_KG2, 14, True)]
    missing = [describe(f | (g << GEOM_SHIFT) | (FORM_F16 if h else 0)) for f, g, h in need if (f, g, h) not in seen]
    assert not missing, missing
    assert any(f & FORM_XCD for f in SEEN), "the XCD dealing never ran"
