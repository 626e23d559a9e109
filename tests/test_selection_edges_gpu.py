"""The match read-out and selection kernels of csrc/stateops.hip -- dr_mutual_topk_select_f32, dr_mutual_match_f32 / _f64,
dr_top1_union_f32 / _f64 -- against the plain statements of tests/selection_ref.py at the sizes where their scans, ballots and LDS
carves change: more than 256 batch elements, more than 256 bit-words, ragged last words, the LDS limits, k = 1 .. 8, ties, NaN, +-inf,
a capacity below the true count, NULL outputs.  Needs a GPU.

All of it is index work: indices are compared with torch.equal, scores and confidences bit for bit (they are copies of the input),
every call runs twice and must return identical bytes, and every output that can be truncated lies between guard bands.
tests/test_selection_edges_cpu.py holds the statements themselves to the reference project's rule and to a second restatement."""
import ctypes
import itertools

import pytest
import torch

from tests import selection_ref as S
from tests.helpers import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, EINVAL, ENOSUP = 0, -1, -3
SENT = -777.25            # an exactly representable value that no input of these tests holds
INF = float("inf")


def dv(x):
    return None if x is None else x.to(DEV)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------
# dr_mutual_topk_select_f32
# ------------------------------------------------------------------------------------------------
def hold_topk(score, k, row_masks=None, col_masks=None, largest=True, threshold=None, mutual=True):
    """the wrapper's (b, i, j, score), twice, against mutual_topk_ref -> the reference's tuple"""
    from diffreg_hip import lib
    ref = S.mutual_topk_ref(score, k, row_masks, col_masks, largest, threshold, mutual)
    runs = [lib.batch_mutual_topk_select(dv(score), k, dv(row_masks), dv(col_masks), largest, threshold, mutual) for _ in range(2)]
    for a, b in zip(*runs):
        assert same_bytes(a, b)
    what = (tuple(score.shape), k, largest, threshold, mutual)
    for got, want in zip(runs[0][:3], ref[:3]):
        assert torch.equal(got.cpu(), want), what
    assert same_bytes(runs[0][3].cpu(), ref[3]), what
    return ref


def raw_topk(score, k, largest=True, threshold=None, mutual=True, capacity=0, null_out=False, spare=4):
    """the C entry with `capacity` rows of room (+ `spare` rows it is not told about) -> (code, total, idx, score), guard bands checked"""
    from diffreg_hip import lib
    r = lib.raw()
    lib.ensure_init()
    s = score.to(DEV).contiguous()
    B, N, M = s.shape
    idx, ck_i = guarded((capacity + spare, 3), torch.int64, DEV, fill=-7)
    sc, ck_s = guarded((capacity + spare,), torch.float32, DEV, fill=SENT)
    tot = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    wsb = r.dr_mutual_topk_workspace_bytes(B, N, M)
    ws, ck_w = guarded((max(wsb, 16),), torch.uint8, DEV)
    code = r.dr_mutual_topk_select_f32(B, N, M, lib.ptr(s), int(k), 1 if largest else 0, 0 if threshold is None else 1,
                                       0.0 if threshold is None else float(threshold), 1 if mutual else 0, None, None,
                                       None if null_out else lib.ptr(idx), None if null_out else lib.ptr(sc), capacity, lib.ptr(tot),
                                       lib.ptr(ws), wsb, stream())
    ck_i(); ck_s(); ck_w()
    return code, int(tot.item()), idx.cpu(), sc.cpu()


@pytest.mark.parametrize("B", [1, 255, 256, 257, 600])
def test_topk_batch_scan_carry(B):
    """mt_scan_kernel scans the per-element counts in blocks of 256 with a running carry: B on both sides of one block and past two,
    with counts that vary and elements that select nothing"""
    c = S.scan_case(B)
    per = torch.bincount(hold_topk(**c)[0], minlength=B)
    if B > 1:
        assert int((per == 0).sum()) >= 3 and per.unique().numel() >= 4
    if B > 256:
        assert int(per[256:].sum()) > 0 and int(per[:256].sum()) > 0


@pytest.mark.parametrize("N,M", [(50, 37), (96, 96), (97, 95), (128, 96), (1, 70), (70, 1), (64, 64), (63, 65)])
def test_topk_word_carry_and_ragged_last_word(N, M):
    """mt_write_kernel walks the N M selection bits in blocks of 256 words with a running carry: below, at and past 256 words
    (96 x 96 = 288, 97 x 95 = 288 and a ragged last one, 128 x 96 = 384), N M off a multiple of 32, one row, one column"""
    k = min(2, N, M)
    for kind, mutual in itertools.product(("distinct", "quant"), (False, True)):
        hold_topk(S.topk_scores(kind, 3, N, M), k, mutual=mutual)
    rm, cm = S.topk_masks("random", 3, N, M)
    hold_topk(S.topk_scores("distinct", 3, N, M), k, rm, cm, threshold=0.0, mutual=False)


def test_topk_lds_limit():
    """both bit planes of one element live in 64 KiB of LDS: 512 x 512 is the largest tile taken, 512 x 513 is refused untouched"""
    for kind, mutual in (("distinct", True), ("quant", False)):
        ref = hold_topk(S.topk_scores(kind, 2, 512, 512), 2, mutual=mutual)
        assert len(ref[0]) >= 2 * 512
    code, total, idx, sc = raw_topk(torch.zeros(1, 512, 513), 2, capacity=64)
    assert code == ENOSUP and total == 0
    assert bool((idx == -7).all()) and bool((sc == SENT).all())


@pytest.mark.parametrize("k", range(1, 9))
def test_topk_every_k(k):
    for kind, mutual, largest in itertools.product(("distinct", "quant"), (False, True), (True, False)):
        hold_topk(S.topk_scores(kind, 3, 16, 24), k, largest=largest, mutual=mutual)


@pytest.mark.parametrize("N,M,k", [(5, 24, 5), (16, 7, 7), (8, 8, 8), (1, 9, 1), (9, 1, 1)])
def test_topk_k_equals_a_side(N, M, k):
    """k == N selects every entry on the column side, k == M on the row side"""
    for kind, mutual in itertools.product(("distinct", "quant", "nan"), (False, True)):
        ref = hold_topk(S.topk_scores(kind, 3, N, M), k, mutual=mutual)
        if kind != "nan" and not mutual:
            assert len(ref[0]) == 3 * N * M


def test_topk_k_above_the_kernels_limit_is_refused():
    code, _, idx, sc = raw_topk(torch.zeros(1, 16, 24), 9, capacity=64)
    assert code == EINVAL
    assert bool((idx == -7).all()) and bool((sc == SENT).all())


@pytest.mark.parametrize("largest,mutual,thresholded", list(itertools.product((True, False), (True, False), (False, True))))
def test_topk_switches(largest, mutual, thresholded):
    """the threshold equals several selected entries exactly; the comparison is strict, so none of them is kept"""
    c = S.switch_case(largest)
    thr = c["threshold"] if thresholded else None
    b, i, j, sc = hold_topk(c["score"], c["k"], largest=largest, threshold=thr, mutual=mutual)
    assert len(b) >= 3
    if thresholded:
        plain = S.mutual_topk_ref(c["score"], c["k"], None, None, largest, None, mutual)[3]
        assert int((plain == thr).sum()) >= 3 and not bool((sc == thr).any())


@pytest.mark.parametrize("masks", ["random", "empty_row_mask", "one_col", "rows_only", "cols_only"])
def test_topk_masks(masks):
    for (kind, N, M), mutual in itertools.product((("quant", 40, 40), ("distinct", 63, 65)), (False, True)):
        rm, cm = S.topk_masks(masks, 3, N, M)
        b = hold_topk(S.topk_scores(kind, 3, N, M), 2, rm, cm, threshold=0.25, mutual=mutual)[0]
        if masks == "empty_row_mask":
            assert int((b == 1).sum()) == 0 and len(b) > 0


@pytest.mark.parametrize("name", sorted(S.TOPK_EDGE_INPUTS))
def test_topk_ties_nan_inf(name):
    """equal scores: the lower index wins; NaN is never selected and ranks after everything; +-inf are ordinary values"""
    score = S.topk_edge_input(name)
    for k, largest, mutual, thr in itertools.product((1, 2, 8), (True, False), (True, False), (None, 0.5)):
        sc = hold_topk(score, k, largest=largest, threshold=thr, mutual=mutual)[3]
        assert not torch.isnan(sc).any()


def test_topk_capacity_below_the_true_count():
    """`total` is the true count whatever the room; the first min(capacity, count) rows are the reference's prefix and nothing
    beyond them is written"""
    score = S.topk_scores("quant", 3, 40, 40)
    b, i, j, s = S.mutual_topk_ref(score, 2, None, None, True, None, False)
    want, count = torch.stack([b, i, j], 1), len(b)
    assert count > 3 * 40 * 2
    for capacity in (0, 1, count - 1, count):
        outs = [raw_topk(score, 2, mutual=False, capacity=capacity, null_out=capacity == 0) for _ in range(2)]
        code, total, idx, sc = outs[0]
        assert code == OK and total == count
        n = min(capacity, count)
        assert torch.equal(idx[:n], want[:n]) and same_bytes(sc[:n], s[:n])
        assert bool((idx[n:] == -7).all()) and bool((sc[n:] == SENT).all())
        assert outs[1][1] == total and same_bytes(outs[1][2], idx) and same_bytes(outs[1][3], sc)


# ------------------------------------------------------------------------------------------------
# dr_mutual_match_f32 / _f64
# ------------------------------------------------------------------------------------------------
DTYPES = [torch.float32, torch.float64]


def hold_match(conf, thr, mutual, cap=None):
    """lib.mutual_match, twice, and Matching.get_match against mutual_match_ref -> number of matches"""
    from diffreg_hip import lib
    from models.matching import Matching
    P, N, M = conf.shape
    ref_mask = S.mutual_match_mask(conf, thr, mutual)
    ref = ref_mask.nonzero()
    ref_conf = conf[ref[:, 0], ref[:, 1], ref[:, 2]]
    per = torch.bincount(ref[:, 0], minlength=P)
    runs = [lib.mutual_match(dv(conf), thr, mutual, cap=cap, want_mask=True) for _ in range(2)]
    for a, b in zip(*runs):
        assert same_bytes(a, b)
    m, mc, cnt, mask = [x.cpu() for x in runs[0]]
    what = (tuple(conf.shape), conf.dtype, thr, mutual)
    assert cnt.tolist() == per.tolist(), what
    assert int(per.max()) <= m.shape[1], what
    assert torch.equal(torch.cat([m[p, :per[p]] for p in range(P)]), ref), what
    assert same_bytes(torch.cat([mc[p, :per[p]] for p in range(P)]), ref_conf), what
    assert torch.equal(mask.bool(), ref_mask), what
    idx, mconf, gmask = Matching.get_match(dv(conf), thr, mutual)
    assert torch.equal(idx.cpu(), ref) and same_bytes(mconf.cpu(), ref_conf) and torch.equal(gmask.cpu(), ref_mask), what
    return len(ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,M", [(1, 1), (15, 63), (16, 64), (17, 65), (33, 129), (200, 130), (3, 4096), (4096, 3)])
def test_match_shapes(N, M, dtype):
    """rows dealt to 16 waves, 64 columns per ballot, MM_MAX = 4096 columns in LDS: one below, at and one past each step.
    Ties that are row and column maxima (columns 63 and 64 where there are that many), NaN in a row, a column and the corner,
    mutual=False with a threshold that keeps about a tenth, and the two infinite thresholds."""
    P = 3
    n = hold_match(S.match_conf("distinct", P, N, M, dtype), 0.0, True)
    assert n >= P
    n = hold_match(S.match_conf("ties", P, N, M, dtype), 0.4, True)
    assert n >= P * (6 if min(N, M) >= 3 else 1)
    hold_match(S.match_conf("nan", P, N, M, dtype), 0.0, True)
    hold_match(S.match_conf("nan", P, N, M, dtype), 0.9, False, cap=N * M)
    conf = S.match_conf("distinct", P, N, M, dtype)
    n = hold_match(conf, 0.9, False, cap=N * M)
    assert 0.05 * P * N * M <= n <= 0.15 * P * N * M or N * M < 1000
    assert hold_match(conf, INF, True) == 0 and hold_match(conf, INF, False) == 0
    assert hold_match(conf, -INF, False, cap=N * M) == P * N * M


def raw_match(conf, thr, mutual, cap, P=None, want_mconf=True, want_mask=True):
    """the C entry -> (code, matches [P,cap,3], mconf [P,cap], count [P], mask [P,N,M]); untouched memory reads -7 / SENT / -5 / 9.
    The two lists have room for one pair more than the call is told of, and that room must stay untouched: a row written past the
    last pair's `cap` lands there, whatever the guard bands' rounding."""
    from diffreg_hip import lib
    r = lib.raw()
    lib.ensure_init()
    c = conf.to(DEV).contiguous()
    P_, N, M = c.shape
    m, ck_m = guarded((P_ + 1, cap, 3), torch.int64, DEV, fill=-7)
    mc, ck_c = guarded((P_ + 1, cap), conf.dtype, DEV, fill=SENT)
    cnt, ck_n = guarded((P_,), torch.int32, DEV, fill=-5)
    mask, ck_k = guarded((P_, N, M), torch.uint8, DEV, fill=9)
    fn = r.dr_mutual_match_f64 if conf.dtype == torch.float64 else r.dr_mutual_match_f32
    code = fn(P_ if P is None else P, N, M, lib.ptr(c), float(thr), 1 if mutual else 0, cap, lib.ptr(m), lib.ptr(mc) if want_mconf else None,
              lib.ptr(cnt), lib.ptr(mask) if want_mask else None, stream())
    ck_m(); ck_c(); ck_n(); ck_k()
    assert bool((m[P_] == -7).all()) and bool((mc[P_] == SENT).all()), "a row was written past the last pair's cap"
    return code, m[:P_].cpu(), mc[:P_].cpu(), cnt.cpu(), mask.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
def test_match_refusals_and_empty_batch(dtype):
    for N, M in ((1, 4097), (4097, 1)):
        code, m, mc, cnt, mask = raw_match(torch.zeros(1, N, M, dtype=dtype), 0.0, True, 8)
        assert code == ENOSUP
        assert bool((m == -7).all()) and bool((mc == SENT).all()) and bool((cnt == -5).all()) and bool((mask == 9).all())
    code, m, mc, cnt, mask = raw_match(S.match_conf("ties", 3, 17, 65, dtype), 0.0, True, 17 + 65, P=0)
    assert code == OK
    assert bool((m == -7).all()) and bool((mc == SENT).all()) and bool((cnt == -5).all()) and bool((mask == 9).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,M", [(17, 65), (33, 129)])
def test_match_truncation(N, M, dtype):
    """a constant matrix: every entry is a mutual match, count = N M > cap = N + M.  The count is the true one, the rows are the
    reference's prefix with their confidences, the mask is complete and nothing lands outside the buffers."""
    P, cap = 3, N + M
    conf = S.match_conf("const", P, N, M, dtype)
    ref = S.mutual_match_ref(conf, 0.0, True)
    assert len(ref) == P * N * M
    outs = [raw_match(conf, 0.0, True, cap) for _ in range(2)]
    code, m, mc, cnt, mask = outs[0]
    assert code == OK and cnt.tolist() == [N * M] * P
    for p in range(P):
        want = ref[ref[:, 0] == p][:cap]
        assert torch.equal(m[p], want)
        assert same_bytes(mc[p], conf[want[:, 0], want[:, 1], want[:, 2]])
    assert bool((mask == 1).all())
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert same_bytes(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_match_null_outputs(dtype):
    """mconf and mask are optional, each alone and together; what is asked for does not change"""
    conf = S.match_conf("ties", 3, 33, 129, dtype)
    _, m0, mc0, cnt0, mask0 = raw_match(conf, 0.4, True, 33 + 129)
    assert int(cnt0.min()) >= 6
    for want_mconf, want_mask in ((False, True), (True, False), (False, False)):
        code, m, mc, cnt, mask = raw_match(conf, 0.4, True, 33 + 129, want_mconf=want_mconf, want_mask=want_mask)
        assert code == OK and same_bytes(m, m0) and same_bytes(cnt, cnt0)
        assert same_bytes(mc, mc0) if want_mconf else bool((mc == SENT).all())
        assert same_bytes(mask, mask0) if want_mask else bool((mask == 9).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_get_match_lists_a_constant_matrix_in_full(dtype):
    """more matches than the N + M rows of the first call: Matching.get_match asks again with N M rows and returns the exact list"""
    from models.matching import Matching
    conf = S.match_conf("const", 3, 17, 65, dtype)
    ref = S.mutual_match_ref(conf, 0.0, True)
    runs = [Matching.get_match(dv(conf), 0.0, True) for _ in range(2)]
    idx, mconf, mask = runs[0]
    assert len(idx) == 3 * 17 * 65 and torch.equal(idx.cpu(), ref)
    assert same_bytes(mconf.cpu(), conf.reshape(-1)) and bool(mask.all())
    for a, b in zip(*runs):
        assert same_bytes(a, b)


# ------------------------------------------------------------------------------------------------
# dr_top1_union_f32 / _f64
# ------------------------------------------------------------------------------------------------
TOP1_KINDS = ("distinct", "quant", "const", "inf")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,M", [(1, 1), (1, 100), (100, 1), (31, 70), (32, 70), (47, 70), (48, 65), (2048, 2048), (4095, 1), (1, 4095)])
def test_top1_shapes(N, M, dtype):
    """N = 31 | 32: the one-workgroup kernel | the row-block kernels with their merge (47 and 48 rows: a ragged and a full third block);
    N + M = T1_MAX = 4096 fills the bitonic sort's LDS exactly; one row, one column.  Three different tiles per call; distinct values,
    8 levels, a constant, whole rows / columns of -inf and single +inf.  First occurrence wins a tie, as torch.argmax.
    NaN is outside this kernel's documented rule and is not tested."""
    from diffreg_hip import lib
    for kind in TOP1_KINDS:
        conf = S.top1_conf(kind, 3, N, M, dtype)
        runs = [lib.top1_union(dv(conf)) for _ in range(2)]
        for p in range(3):
            assert same_bytes(runs[0][p], runs[1][p])
            assert torch.equal(runs[0][p].cpu(), S.top1_union_ref(conf[p])), (kind, N, M, p)


def raw_top1(conf, exact_workspace=True):
    from diffreg_hip import lib
    r = lib.raw()
    lib.ensure_init()
    c = conf.to(DEV).contiguous()
    P, N, M = c.shape
    f64 = conf.dtype == torch.float64
    out, ck_o = guarded((P, N + M, 3), torch.int64, DEV, fill=-7)
    cnt, ck_c = guarded((P,), torch.int32, DEV, fill=-5)
    wsb = r.dr_top1_union_workspace_bytes(P, N, M, 8 if f64 else 4)
    ws, ck_w = guarded((max(wsb, 16),), torch.uint8, DEV)
    code = (r.dr_top1_union_f64 if f64 else r.dr_top1_union_f32)(P, N, M, lib.ptr(c), lib.ptr(out), lib.ptr(cnt), lib.ptr(ws) if wsb else None,
                                                                 wsb, stream())
    ck_o(); ck_c(); ck_w()
    return code, out.cpu(), cnt.cpu(), wsb


@pytest.mark.parametrize("dtype", DTYPES)
def test_top1_refusal_above_the_lds_limit(dtype):
    """NaN is outside this kernel's documented rule and is not tested."""
    for N, M in ((1, 4096), (4096, 1), (2049, 2048)):
        code, out, cnt, _ = raw_top1(torch.zeros(1, N, M, dtype=dtype))
        assert code == ENOSUP and bool((out == -7).all()) and bool((cnt == -5).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,M", [(32, 70), (47, 70), (48, 65), (100, 1), (4095, 1)])
def test_top1_workspace_is_enough(N, M, dtype):
    """from 32 rows on the call takes a workspace: exactly the queried number of bytes between guard bands, and the bands stay intact.
    NaN is outside this kernel's documented rule and is not tested."""
    for kind in ("quant", "inf"):
        conf = S.top1_conf(kind, 3, N, M, dtype)
        outs = [raw_top1(conf) for _ in range(2)]
        code, out, cnt, wsb = outs[0]
        assert code == OK and wsb > 0
        for p in range(3):
            ref = S.top1_union_ref(conf[p])
            assert int(cnt[p]) == len(ref) and torch.equal(out[p, :len(ref)], ref)
            assert bool((out[p, len(ref):] == -7).all())
        assert same_bytes(outs[1][1], out) and same_bytes(outs[1][2], cnt)
