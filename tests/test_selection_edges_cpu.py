"""Keeps tests/selection_ref.py honest, without a GPU: where the reference project's rule is decided (distinct values) the plain statement
equals it and its recorded vectors; where it is not (ties, NaN, +-inf) the statement equals a rank-count restatement of the documented
rule and satisfies the invariants that hold under any tie rule."""
import itertools

import numpy as np
import pytest
import torch

from oracle import diffreg_oracle as orc
from oracle import metrics_oracle as mo
from tests import selection_ref as S
from tests.helpers import topk_case

TOPK_CASES = ["patch64_k2_thr", "ragged_k3_or", "smallest_k1", "masked_k2"]
SWITCHES = list(itertools.product((True, False), (True, False), (None, 0.5)))      # largest, mutual, threshold


@pytest.mark.parametrize("name", TOPK_CASES)
def test_topk_ref_is_the_reference_where_values_are_distinct(golden, name):
    c = topk_case(name)
    for dim in (1, 2):                                              # no tie at the k-th place of any line: torch.topk's pick is decided
        v = c["score"].sort(dim=dim, descending=c["largest"])[0]
        assert bool((v.narrow(dim, c["k"] - 1, 1) != v.narrow(dim, c["k"], 1)).all())
    got = S.mutual_topk_ref(**c)
    want = mo.batch_mutual_topk_select(c["score"], c["k"], c["row_masks"], c["col_masks"], c["largest"], c["threshold"], c["mutual"])
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    g = golden("metrics_ref")
    assert np.array_equal(torch.stack(got[:3], 1).numpy(), g["mts_" + name + "_idx"])
    assert np.array_equal(got[3].numpy(), g["mts_" + name + "_score"])


def rank_count_side(score, k, dim, largest):
    """the documented rule said another way: an entry is among the k best of its line when fewer than k entries of the line rank before
    it -- a better value, or the same value at a lower index; NaN neither ranks nor is selected"""
    s = score if dim == 2 else score.transpose(1, 2)
    a, b = s[:, :, :, None], s[:, :, None, :]                      # entry, rival
    better = (b > a) if largest else (b < a)
    L = s.shape[2]
    lower = torch.arange(L)[None, :] < torch.arange(L)[:, None]     # [entry, rival]: the rival's index is lower
    before = (better | ((b == a) & lower)) & ~torch.isnan(b)
    sel = (before.sum(3) < k) & ~torch.isnan(s)
    return sel if dim == 2 else sel.transpose(1, 2)


def test_stable_sort_puts_the_lower_index_first_by_hand():
    s = torch.tensor([[[1.0, 1.0, 1.0, 0.5], [S.NAN, 2.0, S.NAN, 2.0], [S.NAN, -S.INF, 0.0, S.NAN]]])
    assert S.topk_side(s, 2, 2, True).tolist() == [[[True, True, False, False], [False, True, False, True], [False, True, True, False]]]
    assert S.topk_side(s, 2, 2, False).tolist() == [[[True, False, False, True], [False, True, False, True], [False, True, True, False]]]
    assert S.topk_side(s, 1, 1, True).tolist() == [[[True, False, True, False], [False, True, False, True], [False, False, False, False]]]


@pytest.mark.parametrize("name", sorted(S.TOPK_EDGE_INPUTS))
def test_topk_ref_on_ties_nan_inf(name):
    score = S.topk_edge_input(name)
    B, N, M = score.shape
    finite = bool(torch.isfinite(score).all())
    rm, cm = S.topk_masks("random", B, N, M)
    for k in (1, 2, 8):
        for largest in (True, False):
            rows, cols = S.topk_side(score, k, 2, largest), S.topk_side(score, k, 1, largest)
            assert torch.equal(rows, rank_count_side(score, k, 2, largest)) and torch.equal(cols, rank_count_side(score, k, 1, largest))
            assert not (rows & torch.isnan(score)).any() and not (cols & torch.isnan(score)).any()
            if finite:                                              # exactly k row-side picks per row, k column-side picks per column
                assert bool((rows.sum(2) == k).all()) and bool((cols.sum(1) == k).all())
            else:
                numbers = ~torch.isnan(score)
                assert torch.equal(rows.sum(2), numbers.sum(2).clamp(max=k)) and torch.equal(cols.sum(1), numbers.sum(1).clamp(max=k))
    for (largest, mutual, thr), masks in itertools.product(SWITCHES, ((None, None), (rm, cm))):
        b, i, j, sc = S.mutual_topk_ref(score, 2, masks[0], masks[1], largest, thr, mutual)
        assert not torch.isnan(sc).any()
        if thr is not None:                                         # strict: an entry equal to the threshold is not kept
            assert bool((sc > thr).all() if largest else (sc < thr).all())
        if masks[0] is not None:
            assert bool(masks[0][b, i].all()) and bool(masks[1][b, j].all())
        key = (b * N + i) * M + j
        assert bool((key[1:] > key[:-1]).all())                     # strictly ascending (b, i, j)
        if finite and not mutual and thr is None and masks[0] is None:
            per_row = torch.zeros(B, N, dtype=torch.int64).index_put_((b, i), torch.ones_like(b), accumulate=True)
            assert bool((per_row >= 2).all())                       # the union holds every row's k picks


@pytest.mark.parametrize("B", [1, 255, 256, 257, 600])
def test_scan_case_counts_vary_and_some_are_empty(B):
    c = S.scan_case(B)
    b = S.mutual_topk_ref(**c)[0]
    per = torch.bincount(b, minlength=B)
    if B > 1:
        assert int((per == 0).sum()) >= 3 and per.unique().numel() >= 4
        assert int(per[256:].sum()) > 0 or B <= 256
    else:
        assert int(per[0]) > 0


def test_threshold_equals_selected_entries():
    """the threshold of the switch cases equals entries that the selection holds, so `strict` is exercised, and others pass it"""
    for largest, mutual in itertools.product((True, False), (True, False)):
        c = S.switch_case(largest)
        m = S.mutual_topk_mask(c["score"], c["k"], None, None, largest, None, mutual)
        assert int((m & (c["score"] == c["threshold"])).sum()) >= 3
        kept = S.mutual_topk_mask(c["score"], c["k"], None, None, largest, c["threshold"], mutual)
        assert int(kept.sum()) >= 3 and not (kept & (c["score"] == c["threshold"])).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_match_ref_is_the_oracle_and_the_builders_hold_what_they_promise(dtype):
    for kind, (N, M) in itertools.product(("distinct", "ties", "nan", "const"), ((1, 1), (17, 65), (200, 130))):
        conf = S.match_conf(kind, 3, N, M, dtype)
        for thr in (0.0, 0.4):
            assert torch.equal(S.mutual_match_ref(conf, thr, True), orc.mutual_match(conf, thr))
        assert torch.equal(S.mutual_match_ref(conf, 0.9, False), (conf > 0.9).nonzero())
    ties = S.mutual_match_ref(S.match_conf("ties", 3, 200, 130, dtype), 0.0)
    assert set(map(tuple, ties.tolist())) >= {(p, r, j) for p in range(3) for r in (0, 100, 199) for j in (63, 64)}
    # the NaN cases: dropping the NaN from a maximum would add matches, so a kernel that ignores NaN cannot pass
    conf = S.match_conf("nan", 3, 200, 130, dtype)
    ref = set(map(tuple, S.mutual_match_ref(conf, 0.0).tolist()))
    lenient = set(map(tuple, S.mutual_match_ref(torch.nan_to_num(conf, nan=-1.0), 0.0).tolist()))
    for e in ((0, 0, 129), (0, 2, 1), (1, 2, 1), (0, 40, 70), (2, 33, 69)):
        assert e in lenient and e not in ref


def test_top1_builders():
    for kind in ("distinct", "quant", "const", "inf"):
        c = S.top1_conf(kind, 3, 48, 65, torch.float64)
        assert not torch.isnan(c).any() and not torch.equal(c[0], c[1])
        ref = S.top1_union_ref(c[0])
        assert 65 <= len(ref) <= 48 + 65
    c = S.top1_conf("inf", 3, 48, 65, torch.float32)
    assert bool((c == -S.INF).all(2).any()) and bool((c == -S.INF).all(1).any()) and bool((c == S.INF).any())
