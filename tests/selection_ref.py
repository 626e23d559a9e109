"""Plain statements, in torch on the CPU, of the three read-out / selection rules of csrc/stateops.hip, and the input builders that
tests/test_selection_edges_cpu.py and tests/test_selection_edges_gpu.py share.  Nothing here calls the library.

  mutual_topk_ref   dr_mutual_topk_select_f32: batch_mutual_topk_select (oracle/metrics_oracle.py:178-193) with the kernel's documented
                    tie rule in place of torch.topk's unspecified one
  mutual_match_ref  dr_mutual_match_f32 / _f64: oracle.diffreg_oracle.mutual_match, extended with mutual=False
  top1_union_ref    dr_top1_union_f32 / _f64: oracle.diffreg_oracle.top1_union itself
"""
import functools

import numpy as np
import torch

from diffreg_hip import synth
from oracle.diffreg_oracle import top1_union as top1_union_ref  # noqa: F401  (imported, not restated)

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------
# the rules
# ------------------------------------------------------------------------------------------------
def topk_side(score, k, dim, largest):
    """bool [B,N,M]: the k best entries of every row (dim = 2) or column (dim = 1).  The k best are the first k of a stable sort by
    value, so the lower index wins among equals; NaN ranks after everything and is never selected (a row with fewer than k numbers
    selects them all)."""
    nan = torch.isnan(score)
    by_value = torch.where(nan, torch.zeros_like(score), score).sort(dim=dim, descending=largest, stable=True)[1]
    nan_last = nan.gather(dim, by_value).to(torch.uint8).sort(dim=dim, stable=True)[1]      # stable: the value order survives
    order = by_value.gather(dim, nan_last)
    sel = torch.zeros_like(score, dtype=torch.bool)
    sel.scatter_(dim, order.narrow(dim, 0, k), True)
    return sel & ~nan


def mutual_topk_mask(score, k, row_masks=None, col_masks=None, largest=True, threshold=None, mutual=True):
    rows, cols = topk_side(score, k, 2, largest), topk_side(score, k, 1, largest)
    corr = (rows & cols) if mutual else (rows | cols)
    if threshold is not None:                               # threshold and masks act on the selection, not on the scores; strict
        corr = corr & (score > threshold if largest else score < threshold)
    if row_masks is not None:
        corr = corr & row_masks.bool()[:, :, None]
    if col_masks is not None:
        corr = corr & col_masks.bool()[:, None, :]
    return corr


def mutual_topk_ref(score, k, row_masks=None, col_masks=None, largest=True, threshold=None, mutual=True):
    """score [B,N,M] float32 -> (b, i, j, score) in torch.nonzero order"""
    b, i, j = torch.nonzero(mutual_topk_mask(score, k, row_masks, col_masks, largest, threshold, mutual), as_tuple=True)
    return b, i, j, score[b, i, j]


def mutual_match_mask(conf, thr, mutual=True):
    m = conf > thr
    if mutual:                                              # torch.max propagates NaN: a row / column holding one has no match
        m = m & (conf == conf.max(2, keepdim=True)[0]) & (conf == conf.max(1, keepdim=True)[0])
    return m


def mutual_match_ref(conf, thr, mutual=True):
    """conf [P,N,M] -> int64 [K,3] rows (p, i, j) in nonzero() order: > thr and, with mutual, equal to the row and the column maximum"""
    return mutual_match_mask(conf, thr, mutual).nonzero()


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _u01(seed, shape):
    n = int(np.prod(shape))
    return torch.from_numpy(synth.hash_u01(seed, 7, n).reshape(shape))


def u01(seed, shape, dtype=torch.float32):
    """hash-generated values in (0, 1); a fresh tensor"""
    return _u01(seed, tuple(shape)).to(dtype, copy=True)


def quantise(x, levels=8):
    return torch.floor(x * levels) / levels                 # multiples of 1 / 8: exact in every float type


def scan_case(B):
    """B x 8 x 8, k = 2, mutual, threshold 0.5: the scores of element b are scaled by one of five amplitudes, so the number of
    selected entries beyond the threshold varies from element to element and every fifth element has none"""
    amp = 0.4 + 0.15 * ((torch.arange(B) * 7 + 4) % 5).float()      # 1, .55, .85, .4 (nothing passes 0.5), .7, ...
    return dict(score=u01(11, (B, 8, 8)) * amp[:, None, None], k=2, largest=True, threshold=0.5, mutual=True)


def switch_case(largest):
    """4 x 16 x 24 at 8 levels, k = 4: the four best of a line span two or three levels, and the threshold IS the second level from the
    selected end, so several selected entries equal it exactly (the comparison is strict: they are not kept) while the entries of the
    outermost level pass"""
    return dict(score=quantise(u01(21, (4, 16, 24))), k=4, largest=largest, threshold=0.75 if largest else 0.125)


def topk_scores(kind, B, N, M, seed=3):
    """score matrices for the top-k selection: `distinct` (cosine-like), `quant` (8 levels: ties everywhere), `const`, `nan` (scattered
    NaN, an all-NaN row and an all-NaN column), `inf` (+inf / -inf entries among 8 levels, a row of -inf and a column of +inf)"""
    u = u01(seed + 1000 * N + M, (B, N, M))
    if kind == "distinct":
        return 2 * u - 1
    if kind == "quant":
        return quantise(u)
    if kind == "const":
        return torch.full((B, N, M), 0.25)
    pick = u01(seed + 77, (B, N, M))
    if kind == "nan":
        s = (2 * u - 1).masked_fill(pick < 0.12, NAN)
        s[0, N // 2, :] = NAN
        s[B - 1, :, M // 3] = NAN
        return s
    if kind == "inf":
        s = quantise(u).masked_fill(pick < 0.06, INF).masked_fill(pick > 0.94, -INF)
        s[0, N // 3, :] = -INF
        s[B - 1, :, M // 2] = INF
        return s
    raise KeyError(kind)


def topk_masks(kind, B, N, M, seed=5):
    """(row_masks, col_masks) bool or None: `random`, `empty_row_mask` (all false for element 1), `one_col` (a single true column per
    element), `rows_only` / `cols_only` (None on the other side)"""
    rm = u01(seed, (B, N)) > 0.3
    cm = u01(seed + 1, (B, M)) > 0.3
    if kind == "random":
        return rm, cm
    if kind == "empty_row_mask":
        rm[1 % B] = False
        return rm, cm
    if kind == "one_col":
        cm = torch.zeros(B, M, dtype=torch.bool)
        cm[torch.arange(B), (torch.arange(B) * 5 + M - 1) % M] = True
        return rm, cm
    if kind == "rows_only":
        return rm, None
    if kind == "cols_only":
        return None, cm
    raise KeyError(kind)


# every tie / NaN / inf input of the GPU file: name -> (kind, B, N, M)
TOPK_EDGE_INPUTS = {"quant_40x40": ("quant", 3, 40, 40), "quant_63x65": ("quant", 3, 63, 65), "const_40x40": ("const", 2, 40, 40),
                    "const_63x65": ("const", 2, 63, 65), "nan_40x40": ("nan", 3, 40, 40), "nan_63x65": ("nan", 3, 63, 65),
                    "inf_40x40": ("inf", 3, 40, 40), "inf_63x65": ("inf", 3, 63, 65)}


def topk_edge_input(name):
    kind, B, N, M = TOPK_EDGE_INPUTS[name]
    return topk_scores(kind, B, N, M)


def match_conf(kind, P, N, M, dtype, seed=9):
    """confidence matrices for the mutual read-out.  `distinct`: values in (0, 1).  `ties`: in three rows the value 2 stands in two
    columns -- 63 and 64 where the matrix has them, the first and the last otherwise -- so every one of them equals its row and its
    column maximum.  `nan`: a NaN in the corner of every pair with a value in its column that would match if the NaN were dropped,
    and single NaNs that share a column / a row with such a value.  `const`: every entry is a row and a column maximum."""
    c = u01(seed + 1000 * N + M, (P, N, M), dtype)
    if kind == "distinct":
        return c
    if kind == "const":
        return torch.full((P, N, M), 0.5, dtype=dtype)
    if kind == "ties":
        cols = (63, 64) if M >= 65 else (0, M - 1)
        for r in {0, N // 2, N - 1}:
            for j in cols:
                c[:, r, j] = 2.0
        return c
    if kind == "nan":
        c[:, N - 1, M - 1] = NAN
        if N >= 2:
            c[:, 0, M - 1] = 3.0                             # the maximum of row 0; its column holds the corner's NaN
        if N >= 4 and M >= 4:
            c[0, 1, 1] = NAN; c[0, 2, 1] = 4.0               # NaN in a column: (2, 1) is no match
            c[1 % P, 2, 2] = NAN; c[1 % P, 2, 1] = 4.0       # NaN in a row: (2, 1) is no match
        if N >= 41 and M >= 71:
            c[0, 17, 70] = NAN; c[0, 40, 70] = 5.0           # past the first 16 rows and the first 64 columns
            c[2 % P, 33, 3] = NAN; c[2 % P, 33, 69] = 5.0
        return c
    raise KeyError(kind)


def top1_conf(kind, P, N, M, dtype, seed=13):
    """tiles for the top-1 union, a different one per pair: `distinct`, `quant` (8 levels), `const`, `inf` (whole rows and columns of
    -inf, single +inf entries).  No NaN: the kernel's rule does not cover it."""
    c = u01(seed + 1000 * N + M, (P, N, M), dtype)
    if kind == "distinct":
        return c
    if kind == "quant":
        return quantise(c)
    if kind == "const":
        return torch.full((P, N, M), -1.5, dtype=dtype) * torch.arange(1, P + 1, dtype=dtype)[:, None, None]
    if kind == "inf":
        c = quantise(c)
        for p in range(P):
            c[p, (3 * p + N // 2) % N, :] = -INF
            c[p, :, (5 * p + M // 3) % M] = -INF
            c[p, (7 * p + N - 1) % N, (p + M // 2) % M] = INF
            c[p, p % N, (M - 1 - p) % M] = INF
        return c
    raise KeyError(kind)
