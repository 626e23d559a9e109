"""The float64 statement of the point-backbone primitives (tests/point_backbone_ref.py) against the restatements the project already carries, and
the margins of its input builders -- on the CPU.  The GPU file (tests/test_point_backbone_edges_gpu.py) relies on both: the kernels are held to
this reference, and the discrete decisions they take (neighbour count, nearest kernel point, first maximum, LeakyReLU's sign) are decided away from
float32 ties by the builders, which this file proves for every parametrised case."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import kpfcn_oracle as ko
from tests import pcd_backbone2d3d_ref as P2
from tests import point_backbone_ref as R


def only_ns(idx, Ns):
    """the older restatements know one shadow id: Ns"""
    return torch.where((idx < 0) | (idx >= Ns), torch.full_like(idx, Ns), idx)


@pytest.mark.parametrize("influence,aggregation", R.MODE_CASES)
def test_kpconv_weighted_is_the_oracles_kpconv(influence, aggregation):
    """oracle kpconv (float64) = (weighted @ W2^T) of this file's statement, W2[co][k Cin + c] = weights[k][c][co]; Cin 5, K 15, H 9 and the mode case"""
    for c in (R.kpconv_case(5, 9, 15, "mixed", Nq=61, Ns=80, seed=9), R.mode_case()):
        K, Cin = c["kp"].shape[0], c["x"].shape[1]
        Wk = R.T(R.synth.hash_uniform(10, Cin, (K, Cin, 7)))
        ref = ko.kpconv(c["q"].double(), c["s"].double(), only_ns(c["idx"], len(c["s"])), c["x"].double(), Wk, c["kp"].double(), c["extent"], influence,
                        aggregation)
        wf, counts = R.kpconv_weighted(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"], influence, aggregation)
        assert torch.equal(counts, c["counts"])
        got = wf @ Wk.permute(2, 0, 1).reshape(7, -1).t()
        assert R.rel_dev(got, ref) <= 1e-13
        un, _ = R.kpconv_weighted(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"], influence, aggregation, normalise=False)
        assert torch.equal(wf, un / counts.clamp(min=1)[:, None])


def test_norm_and_pools_are_the_oracles():
    c = R.norm_case(257, 31)
    for form in ("a", "ab_norm", "ab_id"):
        a, b = c["a_" + form].double(), c["b_" + form].double()
        want = {"a": ko.norm_block(a), "ab_norm": ko.norm_block(a) + ko.norm_block(b), "ab_id": ko.norm_block(a) + b}[form]
        assert R.rel_dev(R.norm_block64(a, b, form, activate=False), want) <= 1e-13
        assert R.rel_dev(R.norm_block64(a, b, form), F.leaky_relu(want, 0.1)) <= 1e-13
    assert R.rel_dev(R.norm_block64(c["a_a"], None, "a_noact"), ko.norm_block(c["a_a"].double())) <= 1e-13
    for case in R.POOL_CASES:
        p = R.pool_case(*case)
        H = case[1]
        inds = p["inds"][:, :H]
        assert torch.equal(R.max_pool64(p["x"], inds), ko.max_pool(p["x"].double(), only_ns(inds, p["n1"])))
        assert torch.equal(R.closest_pool64(p["x"], inds), ko.closest_pool(p["x"].double(), only_ns(inds, p["n1"])))


def test_max_pool_gradient_goes_to_the_first_maximum():
    """two bit-equal rows listed as (a, b) and as (b, a): the first listed takes the whole gradient; a shadow that wins takes it away"""
    p = R.pool_case(300, 17, 96, 17)
    x = p["x"].double().requires_grad_(True)
    inds = p["inds"]
    (R.max_pool64(x, inds) * p["G"].double()).sum().backward()
    n1 = p["n1"]
    only = torch.zeros(2, 17, dtype=torch.long) + n1
    only[0, :2] = torch.tensor([n1 - 1, n1 - 2])
    only[1, :2] = torch.tensor([n1 - 2, n1 - 1])
    y = p["x"].double().requires_grad_(True)
    R.max_pool64(y, only).sum().backward()
    pos = (p["x"][n1 - 1] > 0).double()                              # the shadow's zero wins over negative entries
    assert torch.equal(y.grad[n1 - 1], pos) and torch.equal(y.grad[n1 - 2], pos)
    z = p["x"].double().requires_grad_(True)
    R.max_pool64(z, only[:1]).sum().backward()
    assert torch.equal(z.grad[n1 - 1], pos) and not z.grad[n1 - 2].any()
    assert not x.grad[:max(1, n1 // 4)][:, :].isnan().any()


@pytest.mark.parametrize("C,H", [(5, 3), (64, 1)])
def test_knn_interpolate_is_the_restatement(C, H):
    c = R.knn_case(C, H, Nq=200, Ns=150)
    got = R.knn_interpolate64(c["q"], c["s"], c["x"], c["idx"])
    want = P2.knn_interpolate(c["q"].double(), c["s"].double(), c["x"].double(), only_ns(c["idx"], len(c["s"])))
    assert R.rel_dev(got, want) <= 1e-13
    # a coincident support takes the whole weight to within 1e-8 / d^2 of the others
    assert R.rel_dev(got[10:20], c["x"].double()[c["idx"][10:20, 0]]) <= 1e-5


@pytest.mark.parametrize("case", R.KPCONV_CASES, ids=R.kpconv_id)
def test_kpconv_builder_margins(case):
    """the builder's own assertions (feature sums >= 0.5 from zero, a quarter negative, a query of count 0, the all-shadow band, every shadow kind)
    pass, and the reference's counts are the builder's"""
    cin, H, K, shadow = case
    c = R.kpconv_case(cin, H, K, shadow)
    Ns = len(c["s"])
    assert tuple(c["idx"].shape) == (1029, H) and Ns == 500 and 1029 % 4 == 1
    kinds = {"ns": {Ns}, "beyond": {Ns + 7}, "neg": {-1}, "mixed": {Ns, Ns + 7, -1}}[shadow]
    bad = c["idx"][(c["idx"] < 0) | (c["idx"] >= Ns)]
    assert set(bad.unique().tolist()) == kinds
    if cin <= 65:                                                    # the reference's counts at the sizes the CPU does in a moment
        assert torch.equal(R.kpconv_weighted(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"])[1], c["counts"])
    assert int(c["counts"][c["qneg"]]) == 0 and not c["counts"][-5:].any()


def test_closest_margin_and_the_mirror_tie():
    """every real (query, neighbour) pair of the mode case has its two nearest kernel points >= 1e-4 extent apart -- all of them, no pair left out --
    except the planted one, whose two nearest are kernel points 1 and 2 at bit-equal distance (float32 and float64)"""
    c = R.mode_case()
    gap, tie_gap = R.closest_margin(c)
    assert gap >= 1e-4, gap
    assert tie_gap == 0.0
    qi, hi = c["tie"]
    for dt in (torch.float32, torch.float64):
        rel = (c["s"][c["idx"][qi, hi]].to(dt) - c["q"][qi].to(dt))
        d2 = ((rel - c["kp"].to(dt)) ** 2).sum(1)
        assert d2[1] == d2[2] == d2.min() and int(torch.argmin(d2)) == 1
    wf, _ = R.kpconv_weighted(c["q"], c["s"], c["idx"], c["x"], c["kp"], c["extent"], "constant", "closest", normalise=False)
    Cin = c["x"].shape[1]
    lone = c["idx"][qi].clone()
    lone[1:] = len(c["s"])
    w1, _ = R.kpconv_weighted(c["q"][qi:qi + 1], c["s"], lone[None], c["x"], c["kp"], c["extent"], "constant", "closest", normalise=False)
    assert torch.equal(w1[0, Cin:2 * Cin], c["x"][0].double()) and not w1[0, 2 * Cin:3 * Cin].any()


@pytest.mark.parametrize("case", R.NORM_CASES, ids=R.norm_id)
def test_norm_builder_margins(case):
    N, C = case
    c = R.norm_case(N, C)                                            # asserts the sign margin of every activated form
    R_, rows_per = R.slabs_of(N)
    assert R_ == {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 1027: 5, 16385: 64, 16447: 64}[N]
    if case == R.NORM_SPECIAL:
        a = c["a_a"].double()
        assert a[:, 0].var() == 0 and abs(a[:, -1].mean() - 1e4) < 0.2 and 0.8 < a[:, -1].std() < 1.2
        _, _, rstd = R.xhat64(a)
        assert rstd[0] == 1 / math.sqrt(1e-5)
    if N == 1:
        for form in ("a", "ab_norm"):
            assert not R.norm_pre64(c["a_" + form], c["b_" + form], form).any()


def test_leaky_zero_builder():
    c = R.leaky_zero_case()
    assert int(c["zeros"].sum()) == 16
    for form in ("a", "ab_id"):
        a = c["a"].double().requires_grad_(True)
        b = c["b"].double().requires_grad_(True)
        out = R.norm_block64(a, b, form)
        assert bool((out[c["zeros"]] == 0).all())
        (out * c["G"].double()).sum().backward()
        if form == "ab_id":                                          # torch's LeakyReLU backward takes the slope at exactly 0
            assert torch.equal(b.grad[c["zeros"]], c["G"].double()[c["zeros"]] * R.SLOPE)
    # the float32 mean of the built columns is 0.5 whatever the order of the sum
    assert bool((c["a"][:, :4].double().sum(0) == 0.5 * c["a"].shape[0]).all())


@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.pool_id)
def test_pool_builder(case):
    n2, H, d, ld = case
    p = R.pool_case(*case)
    inds, n1 = p["inds"][:, :H], p["n1"]
    assert tuple(p["inds"].shape) == (n2, ld) and tuple(p["x"].shape) == (n1, d)
    out = R.max_pool64(p["x"], inds)
    if n2 >= 8:
        real = (inds >= 0) & (inds < n1)
        assert (~real).all(1).sum() >= 2 and not out[(~real).all(1)].any()
        assert bool((out[2] < 0).all()) and not out[3].any()
        assert torch.equal(out[4], out[5])
        assert set(inds[~real].unique().tolist()) == {n1, n1 + 7, -1}
        if H > 1:
            assert inds[6, 0] == inds[6, 1]
    vals = torch.cat((p["x"].double(), torch.zeros(1, d, dtype=torch.float64)), 0)[only_ns(inds, n1)]
    top = vals.sort(1, descending=True)[0]
    if H > 1:
        gaps = top[:, 0] - top[:, 1]
        assert bool(((gaps == 0) | (gaps >= 1e-3)).all())


@pytest.mark.parametrize("case", R.KNN_CASES, ids=R.knn_id)
def test_knn_builder(case):
    c = R.knn_case(*case)
    assert tuple(c["idx"].shape) == (1029, case[1])
    d2 = ((c["q"][10:20].double() - c["s"].double()[c["idx"][10:20, 0]]) ** 2).sum(1)
    assert not d2.any()


def test_case_lists_cover_the_issue():
    assert {c[0] for c in R.KPCONV_CASES} == set(R.KP_CIN) and {(c[1], c[2]) for c in R.KPCONV_CASES} == set(R.KP_HK)
    for cin in R.KP_CIN:
        assert sum(c[0] == cin for c in R.KPCONV_CASES) >= 2
    for hk in R.KP_HK:
        assert sum((c[1], c[2]) == hk for c in R.KPCONV_CASES) >= 2
        assert {R.cpl_of(c[0]) for c in R.KPCONV_CASES if (c[1], c[2]) == hk} == {1, 2, 4, 8}
    assert {c[3] for c in R.KPCONV_CASES} == set(R.SHADOW_KINDS) and 18 <= len(R.KPCONV_CASES) <= 22
    assert {c[0] for c in R.NORM_CASES} == set(R.NORM_N) and {c[1] for c in R.NORM_CASES} == set(R.NORM_C)
    assert [c for c in R.NORM_CASES if c[0] == 16447] == [(16447, 33)] and R.NORM_SPECIAL in R.NORM_CASES
    assert {R.slabs_of(c[0])[0] for c in R.NORM_CASES} >= {1, 2, 64}
    assert max(c[0] * (c[1] + 5) * 4 for c in R.NORM_CASES) < 3e6
    assert any(R.slabs_of(c[0])[1] % 8 for c in R.NORM_CASES)
    assert {(c[0], c[1], c[2]) for c in R.POOL_CASES} == set(R.POOL_SHAPES) and {c[3] - c[1] for c in R.POOL_CASES} == {0, 3}
    assert set(R.KNN_CASES) == {(c, h) for c in R.KNN_C for h in R.KNN_H}
    ids = " ".join(map(R.kpconv_id, R.KPCONV_CASES))
    assert all(("cpl%d" % k) in ids for k in (1, 2, 4, 8)) and all(("shadow_" + s) in ids for s in R.SHADOW_KINDS)
