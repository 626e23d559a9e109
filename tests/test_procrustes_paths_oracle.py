"""CPU checks of tests/procrustes_ref.py, the float64 reference and the host mirrors that test_procrustes_paths_gpu.py leans on:
fit64 and expected_set agree with the oracle where the oracle is decided (distinct values), and every case of the GPU file's table reaches
the selection branch and the launch form it names.  The size rules below are copied from csrc/procrustes.hip on purpose: a change of
the kernel's thresholds must be met by a change of this table, not absorbed by it."""
import numpy as np
import pytest
import torch

from oracle import diffreg_oracle as orc
from tests import procrustes_ref as pr


@pytest.mark.parametrize("N,M,rate", [(40, 56, 1.0), (128, 128, 1.0), (64, 64, 20.0), (300, 70, 0.3)])
def test_fit64_and_expected_set_agree_with_the_oracle_on_distinct_tiles(N, M, rate):
    K = pr.pair_k(N, M, rate)
    conf = pr.tile("distinct", N, M, K, seed=N + M)
    g = torch.Generator().manual_seed(N)
    src, tgt = torch.rand(N, 3, generator=g), torch.rand(M, 3, generator=g)
    w, i, j = orc.topk_pairs(conf[None], K)
    want = pr.expected_set(conf, K)
    assert torch.equal((i[0] * M + j[0]).sort()[0], want)
    ones = torch.ones(1, N, dtype=torch.bool), torch.ones(1, M, dtype=torch.bool)
    R, t, _, _, cond, _ = orc.procrustes(conf[None], src[None], tgt[None], ones[0], ones[1], rate, 1e9)
    f = pr.fit64(conf.numpy(), src.numpy(), tgt.numpy(), want.numpy())
    # the oracle's own float32 level: mean, centring and the 3 x 3 product in float32 on O(1) data, amplified by the fit's conditioning
    tol = 2e-6 * max(1.0, f.cond)
    assert np.abs(R[0].double().numpy() - f.R).max() < tol
    assert np.abs(t[0, :, 0].double().numpy() - f.t).max() < tol
    assert abs(float(cond[0]) / f.cond - 1.0) < tol
    assert abs(np.linalg.det(f.R) - 1.0) < 1e-12 and np.abs(f.R.T @ f.R - np.eye(3)).max() < 1e-12
    # the yardstick of the GPU file is the same arithmetic
    Ro, to, co = pr.oracle_fit(conf, src, tgt, want)
    assert np.abs(Ro - R[0].double().numpy()).max() < tol and np.abs(to - t[0, :, 0].double().numpy()).max() < tol


def test_expected_set_takes_the_lowest_indices_among_ties():
    conf = torch.tensor([[0.5, 0.25, 0.5], [0.25, 0.5, 0.25], [0.25, 0.0, 0.5]])
    assert pr.expected_set(conf, 2).tolist() == [0, 2]
    assert pr.expected_set(conf, 5).tolist() == [0, 1, 2, 4, 8]
    assert pr.expected_set(conf, 6).tolist() == [0, 1, 2, 3, 4, 8]
    assert pr.expected_set(torch.zeros(4, 4), 3).tolist() == [0, 1, 2]


def test_k_is_the_oracles():
    for case in pr.SELECTION_CASES:
        (N, M), _, rate = case[:3]
        want = int((torch.maximum(torch.full((1,), float(N)), torch.full((1,), float(M))) * rate).int())
        assert pr.pair_k(N, M, rate) == min(want, N * M, pr.PK_MAX), case
        assert want <= pr.PK_MAX, "the entry refuses this K (DR_ENOSUP)"
    assert pr.pair_k(5, 7, 20.0) == 35 and pr.pair_k(64, 64, 20.0) == 1280 and pr.pair_k(2064, 4096, 1.0) == 4096


@pytest.mark.parametrize("case", pr.SELECTION_CASES, ids=pr.case_id)
def test_selection_case_reaches_its_branch(case):
    (N, M), kind, rate, want, want_flat = case
    K = pr.pair_k(N, M, rate)
    conf, _, _ = pr.selection_batch(case)
    assert not torch.equal(conf[0], conf[2])
    if want is None:
        assert pr.launch_form(3, N, M) == 1
        return
    assert pr.launch_form(3, N, M) == 0
    assert [pr.reg_branch(conf[b], K) for b in range(3)] == [want, want_flat, want]
    if kind == "sparse":
        assert int((conf[0] != 0).sum()) < K                     # ties fall among the +0.0 entries
    if kind in ("quantised", "flat", "sparse") and K < N * M:
        top = conf[0].reshape(-1).topk(K)[0]
        assert int((conf[0] == top[-1]).sum()) > int((top == top[-1]).sum()), "no surplus of ties at the K-th value"
    if kind == "sharp_on_quantised":
        assert int((conf[0] >= 0.5).sum()) == K and conf[0][conf[0] >= 0.5].unique().numel() == K


def test_case_table_populates_every_branch_and_form():
    by_kind = {}
    list_more = False
    for case in pr.SELECTION_CASES:
        (N, M), kind, rate, want, want_flat = case
        if want is None or not 4096 < N * M <= pr.REG_MAX:
            continue
        by_kind.setdefault(kind, set()).add(want)
        if want == "list":
            conf, _, _ = pr.selection_batch(case)
            K = pr.pair_k(N, M, rate)
            list_more |= pr.reg_candidates(conf[0], K)[1] > K
    # what each kind can reach on a tile of more than 4096 entries: distinct random values never overflow the list (about 1.2 K candidates),
    # a flat or sparse tile always does (every entry reaches L)
    assert by_kind == {"distinct": {"list", "k_gt_1024"}, "quantised": {"list", "bisect", "k_gt_1024"}, "flat": {"bisect", "k_gt_1024"},
                       "sparse": {"bisect", "k_gt_1024"}, "sharp_on_quantised": {"list", "bisect", "k_gt_1024"}}
    assert list_more
    assert {c[3] for c in pr.SELECTION_CASES} >= {"all", "k_gt_1024", "list", "bisect", None}
    # the long-slice tile and the per-pair-K tiles
    assert pr.slice_len(1, 2064 * 4096) == 33792 and pr.launch_form(1, 2064, 4096) == 2 and pr.pair_k(2064, 4096, 1.0) == pr.PK_MAX
    assert pr.launch_form(4, 96, 80) == 0 and pr.launch_form(4, 300, 400) == 1
    # the scalar arm by both causes
    assert all(c == {"nm", "ptr"} or c == {"nm"} for c in pr.scalar_arm(3, 127, 129)) and pr.scalar_arm(3, 127, 129)[1] == {"nm", "ptr"}
    assert pr.scalar_arm(1, 128, 128, base_ptr=4) == [{"ptr"}] and pr.scalar_arm(3, 128, 128) == [set(), set(), set()]


@pytest.mark.parametrize("N,M", pr.GEOM_TILES)
def test_geometry_cases_are_what_they_claim(N, M):
    K = pr.pair_k(N, M, pr.GEOM_RATE)
    assert K == max(N, M) // 2
    for name, (X, Y, w, group) in pr.geometry_cases(K, seed=N).items():
        conf, src, tgt, match = pr.matching_tile(N, M, X, Y, w, seed=N + len(name))
        assert torch.equal(pr.expected_set(conf, K), match), name
        f = pr.fit64(conf.numpy(), src.numpy(), tgt.numpy(), match.numpy())
        if (N, M) == (64, 64):
            assert pr.reg_branch(conf, K) == "list" and pr.reg_candidates(conf, K)[1] == K, name      # exactly K candidates
        if group == "reflection":
            assert f.det_uv < 0 and abs(np.linalg.det(f.R) - 1.0) < 1e-12
        elif group == "equal_sv":
            two = name.startswith("two")
            assert abs(f.S[1] / f.S[2] - 1.0) < 1e-6 and (abs(f.S[0] / f.S[1] - (4.0 if two else 1.0)) < 1e-5), (name, f.S)
        elif group == "deficient":
            assert f.S[2] <= 1e-7 * f.S[0], (name, f.S)
            if name.startswith("collinear"):
                assert f.S[1] <= 1e-7 * f.S[0], (name, f.S)
        elif group == "near_coplanar":
            assert 1e3 < f.cond < 1e6, f.cond
        elif group == "far":
            assert float(src[match // M].abs().min()) > 990.0 and float(tgt[match % M].abs().min()) > 990.0
        if group in ("motion", "far", "weights", "equal_sv", "near_coplanar"):
            R0 = {"motion_1e-4rad": pr.rotation([1, 2, 3], 1e-4), "motion_90deg": pr.rotation([1, 2, 3], np.pi / 2),
                  "motion_180deg": pr.rotation([1, 2, 3], np.pi)}.get(name, pr.R_RANDOM if "axis" not in name else pr.rotation([0, 0, 1], np.pi / 2))
            # float32 points of a cloud at 1e3 carry 6e-5 of rounding against 0.3 of extent
            assert np.abs(f.R - R0).max() < (1e-3 if group in ("far", "near_coplanar") else 1e-6), (name, np.abs(f.R - R0).max())
        if group not in ("deficient", "near_coplanar"):
            assert f.cond < 200.0, (name, f.cond)
