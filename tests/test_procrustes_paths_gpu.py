"""The Procrustes fit (csrc/procrustes.hip, svd3.h) held to float64 on every selection path and SVD edge.  Needs a GPU.

Selection is index work and is checked exactly: no index twice, the selected values are torch.topk's bit for bit, and among the entries equal
to the K-th value exactly the lowest flat indices are taken (include/diffreg_hip.h) -- on every launch form (dr_debug_procrustes_last_form)
and every branch of the one-workgroup kernel (tests/procrustes_ref.py::reg_branch, an input condition asserted before anything else).

The fit is compared with tests/procrustes_ref.py::fit64 on the device's OWN selected set.  Yardstick: the reference's float32 arithmetic
(oracle kabsch) on the same set; its deviation e_ref from fit64 is computed here and the bars are max(4 e_ref, floor) with the floors of
test_ops_gpu.py::test_procrustes (R 1e-5; t 1e-5 x the largest |coordinate|; cond 1e-4 relative, where cond < 1e4).  Every pair of every case:
|R^T R - I| and |det R - 1| <= 1e-6 (six float32 roundings of 6e-8 on unit-size entries, with margin), (Rf, tf) = (R, t) bit for bit or
(I, 0) according to ok, ok = (cond < max_cond), and a second call gives the same bits and the same set."""
import numpy as np
import pytest
import torch

from oracle import diffreg_oracle as orc
from tests import procrustes_ref as pr
from tests.helpers import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DR_ENOSUP = -3

SEEN = {"form": set(), "branch": set(), "scalar": set(), "k": set(), "guarded_form": set(), "list": set()}
RATIOS = {}                       # group -> (largest device error / bar, what, error, e_ref, bar)


def last_form():
    from diffreg_hip import lib
    return int(lib.raw().dr_debug_procrustes_last_form())


def call(conf_dev, src, tgt, rate, max_cond, sm=None, tm=None, use_len=False, guard=False, prefill=None):
    """one dr_procrustes_f32 -> (rc, form, dict of CPU tensors R [P,3,3], t [P,3], Rf, tf, cond, ok, idx [P,K_fixed]).  guard=False: through the
    wrapper (its zero-filled idx).  guard=True: the raw entry, every buffer it writes between guard bands; prefill: a value the float
    outputs start from (ok and idx start from -7 then)"""
    from diffreg_hip import lib
    P, N, M = conf_dev.shape
    if not guard:
        R, t, Rf, tf, cond, ok, idx = lib.procrustes(conf_dev, src.to(DEV), tgt.to(DEV), sm.to(DEV) if sm is not None else None,
                                                     tm.to(DEV) if tm is not None else None, rate, max_cond, use_mask_len=use_len, want_topk=True)
        form = last_form()
        return 0, form, dict(R=R.cpu(), t=t.cpu()[:, :, 0], Rf=Rf.cpu(), tf=tf.cpu()[:, :, 0], cond=cond.cpu(), ok=ok.cpu(), idx=idx.cpu())
    K_fixed = int(float(torch.tensor(float(max(N, M)), dtype=torch.float32) * rate))
    bufs, checks = {}, []
    for name, shape, dtype in (("R", (P, 3, 3), torch.float32), ("t", (P, 3), torch.float32), ("Rf", (P, 3, 3), torch.float32),
                               ("tf", (P, 3), torch.float32), ("cond", (P,), torch.float64), ("ok", (P,), torch.int32),
                               ("idx", (P, K_fixed), torch.int32)):
        fill = (prefill if dtype.is_floating_point else -7) if prefill is not None else (0 if name == "idx" else None)
        bufs[name], chk = guarded(shape, dtype, DEV, fill=fill)
        checks.append(chk)
    wsb = lib.raw().dr_procrustes_workspace_bytes(P, N, M)
    ws = None
    if wsb:
        ws, chk = guarded((wsb,), torch.uint8, DEV)
        checks.append(chk)
    s, g = src.to(DEV).contiguous(), tgt.to(DEV).contiguous()
    smu = lib.mask_u8(sm.to(DEV)) if sm is not None else None
    tmu = lib.mask_u8(tm.to(DEV)) if tm is not None else None
    rc = lib.raw().dr_procrustes_f32(P, N, M, lib.ptr(conf_dev), lib.ptr(s), lib.ptr(g), lib.ptr(smu), lib.ptr(tmu), 1 if use_len else 0,
                                     float(rate), float(max_cond), lib.ptr(bufs["R"]), lib.ptr(bufs["t"]), lib.ptr(bufs["Rf"]),
                                     lib.ptr(bufs["tf"]), lib.ptr(bufs["cond"]), lib.ptr(bufs["ok"]), lib.ptr(bufs["idx"]), lib.ptr(ws), wsb,
                                     lib.stream_of(conf_dev))
    form = last_form()
    for chk in checks:
        chk()
    out = {k: v.cpu().clone() for k, v in bufs.items()}
    if prefill is None:
        out["ok"] = out["ok"].bool()
    return rc, form, out


def bits(x):
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32)


def same_result(a, b, Ks):
    for k in ("R", "t", "Rf", "tf", "cond"):
        assert torch.equal(bits(a[k]), bits(b[k])), "a second call changed " + k
    assert torch.equal(a["ok"], b["ok"])
    for p, K in enumerate(Ks):
        assert torch.equal(a["idx"][p, :K].sort()[0], b["idx"][p, :K].sort()[0]), "a second call selected another set"


def check_selection(conf_b, idx_row, K):
    """the four selection assertions of one pair"""
    flat = conf_b.reshape(-1)
    got = idx_row[:K].long()
    assert bool((idx_row[K:] == 0).all()), "the tail of topk_idx was written"
    assert got.numel() == K and (K == 0 or (int(got.min()) >= 0 and int(got.max()) < flat.numel()))
    assert got.unique().numel() == K, "an index was selected twice"
    if K == 0:
        return
    top = flat.topk(K)[0]
    assert torch.equal(bits(flat[got].sort(descending=True)[0]), bits(top)), "the selected values are not the K largest"
    kth = top[-1]
    n_ties = int((top == kth).sum())
    tie_idx = (flat == kth).nonzero()[:, 0][:n_ties]
    took = got[flat[got] == kth].sort()[0]
    assert torch.equal(took, tie_idx), "ties at the K-th value: not the lowest flat indices (first differing: %s)" % (
        [(int(a), int(b)) for a, b in zip(took, tie_idx) if a != b][:4],)
    assert torch.equal(got.sort()[0], pr.expected_set(conf_b, K))


def check_invariants(what, out, p, max_cond):
    R, t = out["R"][p], out["t"][p]
    assert bool(torch.isfinite(R).all()) and bool(torch.isfinite(t).all()), (what, "R or t is not finite")
    R64 = R.double().numpy()
    orth, det = np.abs(R64.T @ R64 - np.eye(3)).max(), abs(np.linalg.det(R64) - 1.0)
    assert orth <= 1e-6 and det <= 1e-6, (what, "R is no rotation", orth, det, R64)
    ok, cond = bool(out["ok"][p]), float(out["cond"][p])
    assert ok == (cond < float(np.float32(max_cond))), (what, ok, cond, max_cond)
    if ok:
        assert torch.equal(bits(out["Rf"][p]), bits(R)) and torch.equal(bits(out["tf"][p]), bits(t)), what
    else:
        assert torch.equal(out["Rf"][p], torch.eye(3)) and torch.equal(out["tf"][p], torch.zeros(3)), what


def check_fit(what, group, conf_b, src_b, tgt_b, idx, out, p, max_cond):
    """device R, t, cond of pair p against fit64 on the device's own index set; -> the Fit"""
    f, (eR, et, ec), (bR, bt, bc) = pr.fit_bars(conf_b, src_b, tgt_b, idx)
    dR = np.abs(out["R"][p].double().numpy() - f.R).max()
    dt = np.abs(out["t"][p].double().numpy() - f.t).max()
    rows = [("R", dR, eR, bR), ("t", dt, et, bt)]
    if f.cond < 1e4:
        rows.append(("cond", abs(float(out["cond"][p]) / f.cond - 1.0), ec, bc))
    for name, d, e, b in rows:
        print("%-44s %-5s device %.3e  e_ref %.3e  bar %.3e  cond %.3g" % (what, name, d, e, b, f.cond))
        if d / b > RATIOS.get(group, (-1.0,))[0]:
            RATIOS[group] = (d / b, what + " " + name, d, e, b)
    for name, d, e, b in rows:
        assert d <= b, (what, name, "device error %.3e over its bar %.3e (e_ref %.3e)" % (d, b, e))
    if abs(f.cond / max_cond - 1.0) > 1e-3 and np.isfinite(f.cond):
        assert bool(out["ok"][p]) == (f.cond < max_cond), (what, f.cond, max_cond)
    return f


# ---------------------------------------------------------------------------------------------------------------------------------------
# selection on every branch and form
# ---------------------------------------------------------------------------------------------------------------------------------------
GUARDED = {"128x128-distinct-1", "128x128-flat-1", "127x129-quantised-1", "256x257-quantised-1", "64x64-flat-20"}


def run_selection_case(case, misaligned=False):
    (N, M), kind, rate, want, want_flat = case
    name = pr.case_id(case) + ("-misaligned" if misaligned else "")
    conf, src, tgt = pr.selection_batch(case)
    P = conf.shape[0]
    K = pr.pair_k(N, M, rate)
    K_fixed = int((torch.maximum(torch.full((1,), float(N)), torch.full((1,), float(M))) * rate).int())      # the oracle's (max * rate).int()
    assert K == min(K_fixed, N * M, pr.PK_MAX)
    branches = [pr.reg_branch(conf[b], K) for b in range(P)] if want is not None else [None] * P
    assert branches == [want, want_flat, want], "the case does not reach the branch it was built for"
    if misaligned:
        buf = torch.empty(P * N * M + 4, device=DEV)
        assert buf.data_ptr() % 16 == 0
        conf_dev = buf[1:1 + P * N * M].view(P, N, M)
        conf_dev.copy_(conf)
        assert conf_dev.data_ptr() % 16 == 4 and conf_dev.is_contiguous()
    else:
        conf_dev = conf.to(DEV)
    max_cond = 200.0
    guard = pr.case_id(case) in GUARDED
    rc, form, out = call(conf_dev, src, tgt, rate, max_cond, guard=guard)
    assert rc == 0 and form == pr.launch_form(P, N, M), (rc, form)
    assert out["idx"].shape == (P, K_fixed)
    rc2, form2, again = call(conf_dev, src, tgt, rate, max_cond, guard=guard)
    assert (rc2, form2) == (rc, form)
    same_result(out, again, [K] * P)
    for b in range(P):
        what = "%s pair %d" % (name, b)
        check_selection(conf[b], out["idx"][b], K)
        check_invariants(what, out, b, max_cond)
        # (a flat tile is rank deficient by construction: its lowest indices share a row, and where K covers the tile Sxy = 0)
        if b != 1 and kind != "flat" and not pr.rank_deficient_by_construction(out["idx"][b, :K], conf[b], M):
            check_fit(what, "selection " + kind, conf[b], src[b], tgt[b], out["idx"][b, :K], out, b, max_cond)
    SEEN["form"].add(form)
    SEEN["branch"].update(b for b in branches if b)
    if guard:
        SEEN["guarded_form"].add(form)
    if form == 0:
        for c in pr.scalar_arm(P, N, M, conf_dev.data_ptr()):
            SEEN["scalar"].update(c)
        for b in range(P):
            if branches[b] == "list":
                SEEN["list"].add("more" if pr.reg_candidates(conf[b], K)[1] > K else "exact")
    if K < K_fixed:
        SEEN["k"].add("clipped")


@pytest.mark.parametrize("case", pr.SELECTION_CASES, ids=pr.case_id)
def test_selection(case):
    run_selection_case(case)


@pytest.mark.parametrize("kind", ["distinct", "flat"])
def test_selection_conf_one_float_past_a_16_byte_boundary(kind):
    case = [c for c in pr.SELECTION_CASES if pr.case_id(c) == "128x128-%s-1" % kind][0]
    run_selection_case(case, misaligned=True)


def test_thin_tiles_at_rate_20_are_refused():
    """K = 40960 > PK_MAX: DR_ENOSUP, nothing launched, nothing written"""
    conf = torch.rand(1, 2, 2048)
    rc, form, out = call(conf.to(DEV), torch.rand(1, 2, 3), torch.rand(1, 2048, 3), 20.0, 200.0, guard=True, prefill=float("nan"))
    assert rc == DR_ENOSUP and form == -1
    assert all(bool(torch.isnan(out[k]).all()) for k in ("R", "t", "Rf", "tf", "cond")) and bool((out["ok"] == -7).all()) and bool((out["idx"] == -7).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the long-slice take: P = 1, 2064 x 4096 -> slices of 33792 > 32768 entries, K = PK_MAX
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["distinct", "quantised"])
def test_long_slice_take(kind):
    N, M, rate = 2064, 4096, 1.0
    K = pr.pair_k(N, M, rate)
    assert K == pr.PK_MAX and pr.slice_len(1, N * M) == 33792 and pr.launch_form(1, N, M) == 2
    conf = pr.tile(kind, N, M, K, seed=5)[None]
    g = torch.Generator().manual_seed(6)
    src, tgt = torch.rand(1, N, 3, generator=g), torch.rand(1, M, 3, generator=g)
    conf_dev = conf.to(DEV)
    rc, form, out = call(conf_dev, src, tgt, rate, 200.0, guard=True)
    assert rc == 0 and form == 2
    rc, form, again = call(conf_dev, src, tgt, rate, 200.0, guard=True)
    same_result(out, again, [K])
    check_selection(conf[0], out["idx"][0], K)
    check_invariants("long slice " + kind, out, 0, 200.0)
    if kind == "distinct":
        check_fit("2064x4096-distinct-1", "long slice", conf[0], src[0], tgt[0], out["idx"][0, :K], out, 0, 200.0)
    SEEN["form"].add(form)
    SEEN["guarded_form"].add(form)


def test_long_slice_one_column_more_is_refused():
    N, M = 2064, 4097                                            # K = 4097 > PK_MAX
    conf_dev = torch.zeros(1, N, M, device=DEV)
    rc, form, out = call(conf_dev, torch.rand(1, N, 3), torch.rand(1, M, 3), 1.0, 200.0, guard=True, prefill=float("nan"))
    assert rc == DR_ENOSUP and form == -1
    assert all(bool(torch.isnan(out[k]).all()) for k in ("R", "t", "Rf", "tf", "cond")) and bool((out["ok"] == -7).all()) and bool((out["idx"] == -7).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# per-pair K (4D: use_mask_len)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", [(96, 80), (300, 400)])
def test_per_pair_k(N, M):
    """four pairs, four K: K_fixed, much smaller, 1 and 0 (both masks empty).  The reference is one B = 1 oracle call per pair: the header's
    per-pair meaning, not the batch-mean K of the reference's batched call."""
    P, rate, max_cond = 4, 1.0, 200.0
    lens = [(N, M), (17, 11), (1, 1), (0, 0)]
    sm = torch.stack([torch.arange(N) < a for a, _ in lens])
    tm = torch.stack([torch.arange(M) < b for _, b in lens])
    Ks = [pr.pair_k(N, M, rate, a, b) for a, b in lens]
    K_fixed = pr.pair_k(N, M, rate)
    assert Ks == [K_fixed, 17, 1, 0]
    conf = torch.stack([pr.tile("distinct", N, M, K_fixed, seed=N + b) for b in range(P)])
    g = torch.Generator().manual_seed(N)
    src, tgt = torch.rand(P, N, 3, generator=g), torch.rand(P, M, 3, generator=g)
    conf_dev = conf.to(DEV)
    rc, form, out = call(conf_dev, src, tgt, rate, max_cond, sm=sm, tm=tm, use_len=True, guard=True)
    assert rc == 0 and form == pr.launch_form(P, N, M)
    rc, form, again = call(conf_dev, src, tgt, rate, max_cond, sm=sm, tm=tm, use_len=True, guard=True)
    same_result(out, again, Ks)
    assert out["idx"].shape == (P, K_fixed)
    for b in range(P):
        what = "per-pair K %dx%d pair %d (K = %d)" % (N, M, b, Ks[b])
        check_selection(conf[b], out["idx"][b], Ks[b])
        check_invariants(what, out, b, max_cond)
        if Ks[b] >= 4:
            check_fit(what, "per-pair K", conf[b], src[b], tgt[b], out["idx"][b, :Ks[b]], out, b, max_cond)
            r = orc.procrustes(conf[b:b + 1], src[b:b + 1], tgt[b:b + 1], sm[b:b + 1], tm[b:b + 1], rate, max_cond, variant="4dmatch")
            _, _, (bR, bt, _) = pr.fit_bars(conf[b], src[b], tgt[b], out["idx"][b, :Ks[b]])
            assert np.abs(out["R"][b].numpy() - r[0][0].numpy()).max() <= 2 * bR          # both sides within bR of fit64
            assert np.abs(out["t"][b].numpy() - r[1][0, :, 0].numpy()).max() <= 2 * bt
    assert not bool(out["ok"][3])                                # K = 0: identity and zero forward, finite R (check_invariants)
    SEEN["form"].add(form)
    SEEN["guarded_form"].add(form)
    SEEN["k"].update(["per_pair", "zero"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fit's edges: constructed geometries
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", pr.GEOM_TILES)
def test_fit_edges(N, M):
    rate, max_cond = pr.GEOM_RATE, 200.0
    K = pr.pair_k(N, M, rate)
    cases = pr.geometry_cases(K, seed=N)
    built = {name: pr.matching_tile(N, M, X, Y, w, seed=N + len(name)) for name, (X, Y, w, _) in cases.items()}
    names = [n for n in cases if cases[n][3] != "near_coplanar"]
    conf = torch.stack([built[n][0] for n in names])
    src, tgt = torch.stack([built[n][1] for n in names]), torch.stack([built[n][2] for n in names])
    conf_dev = conf.to(DEV)
    rc, form, out = call(conf_dev, src, tgt, rate, max_cond)
    assert rc == 0 and form == 0
    rc, form, again = call(conf_dev, src, tgt, rate, max_cond)
    same_result(out, again, [K] * len(names))
    for p, n in enumerate(names):
        group, match = cases[n][3], built[n][3]
        what = "%dx%d %s" % (N, M, n)
        check_selection(conf[p], out["idx"][p], K)
        assert torch.equal(out["idx"][p].long().sort()[0], match), what + ": the selected set is not the matching"
        check_invariants(what, out, p, max_cond)
        if group == "deficient":
            assert not bool(out["ok"][p]), (what, float(out["cond"][p]))
            continue
        f = check_fit(what, group, conf[p], src[p], tgt[p], match, out, p, max_cond)
        assert bool(out["ok"][p]), (what, float(out["cond"][p]))
        if group == "reflection":
            assert f.det_uv < 0
        branch = pr.reg_branch(conf[p], K)
        if branch == "list":
            SEEN["list"].add("more" if pr.reg_candidates(conf[p], K)[1] > K else "exact")
    # near-coplanar: either side of the condition gate
    c1, s1, t1, match = built["near_coplanar"]
    f = pr.fit64(c1.numpy(), s1.numpy(), t1.numpy(), match.numpy())
    assert 1e3 < f.cond < 1e6
    for gate, want_ok in ((0.5 * f.cond, False), (2.0 * f.cond, True)):
        rc, form, out = call(c1[None].to(DEV), s1[None], t1[None], rate, gate)
        what = "%dx%d near_coplanar, gate %.3g" % (N, M, gate)
        assert torch.equal(out["idx"][0].long().sort()[0], match)
        check_invariants(what, out, 0, gate)
        check_fit(what, "near_coplanar", c1, s1, t1, match, out, 0, gate)
        assert bool(out["ok"][0]) == want_ok, (what, float(out["cond"][0]), f.cond)


def test_every_branch_and_form_was_seen():
    """the union of what the cases above reached (run the whole file)"""
    for group, (ratio, what, d, e, b) in sorted(RATIOS.items()):
        print("largest device error / bar  %-28s %.3f  (%s: device %.3e, e_ref %.3e, bar %.3e)" % (group, ratio, what, d, e, b))
    assert SEEN["form"] == {0, 1, 2}, SEEN
    assert SEEN["guarded_form"] == {0, 1, 2}, SEEN
    assert SEEN["branch"] == {"all", "k_gt_1024", "list", "bisect"}, SEEN
    assert SEEN["list"] == {"more", "exact"}, SEEN
    assert SEEN["scalar"] == {"nm", "ptr"}, SEEN
    assert SEEN["k"] == {"clipped", "zero", "per_pair"}, SEEN
