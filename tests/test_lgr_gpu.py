"""GPU checks of the RANSAC-free rigid estimators (csrc/lgr.hip): parity with the reference's stored outputs on every fixture scene at the
project's bar -- max(one float32 ulp at the tensor's scale, 4 x the reference's own float32 deviation from float64) -- with indices, counts,
masks and iteration counts equal; the edges against the float64 statement of tests/lgr_ref.py; determinism; capture."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import lgr_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
ALL = R.SCENES + [R.E2E]
NAMES = [s[0] for s in ALL]
ULP = lambda scale: float(np.spacing(np.float32(max(float(scale), 1e-30))))


@pytest.fixture(scope="module")
def G():
    from diffreg_hip import registration
    return registration


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "lgr.npz"))


def scene(gold, name):
    spec = next(s for s in ALL if s[0] == name)
    sc = {k: gold["%s/in_%s" % (name, k)] for k in ("src_knn_points", "tgt_knn_points", "src_masks", "tgt_masks", "score_mat", "global_scores",
                                                    "R", "t")}
    sc.update(name=name, opts=dict(R.OPTS, **spec[3]))
    return sc


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def held(got, want, dev, what):
    """every element within max(1 float32 ulp at the tensor's scale, 4 x dev); -> error / bar"""
    got, want = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.size == 0:
        return 0.0
    bar = max(ULP(np.abs(want).max()), 4.0 * float(dev))
    err = float(np.abs(got - want).max())
    print("%s: error %.3e bar %.3e ratio %.3f" % (what, err, bar, err / bar))
    assert err <= bar, (what, err, bar)
    return err / bar


def module(G, o):
    return G.LocalGlobalRegistration(o["k"], o["radius"], o["mutual"], o["threshold"], o["use_dustbin"], o["use_global_score"], o["use_logits"],
                                     o["min_local"], o["max_global"], o["steps"])


def run_forward(G, sc, **kw):
    return module(G, sc["opts"])(cu(sc["src_knn_points"]), cu(sc["tgt_knn_points"]), cu(sc["src_masks"]), cu(sc["tgt_masks"]), cu(sc["score_mat"]),
                                 cu(sc["global_scores"]), **kw)


@pytest.mark.parametrize("name", NAMES)
def test_fixture_parity(G, gold, name):
    sc = scene(gold, name)
    g = lambda k: gold["%s/%s" % (name, k)]
    d = lambda k: gold["%s/dev_%s" % (name, k)]
    vs, vt, vw, T = run_forward(G, sc)
    assert np.array_equal(vs.cpu().numpy().astype(np.float64), g("src_corr")) and np.array_equal(vt.cpu().numpy().astype(np.float64), g("tgt_corr"))
    held(vw, g("corr_scores"), d("corr_scores"), "corr_scores")
    held(T, g("transform"), d("transform"), "transform")
    ps, pt, pw, pT, cnt = run_forward(G, sc, padded=True)
    n = int(cnt)
    assert n == vw.shape[0] and torch.equal(ps[:n], vs) and torch.equal(pw[:n], vw) and torch.equal(pT, T)
    held(G.weighted_procrustes(vs, vt, vw), g("procrustes"), d("procrustes"), "procrustes")
    held(G.WeightedProcrustes()(vs[None], vt[None])[0], g("procrustes_unweighted"), d("procrustes_unweighted"), "procrustes_unweighted")
    if n <= R.DENSE_MAX:
        held(G.spatial_consistency(vs, vt, R.SIGMA), g("sc"), d("sc"), "sc")
        h = max(n // 2, 1)
        held(G.cross_spatial_consistency(vs[:h], vt[:h], vs, vt, R.SIGMA), g("cross_sc"), d("cross_sc"), "cross_sc")
    held(G.spatial_consistency_counts(vs, vt, R.SIGMA), g("sc_counts"), d("sc_counts"), "sc_counts")
    assert np.array_equal(G.SpatialConsistencyFiltering(min(R.SCF_K, n), R.SIGMA)(vs, vt).cpu().numpy(), g("scf_topk"))
    vec, its = G.leading_eigenvector(vs, tgt_points=vt, sigma=R.SIGMA, num_iterations=R.EIG_ITERS, return_iterations=True)
    assert int(its) == int(g("eig_iterations"))
    held(vec, g("eig"), d("eig"), "eig")
    # the hypotheses and the masks against the statement (the screens keep every residual 1e-5 from the radius)
    b, i, j, rs, rt, rw, r = R.forward(sc)
    o = sc["opts"]
    src, tgt = cu(sc["src_knn_points"][b, i]), cu(sc["tgt_knn_points"][b, j])
    verify = None if len(rw) == len(b) else (vs, vt, vw, cu(np.array([0, len(rw)], np.int32)))
    out = G.local_to_global_registration_pairs(src, tgt, cu(r_scores(sc, b, i, j)), cu(b.astype(np.int32)), cu(np.array([0, len(b)], np.int32)),
                                               o["radius"], o["min_local"], o["steps"], verify, hypotheses=True)
    nch = len(r["chunks"])
    assert out["chunk_offsets"].tolist() == [0, nch] and int(out["best_chunk"][0]) == r["best_chunk"] and int(out["status"][0]) == 0
    assert np.array_equal(out["chunk_counts"][:nch].cpu().numpy(), r["chunk_counts"])
    assert np.array_equal(out["final_scores"].cpu().numpy() != 0, r["final_scores"] != 0)
    for c in range(nch):
        held(out["chunk_transforms"][c], r["chunk_transforms"][c], d("transform"), "chunk %d" % c)
    if name == "end_to_end":
        rot, trn = R.pose_errors(T.cpu().numpy().astype(np.float64), sc["R"], sc["t"])
        want = gold[name + "/pose_error"]
        print("pose error %.6f deg %.6f against the reference's %.6f deg %.6f" % (rot, trn, want[0], want[1]))
        assert rot <= want[0] + np.degrees(ULP(1.0)) and trn <= want[1] + ULP(1.0)


def r_scores(sc, b, i, j):
    o = sc["opts"]
    return R.extract(sc["score_mat"], o["k"], sc["src_masks"], sc["tgt_masks"], sc["global_scores"], o["threshold"], o["mutual"], o["use_dustbin"],
                     o["use_global_score"], o["use_logits"])[3]


def test_batch_of_all_scenes_equals_the_single_calls(G, gold):
    parts, singles = [], []
    for name in NAMES:
        sc = scene(gold, name)
        b, i, j, _, _, _, r = R.forward(sc)
        o = sc["opts"]
        if o["max_global"] is not None or o["steps"] != 5 or o["min_local"] != 3:
            continue
        parts.append((sc["src_knn_points"][b, i], sc["tgt_knn_points"][b, j], r_scores(sc, b, i, j), b.astype(np.int32)))
        singles.append(r)
    off = np.cumsum([0] + [len(p[0]) for p in parts]).astype(np.int32)
    cat = lambda k: cu(np.concatenate([p[k] for p in parts]))
    out = G.local_to_global_registration_pairs(cat(0), cat(1), cat(2), cat(3), cu(off), 0.1, 3, 5, hypotheses=True, host_offsets=off)
    again = G.local_to_global_registration_pairs(cat(0), cat(1), cat(2), cat(3), cu(off), 0.1, 3, 5, hypotheses=True)
    for k in out:
        assert torch.equal(out[k], again[k]), k
    assert out["status"].tolist() == [0] * len(parts)
    assert out["chunk_offsets"].tolist() == list(np.cumsum([0] + [len(r["chunks"]) for r in singles]))
    for p, r in enumerate(singles):
        assert int(out["best_chunk"][p]) == r["best_chunk"]
        held(out["transform"][p], r["transform"], 0.0, "batched transform %d" % p)
        assert np.array_equal(out["final_scores"][off[p]:off[p + 1]].cpu().numpy() != 0, r["final_scores"] != 0)


def groups(lengths, seed=3):
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    Rm, t = R.rigid(rng)
    src = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    tgt = (src @ Rm.T + t + rng.normal(scale=0.01, size=(n, 3))).astype(np.float32)
    w = rng.uniform(0.1, 1.0, size=n).astype(np.float32)
    return src, tgt, w, np.cumsum([0] + list(lengths)).astype(np.int32)


def test_procrustes_edges_and_paths(G):
    limit = G._raw.dr_lgr_wave_limit()
    lengths = [1, 2, 3, 63, 64, 65, limit, limit + 1, 3 * limit + 7]
    src, tgt, w, off = groups(lengths)
    T, st = G.weighted_procrustes_groups(cu(src), cu(tgt), cu(off), cu(w), host_offsets=off)
    Tw, _ = G.weighted_procrustes_groups(cu(src), cu(tgt), cu(off), cu(w), wave_limit=2 ** 31 - 1)
    Tg, _ = G.weighted_procrustes_groups(cu(src), cu(tgt), cu(off), cu(w), wave_limit=0)
    assert torch.equal(T, Tw) and torch.equal(T, Tg)            # the wave path and the workgroup path on the same groups: the same bits
    assert st.tolist() == [0] * len(lengths)
    for g in range(len(lengths)):
        sl = slice(off[g], off[g + 1])
        want = R.weighted_procrustes(src[sl], tgt[sl], w[sl])
        if lengths[g] >= 3:
            held(T[g], want, 0.0, "group of %d" % lengths[g])
            continue
        # one or two rows: H has rank 1 (eps keeps it from zero), so the turn about the fitted direction is whatever the SVD completes its
        # basis with -- LAPACK's in the statement, the Jacobi's on the device.  What the data determine is held: a proper rotation, and
        # where the rows land.  A landed coordinate adds three products of a rotation entry (rounded to float32: half an ulp of 1) with a
        # coordinate and the rounded translation: 4 ulp at the scale of the landed points
        got = T[g].cpu().numpy().astype(np.float64)
        assert float(np.abs(got[:3, :3] @ got[:3, :3].T - np.eye(3)).max()) <= 4 * ULP(1.0) and np.linalg.det(got[:3, :3]) > 0.999999
        land = lambda M: src[sl].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
        a, b = land(got), land(want.astype(np.float32).astype(np.float64))
        assert float(np.abs(a - b).max()) <= 4 * ULP(np.abs(b).max()), (lengths[g], np.abs(a - b).max())
    one, st1 = G.weighted_procrustes_groups(cu(src[:65]), cu(tgt[:65]), cu(np.array([0, 65], np.int32)))
    held(one[0], R.weighted_procrustes(src[:65], tgt[:65]), 0.0, "G = 1, unweighted")
    # all weights zero: identity, bit 16; a NaN coordinate: bit 8, the other groups untouched; bad offsets: bit 4
    w0 = w.copy()
    w0[off[3]:off[4]] = 0.0
    src_bad = src.copy()
    src_bad[off[5]] = np.nan
    off_bad = off.copy()
    off_bad[2] = -5                                              # groups 1 and 2 lose their slices
    out = torch.full((len(lengths), 16), 7.0, device="cuda")
    stat = torch.full((len(lengths),), -1, dtype=torch.int32, device="cuda")
    from diffreg_hip.lib import check, ptr, stream_of
    s, t_, ww, oo = cu(src_bad), cu(tgt), cu(w0), cu(off_bad)
    check(G._raw.dr_weighted_procrustes_f32(len(lengths), len(src), ptr(s), ptr(t_), ptr(ww), ptr(oo), None, 0.0, 1e-5, -1, ptr(out), ptr(stat),
                                            stream_of(s)))
    assert stat.tolist() == [0, 4, 4, 16, 0, 8, 0, 0, 0]
    assert torch.equal(out[3].view(4, 4), torch.eye(4, device="cuda"))
    assert bool((out[[1, 2, 5]] == 7.0).all())                  # skipped groups are not written
    assert torch.equal(out[[4, 6, 7, 8]], T.reshape(-1, 16)[[4, 6, 7, 8]])
    # a host mirror that disagrees with what a mirror must be: refused, nothing launched
    mirror = np.array([0, 9, 4], np.int32)
    rc = G._raw.dr_weighted_procrustes_f32(2, 10, ptr(s), ptr(t_), None, ptr(oo), mirror.ctypes.data_as(ctypes.c_void_p), 0.0, 1e-5, -1, ptr(out),
                                           ptr(stat), stream_of(s))
    assert rc == -1 and bool((out[1] == 7.0).all())


def test_lgr_edges(G):
    src, tgt, w, ids = R.tie_scene()
    # problems: 0 = the tie, 1 = empty, 2 = a NaN coordinate, 3 = the tie again
    S = np.concatenate([src, src, src])
    T_ = np.concatenate([tgt, tgt, tgt])
    W = np.concatenate([w, w, w])
    I = np.concatenate([ids, ids, ids])
    S[8 + 2, 1] = np.nan
    off = np.array([0, 8, 8, 16, 24], np.int32)
    out = G.local_to_global_registration_pairs(cu(S), cu(T_), cu(W), cu(I), cu(off), 0.1, 3, 2, hypotheses=True)
    want = R.lgr(src, tgt, w, ids, 0.1, 3, 2)
    assert out["status"].tolist() == [0, 32, 8, 0] and out["best_chunk"].tolist()[:2] == [0, -1] and int(out["best_chunk"][3]) == 0
    assert out["chunk_offsets"].tolist() == [0, 2, 2, 2, 4] and out["chunk_counts"][:4].tolist() == [4, 4, 4, 4]
    assert torch.equal(out["transform"][1], torch.eye(4, device="cuda")) and torch.equal(out["transform"][0], out["transform"][3])
    held(out["transform"][0], want["transform"], 0.0, "tie transform")
    # an Inf score in one problem, descending patch ids in another: bits 8 and 4, skipped, canaries intact
    W2, I2 = W.copy(), I.copy()
    W2[1] = np.inf
    I2[16:24] = I2[16:24][::-1]
    off3 = np.array([0, 8, 16, 24], np.int32)
    from diffreg_hip.lib import check, ptr, stream_of
    raw = G._raw
    n = 24
    a, b_, c, d = cu(S), cu(T_), cu(W2), cu(I2)
    a[10, 1] = float(src[2, 1])                                  # the NaN of the first call is gone: problem 1 is the tie again
    o = cu(off3)
    tr = torch.full((5, 16), 7.0, device="cuda")
    best = torch.full((5,), 7, dtype=torch.int32, device="cuda")
    fin = torch.full((n + 2,), 7.0, device="cuda")
    st = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    wsb = raw.dr_lgr_workspace_bytes(3, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    call = lambda wsb_, hc=None: raw.dr_lgr_f32(3, n, ptr(a), ptr(b_), ptr(c), ptr(d), ptr(o), n, ptr(a), ptr(b_), ptr(c), ptr(o), hc, None, 0.1, 3,
                                                2, 0.0, 1e-5, ptr(tr[1:4]), ptr(best[1:4]), ptr(fin[1:n + 1]), None, None, None, ptr(st), ptr(ws),
                                                wsb_, stream_of(a))
    assert call(wsb - 1) == -4                                   # a short workspace: DR_EWORKSPACE, nothing launched
    assert call(wsb, np.array([0, 9, 8, 24], np.int32).ctypes.data_as(ctypes.c_void_p)) == -1
    torch.cuda.synchronize()
    assert st.tolist() == [-1, -1, -1] and bool((tr == 7.0).all())
    check(call(wsb))
    assert st.tolist() == [8, 0, 4]
    assert bool((tr[[0, 1, 3, 4]] == 7.0).all()) and bool((fin[:9] == 7.0).all()) and bool((fin[17:] == 7.0).all())
    assert best.tolist() == [7, 7, 0, 7, 7]
    assert torch.equal(tr[2].view(4, 4), out["transform"][0])


def pairs(n, seed, dup=0):
    rng = np.random.default_rng(seed)
    Rm, t = R.rigid(rng)
    src = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    tgt = (src @ Rm.T + t + rng.normal(scale=0.03, size=(n, 3))).astype(np.float32)
    if dup:
        src[n - dup:], tgt[n - dup:] = src[:dup], tgt[:dup]      # duplicated correspondences: delta = 0, sc = 1
    return src, tgt


def test_row_sums_on_both_sides_of_block_and_tile(G):
    blk, tile = G._raw.dr_sc_block(), G._raw.dr_sc_tile()
    sigma = 0.3
    big = pairs(2 * tile + 3, 11, dup=4)
    full = R.spatial_consistency(big[0], big[1], sigma=sigma)    # computed once, sliced below
    assert np.all(np.diag(full)[:4] == 1.0) and np.all(full[np.arange(4), len(full) - 4 + np.arange(4)] == 1.0)
    per = R.sc_bar(sigma, big[0], big[1])
    for nq in (1, blk - 1, blk, blk + 1):
        for ns in (1, tile - 1, tile, tile + 1, 2 * tile + 3):
            got = G.spatial_consistency_counts(cu(big[0][:nq]), cu(big[1][:nq]), sigma, cu(big[0][-ns:]), cu(big[1][-ns:]))
            want = full[:nq, len(full) - ns:].sum(1)
            # every float32 consistency value lies within lgr_ref.sc_bar of the float64 one; ns of them add up, then one rounding of the sum
            bar = ns * per + ULP(np.abs(want).max())
            assert float(np.abs(got.cpu().numpy() - want).max()) <= bar, (nq, ns)
    a = G.spatial_consistency_counts(cu(big[0]), cu(big[1]), sigma)
    assert torch.equal(a, G.spatial_consistency_counts(cu(big[0]), cu(big[1]), sigma))
    dense = G.spatial_consistency(cu(big[0][:blk + 1]), cu(big[1][:blk + 1]), sigma)
    assert torch.equal(dense, G.spatial_consistency(cu(big[0][:blk + 1]), cu(big[1][:blk + 1]), sigma))
    assert float(np.abs(dense.cpu().numpy() - full[:blk + 1, :blk + 1]).max()) <= per
    batched = G.spatial_consistency_counts(cu(np.stack([big[0][:70], big[0][70:140]])), cu(np.stack([big[1][:70], big[1][70:140]])), sigma)
    assert torch.equal(batched[1], G.spatial_consistency_counts(cu(big[0][70:140]), cu(big[1][70:140]), sigma))


def test_eigenvector_edges(G):
    src, tgt = pairs(130, 5)
    vec, its = G.leading_eigenvector(cu(src), tgt_points=cu(tgt), sigma=1e-6, return_iterations=True)
    # every off-diagonal entry is 0: the vector stays the normalised ones vector and the stop holds at the reference's loop index 1, the
    # second iteration (the first moves the ones vector to its normalised form, which allclose tells apart)
    assert int(its) == 2 and R.leading_eigenvector(np.eye(130))[1] == 2
    held(vec, np.full(130, 1.0 / np.sqrt(130.0)), 0.0, "ones")
    # the dense form against eigh in float64, up to sign, on a matrix with a spectral gap of 2 x
    rng = np.random.default_rng(8)
    Q, _ = np.linalg.qr(rng.normal(size=(67, 67)))
    lam = np.concatenate([[4.0], rng.uniform(0.1, 2.0, size=66)])
    M = ((Q * lam) @ Q.T).astype(np.float32)
    truth = np.linalg.eigh(M.astype(np.float64))[1][:, -1]
    v32 = torch.ones(67)
    for _ in range(40):
        v32 = torch.nn.functional.normalize(torch.from_numpy(M) @ v32, dim=0)
    fix = lambda v: v * np.sign(v @ truth)
    dev = float(np.abs(fix(v32.numpy().astype(np.float64)) - truth).max())
    got, its = G.leading_eigenvector(cu(M), num_iterations=40, return_iterations=True)
    again = G.leading_eigenvector(cu(M), num_iterations=40)
    assert torch.equal(got, again) and 1 < int(its) <= 40
    held(fix(got.cpu().numpy().astype(np.float64)), truth, dev, "dense eigenvector")
    two, its2 = G.leading_eigenvector(cu(np.stack([M, np.eye(67, dtype=np.float32)])), num_iterations=40, return_iterations=True)
    assert torch.equal(two[0], got) and its2.tolist() == [int(its), 2]


def test_capture_replays_the_eager_result(G, gold):
    sc = scene(gold, "base")
    b, i, j, _, _, _, r = R.forward(sc)
    args = (cu(sc["src_knn_points"][b, i]), cu(sc["tgt_knn_points"][b, j]), cu(r_scores(sc, b, i, j)), cu(b.astype(np.int32)),
            cu(np.array([0, len(b)], np.int32)), 0.1, 3, 5)
    eager = G.local_to_global_registration_pairs(*args)
    eig = G.leading_eigenvector(args[0], tgt_points=args[1], sigma=R.SIGMA)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            cap = G.local_to_global_registration_pairs(*args)
            cap_eig = G.leading_eigenvector(args[0], tgt_points=args[1], sigma=R.SIGMA)
    cap["transform"].zero_()
    cap_eig.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap["transform"], eager["transform"]) and torch.equal(cap["final_scores"], eager["final_scores"])
    assert torch.equal(cap_eig, eig)
