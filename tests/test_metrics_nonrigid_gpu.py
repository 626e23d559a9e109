"""The non-rigid evaluation on the GPU (dr_knn_points_f32, dr_nn_stats_f32, dr_flow_metrics_f32, diffreg_hip.metrics_nonrigid).

Fixture scenes (tests/golden/metrics_nonrigid.npz, minted by the reference's own functions): indices equal entry for entry, distances and
interpolated flows per element within max(one float32 ulp, 4 x the recorded float32 deviation of the reference), counts equal as integers,
EPE and Chamfer sums under the same bar scaled by n.  Edge cases: against tests/metrics_nonrigid_ref.py in the device's float32 rule, bit for
bit.  Every call is made twice and compared bit-equal."""
import os

import numpy as np
import pytest
import torch

from tests import metrics_nonrigid_ref as R
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
NAMES = [s[0] for s in R.SCENES]
DEV = "cuda:0"
f32 = np.float32


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "metrics_nonrigid.npz"))


@pytest.fixture(scope="module")
def M():
    from diffreg_hip import metrics_nonrigid
    return metrics_nonrigid


@pytest.fixture(scope="module")
def sizes(M):
    from diffreg_hip import lib
    return lib.raw().dr_knn_points_block(), lib.raw().dr_knn_points_tile()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scene(gold, name):
    return {k: gold["%s/in_%s" % (name, k)] for k in ("q", "s", "feats", "transform", "flow", "pred", "tgt_c", "s_moved", "test")}


def twice(fn, *a, **kw):
    r1, r2 = fn(*a, **kw), fn(*a, **kw)
    t1, t2 = (r1 if isinstance(r1, tuple) else (r1,)), (r2 if isinstance(r2, tuple) else (r2,))
    for x, y in zip(t1, t2):
        if x is not None:
            assert torch.equal(x, y) and torch.equal(torch.isnan(x), torch.isnan(y))
    return r1


def bar_of(want, dev32):
    """the project's bar for a float32 result held to a float64 reference, as tests/item3d_ref.py and tests/nonrigid_ref.py state it: max(one
    float32 ulp at the array's largest magnitude, 4 x the reference's own float32 deviation over the array); every element is held to it"""
    ulp = float(np.spacing(np.abs(want).astype(f32).max(initial=f32(0))))
    return max(ulp, 4.0 * float(dev32.max(initial=0.0)))


def within(got, gold, key, scale=1.0):
    want, d32 = np.atleast_1d(gold[key]), np.atleast_1d(gold[key + "_dev32"])
    got = np.atleast_1d(np.asarray(got, np.float64))
    real = np.isfinite(want) & (np.abs(want) < 1e9)          # +inf and the 1e10 padding of padding_mode="empty" are compared exactly
    assert got.shape == want.shape and np.array_equal(got[~real], want[~real]), key
    bar = bar_of(want[real], d32[real]) * scale
    worst = float((np.abs(got[real] - want[real] * scale) / bar).max(initial=0.0))
    print("%s: largest error / bar %.3f" % (key, worst))
    assert worst <= 1.0, (key, worst)
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_fixture_scene(M, gold, name):
    sc = scene(gold, name)
    q, s, T = dev(sc["q"]), dev(sc["s"]), dev(sc["transform"])
    Q, S = q.shape[0], s.shape[0]
    for tag, kw in R.KNN_CASES:
        dist, idx = twice(M.knn, q, s, return_distance=True, **kw)
        want = gold["%s/knn_%s_idx" % (name, tag)]
        assert tuple(idx.shape) == want.shape and np.array_equal(idx.cpu().numpy(), want), tag
        within(dist.cpu().numpy(), gold, "%s/knn_%s_dist" % (name, tag))
    feats = dev(sc["feats"])
    within(twice(M.knn_interpolate, q, s, feats, k=3).cpu().numpy(), gold, name + "/interp")
    within(twice(M.knn_interpolate, q, s, feats, k=3, distance_limit=R.INTERP_LIMIT).cpu().numpy(), gold, name + "/interp_limit")
    flow, pred, tgt_c, s_moved, test = dev(sc["flow"]), dev(sc["pred"]), dev(sc["tgt_c"]), dev(sc["s_moved"]), dev(sc["test"])

    def count(got, key, n):                   # a ratio of the reference (a float32 quotient) and the device's: the same integer over n
        assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
        assert round(float(got) * n) == round(float(gold[name + "/" + key]) * n) and abs(float(got) * n - round(float(got) * n)) < 1e-6, key
    count(twice(M.compute_nonrigid_inlier_ratio, q, tgt_c, flow, T, R.RADIUS), "nir", Q)
    count(twice(M.compute_nonrigid_inlier_ratio, q, tgt_c, flow, None, R.RADIUS), "nir_no_transform", Q)
    count(twice(M.compute_nonrigid_feature_matching_recall, s, s_moved, q, flow, test, T, R.RADIUS, R.NFMR_LIMIT), "nfmr", len(sc["test"]))
    count(twice(M.compute_scene_flow_accuracy, pred, flow, *R.STRICT), "acc_strict", Q)
    count(twice(M.compute_scene_flow_accuracy, pred, flow, *R.RELAXED), "acc_relaxed", Q)
    count(twice(M.compute_scene_flow_outlier_ratio, pred, flow, *R.OUTLIER), "outlier", Q)
    count(twice(M.compute_scene_flow_outlier_ratio, pred, flow, *R.OUTLIER_NONE), "outlier_none", Q)
    count(twice(M.compute_corr_coverage, q, s, R.COVERAGE_LIMIT), "coverage", Q)
    o, st = twice(M.flow_metrics, pred, flow, strict=R.STRICT, relaxed=R.RELAXED, outlier=R.OUTLIER)
    want = R.flow_metrics(sc["pred"], sc["flow"], strict=R.STRICT, relaxed=R.RELAXED, outlier=R.OUTLIER)
    got = o[0].cpu().numpy()
    assert np.array_equal(got[[0, 2, 3, 4, 5]], want[[0, 2, 3, 4, 5]]) and int(st[0]) == 0
    within(got[1], gold, name + "/epe", scale=Q)            # the sum under the bar scaled by n
    a, _ = twice(M.nn_stats, q, s)
    b, _ = twice(M.nn_stats, s, q)
    a, b = a[0].cpu().numpy(), b[0].cpu().numpy()
    assert a[0] == Q and b[0] == S
    within(a[1] * S + b[1] * Q, gold, name + "/chamfer", scale=Q * S)
    within(float(M.compute_chamfer_distance(q, s)), gold, name + "/chamfer")
    within(float(M.compute_chamfer_distance(q, s, squared=True)), gold, name + "/chamfer_squared")


def cloud(rng, n):
    return rng.uniform(-1, 1, (n, 3)).astype(f32)


def check_knn(M, q, s, k, ql=None, sl=None):
    """one ragged call against the float32 statement, bit for bit; -> (dist, idx, status) of the device"""
    dist, idx, st = twice(M.knn_points, dev(q), dev(s), k, ql, sl)
    ql, sl = ql or [len(q)], sl or [len(s)]
    q0 = s0 = 0
    for p, (nq, ns) in enumerate(zip(ql, sl)):
        wd, wi, wst = R.knn_points(q[q0:q0 + nq], s[s0:s0 + ns], k, f32)
        assert np.array_equal(idx[q0:q0 + nq].cpu().numpy(), wi), (p, nq, ns, k)
        assert np.array_equal(dist[q0:q0 + nq].cpu().numpy().view(np.uint32), wd.view(np.uint32)), (p, nq, ns, k)
        assert int(st[p]) == wst
        q0, s0 = q0 + nq, s0 + ns
    return dist, idx, st


def test_knn_query_and_support_edges(M, sizes):
    block, tile = sizes
    rng = np.random.default_rng(5)
    k = 5
    big = cloud(rng, 2 * tile + 1)
    for Q in (1, block - 1, block, block + 1):
        q = cloud(rng, Q)
        for S in (0, 1, k - 1, k, tile - 1, tile, tile + 1, 2 * tile + 1):
            check_knn(M, q, big[:S], k)


@pytest.mark.parametrize("k", [1, 3, 4, 5, 8, 9, 16])
def test_knn_template_widths_and_empty_middle_pair(M, sizes, k):
    block, tile = sizes
    rng = np.random.default_rng(100 + k)
    ql, sl = [block + 3, 0, 70], [tile + 9, 0, k + 1]
    check_knn(M, cloud(rng, sum(ql)), cloud(rng, sum(sl)), k, ql, sl)
    ql, sl = [5, 7, 3], [40, 0, 2]                           # queries without supports: +inf / -1
    check_knn(M, cloud(rng, sum(ql)), cloud(rng, sum(sl)), k, ql, sl)


def test_knn_ties_duplicates_self_and_nonfinite(M, sizes):
    block, tile = sizes
    rng = np.random.default_rng(9)
    s = cloud(rng, tile + 40)
    s[tile + 1:tile + 21] = s[100:120]                       # exact duplicates in another tile (and another wave's quarter): the lower index first
    q = np.concatenate([s[100:120], s[:30], cloud(rng, 20)])
    _, idx, _ = check_knn(M, q, s, 4)
    assert np.array_equal(idx[:20, 0].cpu().numpy(), np.arange(100, 120)) and np.array_equal(idx[:20, 1].cpu().numpy(), np.arange(tile + 1, tile + 21))
    dist, idx = M.knn(dev(q), dev(s), 3, return_distance=True, remove_nearest=True)       # a query that is a support: distance 0, then removed
    wd, wi, _ = R.knn_points(q, s, 4, f32)
    assert np.array_equal(idx.cpu().numpy(), wi[:, 1:]) and float(dist[20:50, 0].min()) > 0
    s2 = s.copy()
    s2[3], s2[tile + 5, 1] = np.nan, np.inf                  # never selected
    _, idx, st = check_knn(M, q, s2, 16)
    assert not np.isin(idx.cpu().numpy(), [3, tile + 5]).any() and int(st[0]) == 0
    q3 = np.concatenate([q, q])
    q3[7, 2] = np.nan                                        # a NaN query: row of -1, status 8 for its pair only
    dist, idx, st = check_knn(M, q3, np.concatenate([s, s[:50]]), 3, [len(q), len(q)], [len(s), 50])
    assert st.tolist() == [R.ST_NONFINITE, 0] and bool((idx[7] == -1).all()) and bool(torch.isinf(dist[7]).all())


def test_knn_merge_takes_the_last_quarter_of_the_last_tile(M, sizes):
    block, tile = sizes
    rng = np.random.default_rng(11)
    S = 2 * tile
    s = cloud(rng, S) + f32(10.0)
    s[S - 16:] = cloud(rng, 16) * f32(0.01)                  # the 16 nearest of every query near the origin lie at the very end
    q = cloud(rng, block + 1) * f32(0.01)
    q[1:] += f32(10.0)
    q[0] = 0
    _, idx, _ = check_knn(M, q, s, 16)
    assert sorted(idx[0].tolist()) == list(range(S - 16, S))


def test_knn_null_outputs_and_device_offsets(M):
    from diffreg_hip import lib
    rng = np.random.default_rng(13)
    q, s = cloud(rng, 70), cloud(rng, 90)
    full = M.knn_points(dev(q), dev(s), 3)
    d_only = M.knn_points(dev(q), dev(s), 3, return_indices=False)
    i_only = M.knn_points(dev(q), dev(s), 3, return_distance=False)
    assert d_only[1] is None and i_only[0] is None and torch.equal(d_only[0], full[0]) and torch.equal(i_only[1], full[1])
    # offsets that are wrong on the device only (no host mirror): status 4, the pair is skipped, the other pair is computed
    raw = lib.raw()
    qd, sd = dev(q), dev(s)
    qo, so = dev(np.array([0, 30, 70], np.int32)), dev(np.array([0, 40, 95], np.int32))
    dist = torch.full((70, 3), -7.0, device=DEV)
    idx = torch.full((70, 3), -7, dtype=torch.int64, device=DEV)
    st = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    lib.check(raw.dr_knn_points_f32(2, 70, lib.ptr(qd), lib.ptr(qo), 90, lib.ptr(sd), lib.ptr(so), None, None, 3, lib.ptr(dist), lib.ptr(idx),
                                    lib.ptr(st), lib.stream_of(qd)))
    assert st.tolist() == [0, R.ST_OFFSETS] and bool((idx[30:] == -7).all()) and bool((dist[30:] == -7).all())
    assert np.array_equal(idx[:30].cpu().numpy(), R.knn_points(q[:30], s[:40], 3, f32)[1])
    idx.fill_(-7)
    so = dev(np.array([0, 40, 90], np.int32))
    qo = dev(np.array([0, 75, 70], np.int32))
    lib.check(raw.dr_knn_points_f32(2, 70, lib.ptr(qd), lib.ptr(qo), 90, lib.ptr(sd), lib.ptr(so), None, None, 3, lib.ptr(dist), lib.ptr(idx),
                                    lib.ptr(st), lib.stream_of(qd)))
    assert st.tolist() == [R.ST_OFFSETS, R.ST_OFFSETS] and bool((idx == -7).all())


def test_knn_batched_leading_dimensions_and_pack_mode(M):
    rng = np.random.default_rng(17)
    q, s = cloud(rng, 2 * 3 * 20).reshape(2, 3, 20, 3), cloud(rng, 2 * 3 * 33).reshape(2, 3, 33, 3)
    dist, idx = M.knn(dev(q), dev(s), 4, return_distance=True)
    assert tuple(idx.shape) == (2, 3, 20, 4)
    for a in range(2):
        for b in range(3):
            wd, wi, _ = R.knn_points(q[a, b], s[a, b], 4, f32)
            assert np.array_equal(idx[a, b].cpu().numpy(), wi) and np.array_equal(dist[a, b].cpu().numpy(), wd)
    t = M.knn(dev(q[0, 0].T.copy()), dev(s[0, 0].T.copy()), 1, transposed=True, squeeze=True)
    assert tuple(t.shape) == (20,) and np.array_equal(t.cpu().numpy(), R.knn_points(q[0, 0], s[0, 0], 1, f32)[1][:, 0])
    flat_q, flat_s = q.reshape(-1, 3), s.reshape(-1, 3)
    pi = M.knn_pack_mode(dev(flat_q), dev(flat_s), [20] * 6, [33] * 6, 4)
    assert torch.equal(pi, idx.reshape(-1, 4))


def test_nn_stats_is_the_ordered_sum_of_the_k1_search(M, sizes):
    block, tile = sizes
    rng = np.random.default_rng(19)
    ql, sl = [3 * block + 7, 0, block, 9], [tile + 3, 5, 0, 40]
    q, s = cloud(rng, sum(ql)), cloud(rng, sum(sl))
    s[2] = np.nan
    limit = 0.3
    st, status = twice(M.nn_stats, dev(q), dev(s), limit, ql, sl)
    dist, idx, _ = M.knn_points(dev(q), dev(s), 1, ql, sl)
    dist, idx, q0 = dist.cpu().numpy()[:, 0], idx.cpu().numpy()[:, 0], 0
    for p, nq in enumerate(ql):
        want = R.ordered_nn_stats(dist[q0:q0 + nq], idx[q0:q0 + nq], limit, block) if nq else np.zeros(4)
        assert np.array_equal(st[p].cpu().numpy().view(np.uint64), want.view(np.uint64)), (p, st[p], want)
        q0 += nq
    assert st[:, 0].tolist() == [ql[0], 0, 0, 9] and status.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_flow_metrics_sizes(M, n):
    rng = np.random.default_rng(23 + n)
    tgt = (0.3 * cloud(rng, n)).astype(f32)
    pred = (tgt + rng.choice([0.01, 0.04, 0.09, 0.3], (n, 1)).astype(f32) * cloud(rng, n)).astype(f32)
    if n > 1:
        tgt[0] = 0                                           # a point exactly at target = 0: rel through eps
        pred[0] = (0, 0, 1e-3) if n > 63 else (0, 0, 0)
    mask = rng.uniform(size=n) < 0.7
    ang = 0.4
    T = np.eye(4, dtype=f32)
    T[:3, :3] = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], f32)
    T[:3, 3] = (0.01, -0.02, 0.03)
    cases = (dict(strict=(0.05, 0.05), relaxed=(0.1, 0.1), outlier=(0.3, 0.1)), dict(strict=(0.05, 0.05), relaxed=(0.1, 0.1), outlier=(None, 0.1)),
             dict(strict=(0.05, 0.05), relaxed=(0.1, 0.1), outlier=(0.3, None)), dict(outlier=(None, None)))
    for kw in cases:
        for m, tr in ((None, None), (mask, None), (np.zeros(n, bool), None), (None, T)):
            rot = trn = None
            if tr is not None:
                rot, trn = dev(tr[None, :3, :3]), dev(tr[None, :3, 3])
            got, st = twice(M.flow_metrics, dev(pred), dev(tgt), mask=None if m is None else dev(m), rot=rot, trn=trn, **kw)
            want = R.flow_metrics(pred, tgt, mask=m, transform=tr, dtype=f32, **kw)
            g = got[0].cpu().numpy()
            if tr is None:                                   # float32 in the statement's own order: the same integers
                assert np.array_equal(g[[0, 2, 3, 4, 5]], want[[0, 2, 3, 4, 5]]), (n, kw, g, want)
            else:                                            # the rotation's float32 order is the device's own: counts within the points near a threshold
                e, rel = R.flow_terms(R.apply_transform(pred, tr), tgt)
                near = sum(int((np.abs(x - t) < 1e-6).sum()) for x, t in ((e, 0.05), (e, 0.1), (e, 0.3), (rel, 0.05), (rel, 0.1)))
                assert np.all(np.abs(g[[0, 2, 3, 4, 5]] - R.flow_metrics(pred, tgt, transform=tr, **kw)[[0, 2, 3, 4, 5]]) <= near)
            assert abs(g[1] - want[1]) <= max(n, 1) * 2e-7 * 2 and int(st[0]) == 0
            if m is not None and not m.any():
                assert not g.any()


def test_evaluate_pairs_equals_the_functions_pair_by_pair(M, gold):
    from diffreg_hip import shard
    scs = [scene(gold, "d"), scene(gold, "g")]
    src = [dev(sc["q"]) for sc in scs]
    flows = [dev(sc["flow"]) for sc in scs]
    tgt = [dev(sc["s"]) for sc in scs]
    Ts = [dev(sc["transform"]) for sc in scs]
    warped = [dev((R.apply_transform(sc["q"] + sc["pred"], sc["transform"], f32)).astype(f32)) for sc in scs]
    rng = np.random.default_rng(3)
    matches = [dev(np.stack([rng.integers(0, len(sc["q"]), 50), rng.integers(0, len(sc["s"]), 50)], 1).astype(np.int64)) for sc in scs]
    test = [dev(sc["test"]) for sc in scs]
    kw = dict(strict=R.STRICT, relaxed=R.RELAXED, outlier=R.OUTLIER, acceptance_radius=R.RADIUS, distance_limit=R.NFMR_LIMIT,
              coverage_limit=R.COVERAGE_LIMIT)
    ev = M.evaluate_nonrigid_pairs(src, warped, flows, tgt, Ts, matches, test, **kw)
    ev2 = M.evaluate_nonrigid_pairs(src, warped, flows, tgt, Ts, matches, test, **kw)
    assert torch.equal(ev["vector"], ev2["vector"]) and ev["vector"].dtype == torch.float64 and ev["vector"].is_cuda
    from diffreg_hip.metrics_nonrigid import _rt
    for p in range(2):
        rot, trn = _rt(Ts[p])
        target = torch.bmm(rot.expand(len(src[p]), 3, 3), (src[p] + flows[p])[:, :, None])[:, :, 0] + trn - src[p]
        pf = warped[p] - src[p]
        o, _ = M.flow_metrics(pf, target, strict=R.STRICT, relaxed=R.RELAXED, outlier=R.OUTLIER)
        sc, tc = src[p][matches[p][:, 0]], tgt[p][matches[p][:, 1]]
        want = {"EPE": o[0, 1] / o[0, 0], "AccS": M.compute_scene_flow_accuracy(pf, target, *R.STRICT),
                "AccR": M.compute_scene_flow_accuracy(pf, target, *R.RELAXED), "outlier": M.compute_scene_flow_outlier_ratio(pf, target, *R.OUTLIER),
                "NIR": M.compute_nonrigid_inlier_ratio(sc, tc, flows[p][matches[p][:, 0]], Ts[p], R.RADIUS),
                "NFMR": M.compute_nonrigid_feature_matching_recall(sc, tc, src[p], flows[p], test[p], Ts[p], R.RADIUS, R.NFMR_LIMIT),
                "chamfer": M.compute_chamfer_distance(warped[p], tgt[p]), "coverage": M.compute_corr_coverage(src[p], sc, R.COVERAGE_LIMIT)}
        for key, w in want.items():
            assert float(ev[key][p]) == float(w), (p, key, float(ev[key][p]), float(w))
    vec = ev["vector"].cpu().numpy()
    names = M.VECTOR_NAMES
    for key, slot in (("NIR", "sum_inlier_ratio"), ("NFMR", "sum_fmr"), ("EPE", "sum_EPE"), ("AccS", "sum_AccS"), ("AccR", "sum_AccR"),
                      ("outlier", "sum_outlier"), ("chamfer", "sum_chamfer"), ("coverage", "sum_coverage")):
        assert vec[names.index(slot)] == float(ev[key].sum()), key
    assert vec[names.index("n_pairs")] == 2 and vec[2] == 0 and vec[4] == 0
    red = shard.reduce_metrics(ev["vector"][:5])
    assert red["mean_inlier_ratio"] == pytest.approx(float(ev["NIR"].mean())) and red["fmr"] == pytest.approx(float(ev["NFMR"].mean()))
    full = M.reduce_pair_metrics(ev["vector"])
    assert full["EPE"] == pytest.approx(float(ev["EPE"].mean())) and full["chamfer"] == pytest.approx(float(ev["chamfer"].mean()))


def test_registration_evaluate_forwards(M):
    from diffreg_hip.nonrigid import NonRigidRegistration
    rng = np.random.default_rng(29)
    src = dev(cloud(rng, 300))
    flow = dev((0.05 * cloud(rng, 300)).astype(f32))
    tgt = src + flow
    matches = dev(np.stack([np.arange(0, 300, 3), np.arange(0, 300, 3)], 1).astype(np.int64))
    reg = NonRigidRegistration(node_coverage=0.5, num_iterations=20)
    result = reg(src, tgt, matches)
    kw = dict(strict=R.STRICT, relaxed=R.RELAXED, outlier=R.OUTLIER)
    ev = reg.evaluate(result, src, flow, tgt, matches=matches, **kw)
    want = M.evaluate_nonrigid_pairs([src], [result[0]], [flow], [tgt], None, [matches], None, **kw)
    assert torch.equal(ev["vector"], want["vector"]) and float(ev["NIR"][0]) == 1.0


def test_graph_capture_replays_equal(M):
    rng = np.random.default_rng(31)
    q, s = dev(cloud(rng, 200)), dev(cloud(rng, 1100))
    want = M.knn_points(q, s, 8)
    want_st = M.nn_stats(q, s, 0.2)
    from diffreg_hip import lib
    raw = lib.raw()
    qo, so = dev(np.array([0, 200], np.int32)), dev(np.array([0, 1100], np.int32))
    dist, idx = torch.zeros(200, 8, device=DEV), torch.zeros(200, 8, dtype=torch.int64, device=DEV)
    status, stats = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, 4, dtype=torch.float64, device=DEV)
    wsb = raw.dr_nn_stats_workspace_bytes(1, 200)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            lib.check(raw.dr_knn_points_f32(1, 200, lib.ptr(q), lib.ptr(qo), 1100, lib.ptr(s), lib.ptr(so), None, None, 8, lib.ptr(dist),
                                            lib.ptr(idx), lib.ptr(status), lib.stream_of(q)))
            lib.check(raw.dr_nn_stats_f32(1, 200, lib.ptr(q), lib.ptr(qo), 1100, lib.ptr(s), lib.ptr(so), None, None, 0.2, lib.ptr(stats),
                                          lib.ptr(status), lib.ptr(ws), wsb, lib.stream_of(q)))
    for _ in range(2):
        dist.zero_(), idx.zero_(), stats.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(dist, want[0]) and torch.equal(idx, want[1]) and torch.equal(stats, want_st[0])
