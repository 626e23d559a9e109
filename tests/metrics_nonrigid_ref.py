"""The statement of the non-rigid evaluation (dr_knn_points_f32, dr_nn_stats_f32, dr_flow_metrics_f32 and diffreg_hip.metrics_nonrigid) in numpy,
for the GPU edge tests to call; tests/test_metrics_nonrigid_cpu.py holds it to what the reference's own functions produced
(tests/golden/metrics_nonrigid.npz, tools/golden/make_golden_metrics_nonrigid.py).

dtype=np.float64 is the float64 statement the fixture is compared with.  dtype=np.float32 is the DEVICE's rule operation by operation --
d2 = (dx dx + dy dy) + dz dz in float32 (numpy never fuses), slots ascending by (d2, support index), dist = sqrt(d2) -- so that an edge test
compares indices and distances bit for bit."""
import numpy as np

ST_OFFSETS, ST_NONFINITE = 4, 8
SCENES = (  # name, Q, S, duplicated supports
    ("a", 40, 12, 0), ("b", 63, 64, 0), ("c", 64, 65, 0), ("d", 65, 100, 6), ("e", 33, 90, 0), ("f", 70, 257, 0), ("g", 129, 200, 8),
    ("h", 30, 320, 0), ("i", 100, 400, 0), ("j", 20, 33, 0))
KNN_CASES = (  # tag, keyword arguments of the reference's knn
    ("k1", dict(k=1)), ("k3", dict(k=3)), ("k8", dict(k=8)), ("k16", dict(k=16)), ("k3rm", dict(k=3, remove_nearest=True)),
    ("k4d2", dict(k=4, dilation=2)), ("k8near", dict(k=8, distance_limit=0.45, padding_mode="nearest")),
    ("k8empty", dict(k=8, distance_limit=0.45, padding_mode="empty")))
INTERP_LIMIT = 0.35
STRICT, RELAXED, OUTLIER, OUTLIER_NONE = (0.05, 0.05), (0.1, 0.1), (0.3, 0.1), (None, 0.1)
RADIUS, NFMR_LIMIT, COVERAGE_LIMIT = 0.08, 0.4, 0.2
SCREEN_GAP = 1e-5
SCREEN_RANK = 18                     # gaps through position k + 1 of the deepest search of the fixture (k = 16, and 17 with remove_nearest)


def d2_matrix(q, s, dtype):
    q, s = np.asarray(q, dtype), np.asarray(s, dtype)
    dx, dy, dz = (q[:, None, c] - s[None, :, c] for c in range(3))
    return (dx * dx + dy * dy) + dz * dz


def knn_points(q, s, k, dtype=np.float64):
    """-> (dist [Q, k], idx [Q, k] int64, status): +inf / -1 where a slot has no support; a non-finite support (or d2) is never selected; a
    non-finite query has an all -1 row and sets status 8"""
    q, s = np.asarray(q, dtype).reshape(-1, 3), np.asarray(s, dtype).reshape(-1, 3)
    Q, S = q.shape[0], s.shape[0]
    with np.errstate(all="ignore"):
        d2 = d2_matrix(q, s, dtype)
        d2 = np.where(np.isfinite(d2), d2, np.inf)
    order = np.argsort(d2, axis=1, kind="stable")
    dist, idx = np.full((Q, k), np.inf, dtype), np.full((Q, k), -1, np.int64)
    kk = min(k, S)
    if kk:
        top = order[:, :kk]
        dd = np.take_along_axis(d2, top, 1)
        dist[:, :kk] = np.sqrt(dd)
        idx[:, :kk] = np.where(np.isfinite(dd), top, -1)
    bad = ~np.isfinite(q).all(1)
    return dist, idx, (ST_NONFINITE if bad.any() else 0)


def knn(q, s, k, dilation=1, distance_limit=None, remove_nearest=False, padding_mode="nearest", padding_value=1e10, dtype=np.float64):
    """vision3d/ops/knn.py:30-107 -> (distances, indices)"""
    S = np.asarray(s).shape[0]
    dk = (k - 1) * dilation + 1 + (1 if remove_nearest else 0)
    dist, idx, _ = knn_points(q, s, max(min(dk, S), 1), dtype)
    dist, idx = dist[:, :min(dk, S)], idx[:, :min(dk, S)]
    if remove_nearest:
        dist, idx = dist[:, 1:], idx[:, 1:]
    if dilation > 1:
        dist, idx = dist[:, ::dilation], idx[:, ::dilation]
    dist, idx = dist.copy(), idx.copy()
    if distance_limit is not None:
        far = dist >= dtype(distance_limit)
        if padding_mode == "nearest":
            dist, idx = np.where(far, dist[:, :1], dist), np.where(far, idx[:, :1], idx)
        else:
            dist[far], idx[far] = padding_value, S
    return dist, idx


def knn_interpolate(q, s, feats, k=3, eps=1e-10, distance_limit=None, dtype=np.float64):
    """vision3d/ops/knn_interpolate.py:10-40"""
    dist, idx, _ = knn_points(q, s, k, dtype)
    if distance_limit is not None:
        dist = np.where(dist > dtype(distance_limit), dtype(1e10), dist)
    w = dtype(1.0) / (dist + dtype(eps))
    w = w / w.sum(1, keepdims=True)
    return (np.asarray(feats, dtype)[np.maximum(idx, 0)] * w[:, :, None]).sum(1)


def nn_stats(q, s, distance_limit=np.inf, dtype=np.float64):
    """-> [queries with a nearest support, sum dist, sum dist^2, count(dist < limit)] as float64"""
    dist, idx, _ = knn_points(q, s, 1, dtype)
    have = idx[:, 0] >= 0
    d = dist[have, 0].astype(np.float64)
    return np.array([have.sum(), d.sum(), (d * d).sum(), (dist[have, 0] < dtype(distance_limit)).sum()], np.float64)


def ordered_nn_stats(dist_f32, idx, distance_limit, block):
    """dr_nn_stats_f32's own order on dr_knn_points_f32(k = 1)'s outputs: the `block` queries of a block by the tree lane l += lane l + off,
    off = block / 2 .. 1, the blocks ascending, in double -> the four numbers bit for bit"""
    have = idx >= 0
    d = np.where(have, dist_f32, np.float32(0)).astype(np.float64)
    terms = [have.astype(np.float64), d, d * d, (have & (dist_f32 < np.float32(distance_limit))).astype(np.float64)]
    out = []
    for t in terms:
        nb = (len(t) + block - 1) // block
        v = np.zeros(nb * block)
        v[:len(t)] = t
        v = v.reshape(nb, block)
        off = block // 2
        while off >= 1:
            v = v[:, :off] + v[:, off:2 * off]
            off //= 2
        acc = 0.0
        for b in range(nb):
            acc = acc + v[b, 0]
        out.append(acc)
    return np.array(out, np.float64)


def apply_transform(p, T, dtype=np.float64):
    T = np.asarray(T, dtype)
    return np.asarray(p, dtype) @ T[:3, :3].T + T[:3, 3]


def flow_terms(pred, target, eps=1e-20, dtype=np.float64):
    """-> (|e|, rel) per point, the reference's arithmetic in `dtype`"""
    pred, target = np.asarray(pred, dtype).reshape(-1, 3), np.asarray(target, dtype).reshape(-1, 3)
    d = pred - target
    e = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    ln = np.sqrt((target[:, 0] * target[:, 0] + target[:, 1] * target[:, 1]) + target[:, 2] * target[:, 2])
    with np.errstate(all="ignore"):
        rel = e / (ln + dtype(eps))
    return e, rel


def flow_metrics(pred, target, mask=None, transform=None, strict=(np.inf, np.inf), relaxed=(np.inf, np.inf), outlier=(None, None), eps=1e-20,
                 dtype=np.float64):
    """-> [n, sum |e|, n_strict, n_relaxed, n_outlier, n_within] as float64"""
    pred = np.asarray(pred, dtype).reshape(-1, 3)
    if transform is not None:
        pred = apply_transform(pred, transform, dtype)
    e, rel = flow_terms(pred, target, eps, dtype)
    m = np.ones(len(e), bool) if mask is None else np.asarray(mask).astype(bool)
    t = lambda x: dtype(x)
    out_l = np.zeros(len(e), bool)
    if outlier[0] is not None:
        out_l |= e > t(outlier[0])
    if outlier[1] is not None:
        out_l |= rel > t(outlier[1])
    return np.array([m.sum(), e[m].astype(np.float64).sum(), ((e < t(strict[0])) | (rel < t(strict[1])))[m].sum(),
                     ((e < t(relaxed[0])) | (rel < t(relaxed[1])))[m].sum(), out_l[m].sum(), (e < t(strict[0]))[m].sum()], np.float64)


def _ratio(a, b, nan_to_num):
    if b == 0:
        return 0.0 if nan_to_num else float("nan")
    return a / b


def nonrigid_inlier_ratio(src_c, tgt_c, flows, transform=None, radius=0.04, dtype=np.float64):
    o = flow_metrics(np.asarray(src_c, dtype) + np.asarray(flows, dtype), tgt_c, transform=transform, strict=(radius, -1.0), dtype=dtype)
    return _ratio(o[5], o[0], True)


def nonrigid_fmr(src_c, tgt_c, src, flows, test_indices, transform=None, radius=0.04, distance_limit=0.1, dtype=np.float64):
    src_c, tgt_c, src, flows = (np.asarray(a, dtype) for a in (src_c, tgt_c, src, flows))
    st = src[test_indices]
    pred = st + knn_interpolate(st, src_c, tgt_c - src_c, 3, 1e-10, distance_limit, dtype)
    o = flow_metrics(st + flows[test_indices], pred, transform=transform, strict=(radius, -1.0), dtype=dtype)
    return _ratio(o[5], o[0], True), pred


def scene_flow_accuracy(inputs, targets, a, r, dtype=np.float64):
    o = flow_metrics(inputs, targets, strict=(a, r), dtype=dtype)
    return _ratio(o[2], o[0], False)


def scene_flow_outlier_ratio(inputs, targets, a, r, dtype=np.float64):
    o = flow_metrics(inputs, targets, outlier=(a, r), dtype=dtype)
    return _ratio(o[4], o[0], False)


def corr_coverage(q, s, limit, dtype=np.float64):
    return _ratio(nn_stats(q, s, limit, dtype)[3], np.asarray(q).reshape(-1, 3).shape[0], True)


def chamfer_distance(q, s, squared=False, dtype=np.float64):
    a, b = nn_stats(q, s, dtype=dtype), nn_stats(s, q, dtype=dtype)
    c = 2 if squared else 1
    return _ratio(a[c], a[0], False) + _ratio(b[c], b[0], False)


# ------------------------------------------------------------------------------------------------ the fixture's scenes and screens
def make_scene(name, attempt=0):
    """inputs of scene `name` (float32 arrays); the minting tool raises `attempt` until both screens pass"""
    i, (_, Q, S, dup) = next((i, s) for i, s in enumerate(SCENES) if s[0] == name)
    rng = np.random.default_rng(1000 * i + 77 + 100000 * attempt)
    f = lambda *shape: rng.uniform(-1.0, 1.0, shape).astype(np.float32)
    q, s = f(Q, 3), f(S, 3)
    if dup:                                   # exact duplicates among the supports, put in on purpose: the lower index comes first
        s[S - dup:] = s[:dup]
    q[:min(Q, S) // 4] = s[:min(Q, S) // 4]   # queries that are themselves supports: distance 0, then remove_nearest
    ang = rng.uniform(-0.3, 0.3, 3)
    cx, cy, cz, sx, sy, sz = *np.cos(ang), *np.sin(ang)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R.astype(np.float32), rng.uniform(-0.2, 0.2, 3).astype(np.float32)
    flow = 0.3 * f(Q, 3)                      # ground-truth scene flow of the queries (the "source cloud")
    flow[:3] = 0.0
    scale = rng.choice([0.01, 0.04, 0.09, 0.2, 0.5], (Q, 1)).astype(np.float32)
    pred = (flow + scale * f(Q, 3)).astype(np.float32)
    pred[0] = 0.0                             # a point exactly at target = 0 with |e| = 0, and two with |e| > 0: rel through eps
    tgt_c = (apply_transform(q + flow, T).astype(np.float32) + scale * f(Q, 3)).astype(np.float32)
    motion = (0.2 * f(S, 3)).astype(np.float32)
    test = rng.permutation(Q)[:max(Q // 2, 1)].astype(np.int64)
    return dict(q=q, s=s, feats=f(S, 5), transform=T, flow=flow, pred=pred, tgt_c=tgt_c, s_moved=(s + motion).astype(np.float32), test=test)


def screen_gaps(q, s, rank=SCREEN_RANK):
    """the smallest gap between consecutive sorted float64 distances of any query, through position `rank`, that is not exactly 0"""
    d = np.sort(np.sqrt(d2_matrix(q, s, np.float64)), axis=1)[:, :rank]
    g = np.diff(d, axis=1)
    g = g[g != 0.0]
    return float(g.min()) if g.size else float("inf")


def screen_thresholds(sc):
    """the smallest distance of any compared quantity of the fixture to the threshold it is compared with"""
    m = np.inf
    near = lambda x, thr: float(np.abs(np.asarray(x, np.float64) - thr).min(initial=np.inf))
    d8 = knn_points(sc["q"], sc["s"], min(8, len(sc["s"])))[0]
    m = min(m, near(d8, 0.45), near(knn_points(sc["q"], sc["s"], min(3, len(sc["s"])))[0], INTERP_LIMIT), near(d8[:, :1], COVERAGE_LIMIT))
    e, rel = flow_terms(sc["pred"], sc["flow"])
    for a, r in (STRICT, RELAXED, OUTLIER):
        m = min(m, near(e, a), near(rel[np.isfinite(rel)], r))
    e, _ = flow_terms(apply_transform(sc["q"].astype(np.float64) + sc["flow"], sc["transform"]), sc["tgt_c"])
    m = min(m, near(e, RADIUS))
    st = sc["q"][sc["test"]]
    m = min(m, near(knn_points(st, sc["s"], min(3, len(sc["s"])))[0], NFMR_LIMIT))
    pred = nonrigid_fmr(sc["s"], sc["s_moved"], sc["q"], sc["flow"], sc["test"], sc["transform"], RADIUS, NFMR_LIMIT)[1]
    e, _ = flow_terms(apply_transform(st.astype(np.float64) + sc["flow"][sc["test"]], sc["transform"]), pred)
    return min(m, near(e, RADIUS))
