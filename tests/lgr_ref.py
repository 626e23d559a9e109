"""The RANSAC-free rigid estimators (twentieth set; include/diffreg_hip.h) restated in float64 numpy, and the scenes their fixture is minted
on.  Shared by tools/golden/make_golden_lgr.py and the tests.  The restatement follows the header's rules, not the reference's code: the
distances of the spatial consistency take the difference first, the fit divides the weighted sums by (W + eps) once.  `dtype=np.float32`
evaluates the float32 rules (the residual, the consistency value, allclose) in float32 operation by operation, as the kernels do."""
import numpy as np

ST_OFFSETS, ST_NONFINITE, ST_DEGENERATE, ST_EMPTY = 4, 8, 16, 32
SCREEN_RADIUS = 1e-5          # no verification residual lies this close to acceptance_radius
SCREEN_SCORE = 1e-5           # no score lies this close to confidence_threshold
SCREEN_SV = 1e-3              # s2 >= SCREEN_SV s1 and s2 - s3 >= SCREEN_SV s1 for every fitted H
SCREEN_TOPK = 1e-3            # the k-th and (k + 1)-th row sums differ by at least this
SIGMA = 0.1                   # spatial-consistency sensitivity of the scenes
SCF_K = 6                     # SpatialConsistencyFiltering's num_correspondences on the scenes
EIG_ITERS = 10
DENSE_MAX = 64                # the fixture stores the dense consistency matrices of scenes with at most this many correspondences


# ---------------------------------------------------------------------------------------------- rule 1
def weighted_procrustes(src, tgt, weights=None, weight_threshold=0.0, eps=1e-5, full=False):
    """-> transform [4, 4] float64 (full: also the status flag, H and its singular values)"""
    p, q = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(tgt, np.float64).reshape(-1, 3)
    w = np.ones(len(p)) if weights is None else np.asarray(weights, np.float64).copy()
    w[w < weight_threshold] = 0.0
    W = w.sum()
    inv = 1.0 / (W + eps)
    pc, qc = (w[:, None] * p).sum(0) * inv, (w[:, None] * q).sum(0) * inv
    H = (p - pc).T @ ((w * inv)[:, None] * (q - qc))
    T, flag, sv = np.eye(4), 0, np.zeros(3)
    if not W > 0.0 or not H.any():
        flag = ST_DEGENERATE
    else:
        U, sv, Vt = np.linalg.svd(H)
        V = Vt.T
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(V @ U.T))])
        T[:3, :3] = V @ D @ U.T
    T[:3, 3] = qc - T[:3, :3] @ pc
    return (T, flag, H, sv) if full else T


def residuals(T, src, tgt, dtype=np.float64):
    """the residual rule: |tgt - (R src + t)| with the transform rounded to float32 first"""
    T = np.asarray(T, np.float32).astype(dtype)
    s, t = np.asarray(src, np.float32).astype(dtype), np.asarray(tgt, np.float32).astype(dtype)
    a = [((T[i, 0] * s[:, 0] + T[i, 1] * s[:, 1]) + T[i, 2] * s[:, 2]) + T[i, 3] for i in range(3)]
    dx, dy, dz = t[:, 0] - a[0], t[:, 1] - a[1], t[:, 2] - a[2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def chunks_of(ids, min_local):
    """runs of equal patch id of at least min_local rows -> [(start, end)]"""
    ids = np.asarray(ids)
    if len(ids) == 0:
        return []
    cut = [0] + list(np.nonzero(ids[1:] != ids[:-1])[0] + 1) + [len(ids)]
    return [(int(a), int(b)) for a, b in zip(cut[:-1], cut[1:]) if b - a >= min_local]


def lgr(src, tgt, scores, ids, radius, min_local=3, steps=5, verify=None, dtype=np.float64):
    """local_to_global_registration on one problem -> dict.  verify = (v_src, v_tgt, v_scores) or None (the correspondences themselves).
    `margin` is the smallest |residual - radius| met, `sv` the smallest of s2 / s1 and (s2 - s3) / s1 over every fit."""
    src, tgt = np.asarray(src, np.float32), np.asarray(tgt, np.float32)
    scores = np.asarray(scores, np.float32)
    vs, vt, vw = (src, tgt, scores) if verify is None else [np.asarray(a, np.float32) for a in verify]
    out = dict(status=0, margin=np.inf, sv=np.inf, min_det=np.inf)
    if len(src) == 0 or len(vs) == 0:
        out.update(status=ST_EMPTY, transform=np.eye(4), best_chunk=-1, chunks=[], chunk_counts=np.zeros(0, np.int64),
                   chunk_transforms=np.zeros((0, 4, 4)), final_scores=np.zeros(0, np.float32), masks=[])
        return out
    rad = np.float32(radius)

    def fit(p, q, w):
        T, flag, H, sv = weighted_procrustes(p, q, w, full=True)
        if not flag:
            out["sv"] = min(out["sv"], sv[1] / sv[0], (sv[1] - sv[2]) / sv[0])
            U, _, Vt = np.linalg.svd(H)
            out["min_det"] = min(out["min_det"], np.linalg.det(Vt.T @ U.T))
        return T, flag

    def inl(T):
        r = residuals(T, vs, vt, dtype)
        out["margin"] = min(out["margin"], float(np.abs(r.astype(np.float64) - float(rad)).min()))
        return r < rad.astype(dtype)
    ch = chunks_of(ids, min_local)
    cT = np.zeros((len(ch), 4, 4))
    cc = np.zeros(len(ch), np.int64)
    masks, flag = [], 0
    if ch:
        cm = []
        for j, (a, b) in enumerate(ch):
            cT[j], _ = fit(src[a:b], tgt[a:b], scores[a:b])
            cm.append(inl(cT[j]))
            cc[j] = cm[-1].sum()
        best = int(np.argmax(cc))                    # the first of equal counts
        T = cT[best]
        out["unique_best"] = int((cc == cc[best]).sum()) == 1
    else:
        best = -1
        T, flag = fit(vs, vt, vw)
        out["unique_best"] = True
    cur = vw
    for _ in range(steps):
        m = inl(T)
        masks.append(m)
        cur = np.where(m, vw, np.float32(0.0)).astype(np.float32)
        T, flag = fit(vs, vt, cur)
    out.update(status=flag, transform=T, best_chunk=best, chunks=ch, chunk_counts=cc, chunk_transforms=cT, final_scores=cur, masks=masks)
    return out


# ---------------------------------------------------------------------------------------------- the extraction of forward()
def topk_mask(score, k, axis):
    """the entries among the k largest along `axis` (ties to the lower index, as a stable descending sort)"""
    order = np.argsort(-score, axis=axis, kind="stable")
    top = np.take(order, np.arange(k), axis=axis)
    m = np.zeros(score.shape, bool)
    np.put_along_axis(m, top, True, axis=axis)
    return m


def extract(score_mat, k, src_masks, tgt_masks, global_scores, threshold=0.05, mutual=True, use_dustbin=False, use_global_score=False,
            use_logits=True):
    """LocalGlobalRegistration.forward up to the correspondence list -> (b, i, j int64; scores float32) in torch.nonzero order, and the
    smallest |score - threshold| and the smallest gap at a k-th place of the float32 score matrix"""
    s = np.asarray(score_mat, np.float32)
    if use_logits:
        s = np.exp(s).astype(np.float32)
    row, col = topk_mask(s, k, 2), topk_mask(s, k, 1)
    m = (row & col) if mutual else (row | col)
    m &= s > np.float32(threshold)
    m &= np.asarray(src_masks, bool)[:, :, None] & np.asarray(tgt_masks, bool)[:, None, :]
    margin = float(np.abs(s.astype(np.float64) - threshold).min())
    srt_r, srt_c = -np.sort(-s, axis=2), -np.sort(-s, axis=1)
    gap = np.inf
    if k < s.shape[2]:
        gap = min(gap, float((srt_r[:, :, k - 1] - srt_r[:, :, k]).min()), float((srt_c[:, k - 1, :] - srt_c[:, k, :]).min()))
    if use_dustbin:
        m, s = m[:, :-1, :-1], s[:, :-1, :-1]
    if use_global_score:
        s = s * np.asarray(global_scores, np.float32)[:, None, None]
    b, i, j = np.nonzero(m)
    return b.astype(np.int64), i.astype(np.int64), j.astype(np.int64), s[b, i, j].astype(np.float32), margin, gap


def forward(sc, dtype=np.float64):
    """the whole forward of a scene -> (b, i, j, src_corr, tgt_corr, corr_scores (the verification set), lgr dict)"""
    o = sc["opts"]
    b, i, j, s, margin, gap = extract(sc["score_mat"], o["k"], sc["src_masks"], sc["tgt_masks"], sc["global_scores"], o["threshold"], o["mutual"],
                                      o["use_dustbin"], o["use_global_score"], o["use_logits"])
    src, tgt = sc["src_knn_points"][b, i], sc["tgt_knn_points"][b, j]
    verify, sel = None, np.arange(len(s))
    mg = o["max_global"]
    if mg is not None and len(s) > mg:
        sel = np.argsort(-s, kind="stable")[:mg]
        verify = (src[sel], tgt[sel], s[sel])
    r = lgr(src, tgt, s, b, o["radius"], o["min_local"], o["steps"], verify, dtype)
    r.update(extract_margin=margin, extract_gap=gap, sel=sel)
    return b, i, j, src[sel], tgt[sel], s[sel], r


# ---------------------------------------------------------------------------------------------- spatial consistency, power iteration
def spatial_consistency(q_src, q_tgt, s_src=None, s_tgt=None, sigma=SIGMA, dtype=np.float64):
    s_src, s_tgt = (q_src if s_src is None else s_src), (q_tgt if s_tgt is None else s_tgt)
    f = lambda a: np.asarray(a, np.float32).astype(dtype)

    def dist(a, b):
        a, b = f(a), f(b)
        dx, dy, dz = a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1], a[:, None, 2] - b[None, :, 2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz)
    delta = np.abs(dist(q_src, s_src) - dist(q_tgt, s_tgt))
    sg = np.float32(sigma).astype(dtype)
    return np.maximum(dtype(1.0) - (delta * delta) / (sg * sg), dtype(0.0))


def sc_bar(sigma, *clouds):
    """bound on the difference between two float32 evaluations (or a float32 and the float64 one) of ONE consistency value, u = 2^-24:
    d2 = (dx dx + dy dy) + dz dz carries at most 5u relative, its root 3.5u, so each distance errs by at most 3.5u dmax and delta by
    8u dmax with its own rounding; where the value is positive delta <= sigma, so d sc = (2 delta / sigma^2) d delta <= (2 / sigma) 8u dmax,
    plus 3u for the square, the quotient and the difference at a scale below 1"""
    u = 2.0 ** -24
    dmax = 2.0 * np.sqrt(3.0) * max(float(np.abs(c).max()) for c in clouds)
    return (2.0 / sigma) * 8.0 * u * dmax + 3.0 * u


def leading_eigenvector(mat, num_iterations=EIG_ITERS, dtype=np.float64):
    """power iteration with torch.allclose's stop -> (vector, iterations that ran, per iteration max |a - b| / (1e-8 + 1e-5 |b|))"""
    m = np.asarray(mat).astype(dtype)
    v = np.ones(m.shape[0], dtype)
    ratios, it = [], 0
    for it in range(1, num_iterations + 1):
        y = (m @ v).astype(dtype)
        new = (y / max(dtype(np.sqrt((y.astype(np.float64) ** 2).sum())), dtype(1e-12))).astype(dtype)
        ratios.append(float((np.abs(new - v) / (dtype(1e-8) + dtype(1e-5) * np.abs(v))).max()) if len(v) else 0.0)
        v = new
        if ratios[-1] <= 1.0:
            break
    return v, it, ratios


# ---------------------------------------------------------------------------------------------- scenes
def rigid(rng):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(0.3, 1.2)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    return R, rng.uniform(-0.5, 0.5, size=3)


OPTS = dict(k=1, radius=0.1, mutual=True, threshold=0.05, use_dustbin=False, use_global_score=False, use_logits=True, min_local=3,
            max_global=None, steps=5, need_full=False)      # need_full: the power iteration must run all EIG_ITERS iterations without stopping
# (name, K, matches per patch (negative: an outlier patch of that many matches; "m3": three mirrored points), option overrides, masked rows)
SCENES = [
    ("base", 10, [6, 7, -6, 8, -5, 6, 9, -7, 5, 6, "m3", "m6", 7], {}, 0),
    ("min_local_edges", 8, [2, 3, 4, 2, 5, 3, 6, "m3"], dict(k=2), 0),
    ("wave_edges", 66, [63, 64, 65], dict(steps=1), 0),
    ("no_valid_chunk", 8, [2, 2, 1, 2, 2, 2], {}, 0),
    ("one_valid_chunk", 8, [2, 6, 2, 1], {}, 0),
    ("masked_rows", 10, [7, 8, -6, 7, 8, "m3"], {}, 2),
    ("dustbin", 9, [6, 7, -5, 8, 6, "m3"], dict(use_dustbin=True), 0),
    ("global_score", 9, [6, 7, -5, 8, 6, "m3"], dict(use_global_score=True), 0),
    ("probabilities", 9, [6, 7, -5, 8, 6, "m3"], dict(use_logits=False, mutual=False, k=2), 0),
    ("max_global", 10, [8, 9, -6, 8, 9, 7, "m3"], dict(max_global=30), 0),
    ("power_runs_out", 10, [8, "b8", 9, "b9", 7, "b7", 8], dict(need_full=True), 0),
]
E2E = ("end_to_end", 12, [8, -7, 9, -8, 8, -9, 9, -8, 10, -7], {}, 0)      # 50 % outlier patches
NAMES = [s[0] for s in SCENES]


def make_scene(spec, seed):
    name, K, patches, over, masked = spec
    rng = np.random.default_rng(seed)
    o = dict(OPTS, **over)
    R, t = rigid(rng)
    if any(isinstance(m, str) and m[0] == "b" for m in patches):
        R2, t2 = rigid(rng)
    B = len(patches)
    Ks = K + 1 if o["use_dustbin"] else K
    src = np.zeros((B, K, 3), np.float32)
    tgt = np.zeros((B, K, 3), np.float32)
    prob = rng.uniform(1e-4, 2e-2, size=(B, Ks, Ks))             # far below the threshold
    src_m, tgt_m = np.ones((B, Ks), bool), np.ones((B, Ks), bool)
    for b, m in enumerate(patches):
        centre = rng.uniform(-1.0, 1.0, size=3)
        p = centre + rng.uniform(-0.3, 0.3, size=(K, 3))
        perm = rng.permutation(K)
        q = np.empty((K, 3))
        if isinstance(m, str) and m[0] == "b":                   # a patch that follows a SECOND rigid motion: two consistent clusters of
            n = int(m[1:])                                       # similar size, so the power iteration converges slowly
            q[perm] = p @ R2.T + t2 + rng.normal(scale=rng.uniform(0.003, 0.01), size=(K, 3))
        elif isinstance(m, str):                                 # points and their mirror images: det(V U^T) < 0 before the sign fix
            n = int(m[1:])
            if n == 3:
                p[:3] = centre + np.array([[0.3, 0.0, 0.0], [0.0, 0.2, 0.0], [-0.1, -0.15, 0.05]])
            q[perm] = p * np.array([1.0, 1.0, -1.0]) + rng.uniform(-1, 1, size=3)
        elif m < 0:
            n = -m
            q[perm] = rng.uniform(-1.5, 1.5, size=(K, 3))
        else:
            n = m
            q[perm] = p @ R.T + t + rng.normal(scale=rng.uniform(0.003, 0.03), size=(K, 3))       # graded noise: the chunks' counts differ
        src[b], tgt[b] = p, q
        for i in range(n):
            prob[b, i, perm[i]] = rng.uniform(0.3, 0.9)
        if masked and b < masked:
            src_m[b, 0] = False                                  # removes a matched row
    if o["use_dustbin"]:
        src_m[:, -1] = False
        tgt_m[:, -1] = False
    score = (np.log(prob) if o["use_logits"] else prob).astype(np.float32)
    return dict(name=name, opts=o, src_knn_points=src, tgt_knn_points=tgt, src_masks=src_m, tgt_masks=tgt_m, score_mat=score,
                global_scores=rng.uniform(0.5, 1.0, size=B).astype(np.float32), R=R, t=t)


def screens(sc):
    """-> dict of the margins of a scene, `ok` when every screen passes.  Nothing is dropped: the figures range over every correspondence."""
    b, i, j, vs, vt, vw, r64 = forward(sc, np.float64)
    _, _, _, _, _, _, r32 = forward(sc, np.float32)
    o = sc["opts"]
    same = (len(r64["masks"]) == len(r32["masks"]) and all(np.array_equal(a, c) for a, c in zip(r64["masks"], r32["masks"])) and
            np.array_equal(r64["chunk_counts"], r32["chunk_counts"]) and r64["best_chunk"] == r32["best_chunk"])
    m = dict(radius=r64["margin"], sv=r64["sv"], extract=r64["extract_margin"], gap=r64["extract_gap"], n_corr=len(b), n_verify=len(vw),
             unique_best=bool(r64["unique_best"]), f32_same=bool(same), min_det=r64["min_det"])
    ok = (m["radius"] >= SCREEN_RADIUS and m["sv"] >= SCREEN_SV and m["extract"] >= SCREEN_SCORE and m["gap"] > 0 and same and
          m["unique_best"] and len(b) > 0)
    # power iteration and the top-k of the row sums, on the verification set
    mat64, mat32 = spatial_consistency(vs, vt, dtype=np.float64), spatial_consistency(vs, vt, dtype=np.float32)
    _, it64, ra64 = leading_eigenvector(mat64, EIG_ITERS, np.float64)
    _, it32, ra32 = leading_eigenvector(mat32, EIG_ITERS, np.float32)
    early = [x for ra in (ra64[:it64 - 1], ra32[:it32 - 1]) for x in ra]
    stopped = ra64[-1] <= 1.0
    m.update(eig_iterations=it64, eig_stopped=bool(stopped), eig_early=min(early) if early else np.inf,
             eig_last=max(ra64[-1], ra32[-1]) if stopped else 0.0)
    ok = ok and it64 == it32 and m["eig_early"] >= 2.0 and m["eig_last"] <= 0.5
    if not stopped:
        ok = ok and min(ra64[-1], ra32[-1]) >= 2.0
    if o["need_full"]:
        ok = ok and not stopped
    sums = np.sort(mat64.sum(1))[::-1]
    kk = min(SCF_K, len(sums))
    m["topk_gap"] = float(sums[kk - 1] - sums[kk]) if kk < len(sums) else np.inf
    m["ok"] = bool(ok and m["topk_gap"] >= SCREEN_TOPK)
    return m


MARGIN_KEYS = ("radius", "sv", "extract", "gap", "eig_early", "eig_last", "topk_gap", "min_det")


def find_scene(spec, first_seed, budget=400):
    for seed in range(first_seed, first_seed + budget):
        sc = make_scene(spec, seed)
        m = screens(sc)
        if m["ok"]:
            return sc, m, seed
    raise RuntimeError("no scene of %s passes the screens within %d attempts" % (spec[0], budget))


def tie_scene():
    """two chunks that explain the SAME number of verification correspondences (each its own four points, exactly): the lower index wins"""
    a = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    src = np.concatenate([a, a + np.float32(4.0)])
    tgt = np.concatenate([a + np.float32([0.5, 0, 0]), a + np.float32(4.0) + np.float32([0, 8.0, 0])])
    return src, tgt, np.full(8, 0.5, np.float32), np.array([0] * 4 + [1] * 4, np.int32)


def pose_errors(T, R, t):
    """(rotation error in degrees, translation error) of a 4 x 4 estimate against (R, t)"""
    c = (np.trace(np.asarray(T)[:3, :3].T @ R) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(np.linalg.norm(np.asarray(T)[:3, 3] - t))
