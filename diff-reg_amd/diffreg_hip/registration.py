"""vision3d's RANSAC-free rigid estimators on the device (twentieth set after ABI 0.7.0; csrc/lgr.hip, rules in include/diffreg_hip.h):

    weighted_procrustes, WeightedProcrustes                vision3d/ops/weighted_procrustes.py, vision3d/layers/weighted_procrustes.py
    LocalGlobalRegistration                                vision3d/models/geotransformer/local_global_registration.py
    local_to_global_registration_pairs                     the same for P pairs in one call (ragged)
    spatial_consistency, cross_spatial_consistency         vision3d/ops/spatial_consistency.py
    spatial_consistency_counts, SpatialConsistencyFiltering  vision3d/models/geotransformer/spatial_consistency_filtering.py
    leading_eigenvector                                    vision3d/ops/eigenvector.py

Tensors on a ROCm device go through the library; CPU tensors take a plain-torch statement of the same rules (double sums, float32 residual
and consistency rules), as elsewhere in the package.  Nothing here reads the device back except where a docstring says so."""
import torch
import torch.nn as nn

from . import lib
from .lib import check, ptr, stream_of

_raw = lib.raw()
SELECT_MAX_K, SELECT_MAX_CELLS = 8, 262144        # what dr_mutual_topk_select_f32 accepts


def _f32(x):
    return x.to(torch.float32).contiguous()


def _regular_offsets(B, N, device):
    return (torch.arange(B + 1, device=device, dtype=torch.int64) * N).to(torch.int32)


def _i32(dev, n, fill=None):
    return torch.empty(n, dtype=torch.int32, device=dev) if fill is None else torch.full((n,), fill, dtype=torch.int32, device=dev)


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


# ---------------------------------------------------------------------------------------------- CPU statements of the rules
def _cpu_fit(src, tgt, w, thr, eps):
    p, q = src.double(), tgt.double()
    w = torch.ones(p.shape[0], dtype=torch.float32) if w is None else w.to(torch.float32)
    w = torch.where(w < thr, torch.zeros_like(w), w).double()
    W = w.sum()
    inv = 1.0 / (W + float(eps))
    pc, qc = (w[:, None] * p).sum(0) * inv, (w[:, None] * q).sum(0) * inv
    H = (p - pc).T @ ((w * inv)[:, None] * (q - qc))
    T = torch.eye(4, dtype=torch.float64)
    if bool(W > 0) and bool(H.abs().sum() > 0):
        U, _, Vh = torch.linalg.svd(H)
        V = Vh.T
        D = torch.diag(torch.tensor([1.0, 1.0, float(torch.sign(torch.det(V @ U.T)))], dtype=torch.float64))
        T[:3, :3] = V @ D @ U.T
    T[:3, 3] = qc - T[:3, :3] @ pc
    return T.float()


def _cpu_inliers(T, src, tgt, radius):
    T, s, t = T.float(), src.float(), tgt.float()
    a = [((T[i, 0] * s[:, 0] + T[i, 1] * s[:, 1]) + T[i, 2] * s[:, 2]) + T[i, 3] for i in range(3)]
    dx, dy, dz = t[:, 0] - a[0], t[:, 1] - a[1], t[:, 2] - a[2]
    return torch.sqrt((dx * dx + dy * dy) + dz * dz) < torch.tensor(radius, dtype=torch.float32)


def _cpu_lgr(src, tgt, scores, ids, vs, vt, vw, radius, min_local, steps, thr, eps):
    n = ids.shape[0]
    cut = [0] + (torch.nonzero(ids[1:] != ids[:-1])[:, 0] + 1).tolist() + [n] if n else [0]
    chunks = [(a, b) for a, b in zip(cut[:-1], cut[1:]) if b - a >= min_local]
    if chunks:
        cT = [_cpu_fit(src[a:b], tgt[a:b], scores[a:b], thr, eps) for a, b in chunks]
        counts = torch.tensor([int(_cpu_inliers(T, vs, vt, radius).sum()) for T in cT])
        best = int(torch.argmax(counts))
        best = int(torch.nonzero(counts == counts[best])[0, 0])          # the lowest index among equal counts
        T = cT[best]
    else:
        best, T = -1, _cpu_fit(vs, vt, vw, thr, eps)
    cur = vw
    for _ in range(steps):
        cur = torch.where(_cpu_inliers(T, vs, vt, radius), vw, torch.zeros_like(vw))
        T = _cpu_fit(vs, vt, cur, thr, eps)
    return T, best, cur


def _cpu_sc(qs, qt, ss, st, sigma):
    def dist(a, b):
        a, b = a.float(), b.float()
        dx, dy, dz = a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1], a[:, None, 2] - b[None, :, 2]
        return torch.sqrt((dx * dx + dy * dy) + dz * dz)
    delta = (dist(qs, ss) - dist(qt, st)).abs()
    sg = torch.tensor(sigma, dtype=torch.float32)
    return torch.clamp(1.0 - (delta * delta) / (sg * sg), min=0.0)


def _cpu_power(mat, num_iterations):
    m = mat.double()
    v = torch.ones(m.shape[0], dtype=torch.float32)
    it = 0
    for it in range(1, num_iterations + 1):
        y = (m @ v.double()).float()
        new = y / torch.clamp(y.double().pow(2).sum().sqrt().float(), min=1e-12)
        stop = bool(((new - v).abs() <= 1e-8 + 1e-5 * v.abs()).all())
        v = new
        if stop:
            break
    return v, it


# ---------------------------------------------------------------------------------------------- rule 1
def weighted_procrustes_groups(src_points, tgt_points, offsets, weights=None, weight_threshold=0.0, eps=1e-5, wave_limit=-1, host_offsets=None):
    """G groups of stacked (n, 3) points under int32 device offsets (G + 1) -> (transforms (G, 4, 4), status (G,) int32).  wave_limit picks
    the path (see dr_weighted_procrustes_f32); both paths give the same bits."""
    lib.ensure_init()
    src, tgt = _f32(src_points), _f32(tgt_points)
    w = None if weights is None else _f32(weights)
    G, dev = offsets.numel() - 1, src.device
    T = torch.empty(max(G, 1), 16, dtype=torch.float32, device=dev)
    st = _i32(dev, max(G, 1), 0)
    hp = None if host_offsets is None else host_offsets.ctypes.data
    check(_raw.dr_weighted_procrustes_f32(G, src.shape[0], ptr(src), ptr(tgt), ptr(w), ptr(offsets), hp, float(weight_threshold), float(eps),
                                          int(wave_limit), ptr(T), ptr(st), stream_of(src)))
    return T[:G].view(G, 4, 4), st[:G]


def weighted_procrustes(src_points, tgt_points, weights=None, weight_threshold=0.0, eps=1e-5):
    """vision3d.ops.weighted_procrustes: (N, 3) or (B, N, 3) -> (4, 4) or (B, 4, 4).  A group without positive weight gives the identity."""
    squeeze = src_points.dim() == 2
    s = src_points[None] if squeeze else src_points
    t = tgt_points[None] if squeeze else tgt_points
    w = None if weights is None else (weights[None] if squeeze else weights)
    B, N = s.shape[0], s.shape[1]
    if not s.is_cuda:
        out = torch.stack([_cpu_fit(s[b], t[b], None if w is None else w[b], weight_threshold, eps) for b in range(B)]) if B else s.new_zeros(0, 4, 4)
    else:
        out, _ = weighted_procrustes_groups(s.reshape(-1, 3), t.reshape(-1, 3), _regular_offsets(B, N, s.device),
                                            None if w is None else w.reshape(-1), weight_threshold, eps)
    return out[0] if squeeze else out


class WeightedProcrustes(nn.Module):
    def __init__(self, weight_threshold=0.0, eps=1e-5):
        super().__init__()
        self.weight_threshold = weight_threshold
        self.eps = eps

    def forward(self, src_points, tgt_points, weights=None):
        return weighted_procrustes(src_points, tgt_points, weights=weights, weight_threshold=self.weight_threshold, eps=self.eps)

    def extra_repr(self):
        return "weight_threshold=%g, eps=%g" % (self.weight_threshold, self.eps)


# ---------------------------------------------------------------------------------------------- local-to-global registration
def local_to_global_registration_pairs(src_points, tgt_points, scores, patch_ids, offsets, acceptance_radius, min_local_correspondences=3,
                                       num_refinement_steps=5, verify=None, weight_threshold=0.0, eps=1e-5, hypotheses=False,
                                       host_offsets=None, host_verify_offsets=None):
    """local_to_global_registration for P pairs in one call (five launches, nothing read back).  src_points / tgt_points (n, 3), scores (n,),
    patch_ids (n,) non-descending inside a pair, offsets (P + 1,) int32 on the device.  verify = (v_src, v_tgt, v_scores, v_offsets), the
    verification set of every pair (default: the correspondences themselves).  -> dict(transform (P, 4, 4), best_chunk (P,), final_scores
    (n_verify,), status (P,); with hypotheses=True also chunk_transforms (n, 4, 4), chunk_counts (n,), chunk_offsets (P + 1,))."""
    src, tgt, sc = _f32(src_points), _f32(tgt_points), _f32(scores)
    ids = patch_ids.to(torch.int32).contiguous()
    off = offsets.to(torch.int32).contiguous()
    vs, vt, vw, voff = (src, tgt, sc, off) if verify is None else (_f32(verify[0]), _f32(verify[1]), _f32(verify[2]), verify[3].to(torch.int32).contiguous())
    P, n, nv, dev = off.numel() - 1, src.shape[0], vs.shape[0], src.device
    if not src.is_cuda:
        o, vo = off.tolist(), voff.tolist()
        T, best, fin = [], [], torch.zeros(nv)
        for p in range(P):
            a, b, c, d = o[p], o[p + 1], vo[p], vo[p + 1]
            if b == a or d == c:
                T.append(torch.eye(4)), best.append(-1)
                continue
            Tp, bp, cur = _cpu_lgr(src[a:b], tgt[a:b], sc[a:b], ids[a:b], vs[c:d], vt[c:d], vw[c:d], acceptance_radius,
                                   min_local_correspondences, num_refinement_steps, weight_threshold, eps)
            T.append(Tp), best.append(bp)
            fin[c:d] = cur
        return dict(transform=torch.stack(T) if P else torch.zeros(0, 4, 4), best_chunk=torch.tensor(best, dtype=torch.int32), final_scores=fin,
                    status=torch.tensor([32 if o[p + 1] == o[p] else 0 for p in range(P)], dtype=torch.int32))
    lib.ensure_init()
    out = dict(transform=torch.empty(max(P, 1), 16, device=dev), best_chunk=_i32(dev, max(P, 1), -1), final_scores=torch.zeros(max(nv, 1), device=dev),
               status=_i32(dev, max(P, 1), 0))
    cT = cc = co = None
    if hypotheses:
        cT, cc, co = torch.zeros(max(n, 1), 16, device=dev), _i32(dev, max(n, 1), 0), _i32(dev, P + 1, 0)
    wsb = _raw.dr_lgr_workspace_bytes(P, n)
    ws = _ws(wsb, dev)
    hp = lambda h: None if h is None else h.ctypes.data
    check(_raw.dr_lgr_f32(P, n, ptr(src), ptr(tgt), ptr(sc), ptr(ids), ptr(off), nv, ptr(vs), ptr(vt), ptr(vw), ptr(voff), hp(host_offsets),
                          hp(host_verify_offsets), float(acceptance_radius), int(min_local_correspondences), int(num_refinement_steps),
                          float(weight_threshold), float(eps), ptr(out["transform"]), ptr(out["best_chunk"]), ptr(out["final_scores"]), ptr(cT),
                          ptr(cc), ptr(co), ptr(out["status"]), ptr(ws), wsb, stream_of(src)))
    out = dict(transform=out["transform"][:P].view(P, 4, 4), best_chunk=out["best_chunk"][:P], final_scores=out["final_scores"][:nv],
               status=out["status"][:P])
    if hypotheses:
        out.update(chunk_transforms=cT[:n].view(n, 4, 4), chunk_counts=cc[:n], chunk_offsets=co)
    return out


class LocalGlobalRegistration(nn.Module):
    """Point matching with local-to-global registration; the reference's constructor and forward.  On the device forward reads ONE word back
    (the number of correspondences, to size the outputs); forward(..., padded=True) reads nothing and returns capacity-sized tensors, whose
    rows behind the count are unspecified, plus the device count."""

    def __init__(self, k, acceptance_radius, mutual=True, confidence_threshold=0.05, use_dustbin=False, use_global_score=False,
                 use_logits=True, min_local_correspondences=3, max_global_correspondences=None, num_refinement_steps=5):
        super().__init__()
        self.k = k
        self.acceptance_radius = acceptance_radius
        self.mutual = mutual
        self.confidence_threshold = confidence_threshold
        self.use_dustbin = use_dustbin
        self.use_global_score = use_global_score
        self.use_logits = use_logits
        self.min_local_correspondences = min_local_correspondences
        self.max_global_correspondences = max_global_correspondences
        self.num_refinement_steps = num_refinement_steps
        self.procrustes = WeightedProcrustes()

    def _cpu_forward(self, src_knn_points, tgt_knn_points, src_knn_masks, tgt_knn_masks, score_mat, global_scores):
        s = score_mat.float()
        if self.use_logits:
            s = torch.exp(s)
        k = self.k
        row = torch.zeros_like(s, dtype=torch.bool).scatter_(2, torch.argsort(s, dim=2, descending=True, stable=True)[:, :, :k], True)
        col = torch.zeros_like(s, dtype=torch.bool).scatter_(1, torch.argsort(s, dim=1, descending=True, stable=True)[:, :k, :], True)
        m = (row & col) if self.mutual else (row | col)
        m = m & (s > self.confidence_threshold) & src_knn_masks.bool()[:, :, None] & tgt_knn_masks.bool()[:, None, :]
        if self.use_dustbin:
            m, s = m[:, :-1, :-1], s[:, :-1, :-1]
        if self.use_global_score:
            s = s * global_scores.float().view(-1, 1, 1)
        b, i, j = torch.nonzero(m, as_tuple=True)
        src, tgt, sc = src_knn_points.float()[b, i], tgt_knn_points.float()[b, j], s[b, i, j]
        vs, vt, vw = src, tgt, sc
        mg = self.max_global_correspondences
        if mg is not None and sc.shape[0] > mg:
            sel = torch.argsort(sc, descending=True, stable=True)[:mg]
            vs, vt, vw = src[sel], tgt[sel], sc[sel]
        if sc.shape[0] == 0:
            return vs, vt, vw, torch.eye(4)
        T, _, _ = _cpu_lgr(src, tgt, sc, b, vs, vt, vw, self.acceptance_radius, self.min_local_correspondences, self.num_refinement_steps, 0.0,
                           1e-5)
        return vs, vt, vw, T

    def forward(self, src_knn_points, tgt_knn_points, src_knn_masks, tgt_knn_masks, score_mat, global_scores, padded=False):
        if not score_mat.is_cuda:
            return self._cpu_forward(src_knn_points, tgt_knn_points, src_knn_masks, tgt_knn_masks, score_mat, global_scores)
        lib.ensure_init()
        s = _f32(score_mat)
        B, Ks, Ms = s.shape
        if self.k > SELECT_MAX_K:
            raise ValueError("LocalGlobalRegistration: k = %d, the device selection takes k <= %d" % (self.k, SELECT_MAX_K))
        if Ks * Ms > SELECT_MAX_CELLS:
            raise ValueError("LocalGlobalRegistration: a %d x %d score matrix, the device selection takes at most %d cells"
                             % (Ks, Ms, SELECT_MAX_CELLS))
        if self.use_logits:
            s = torch.exp(s)
        dev = s.device
        rm, cm = src_knn_masks.to(torch.bool), tgt_knn_masks.to(torch.bool)
        if self.use_dustbin:                         # dropping the dustbin row and column after the selection = masking them in it
            rm, cm = rm.clone(), cm.clone()
            rm[:, -1] = False
            cm[:, -1] = False
        cap = B * (min(Ks, Ms) if self.mutual else (Ks + Ms)) * self.k
        idx = torch.zeros(max(cap, 1), 3, dtype=torch.int64, device=dev)        # rows behind the count stay (0, 0, 0): safe to gather with
        sc = torch.zeros(max(cap, 1), device=dev)
        tot = _i32(dev, 1, 0)
        wsb = _raw.dr_mutual_topk_workspace_bytes(B, Ks, Ms)
        ws = _ws(wsb, dev)
        ru8, cu8 = lib.mask_u8(rm), lib.mask_u8(cm)
        check(_raw.dr_mutual_topk_select_f32(B, Ks, Ms, ptr(s), int(self.k), 1, 1, float(self.confidence_threshold), 1 if self.mutual else 0,
                                             ptr(ru8), ptr(cu8), ptr(idx), ptr(sc), cap, ptr(tot), ptr(ws), wsb,
                                             stream_of(s)))
        count = tot.clamp(max=cap)
        b, i, j = idx[:, 0], idx[:, 1], idx[:, 2]
        if self.use_global_score:
            sc = sc * _f32(global_scores)[b]
        src, tgt = _f32(src_knn_points)[b, i], _f32(tgt_knn_points)[b, j]
        off = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), count])
        verify, vs, vt, vw, vcount = None, src, tgt, sc, count
        mg = self.max_global_correspondences
        if mg is not None and mg < max(cap, 1):
            live = torch.arange(sc.shape[0], device=dev) < count
            top = torch.topk(torch.where(live, sc, torch.full_like(sc, -float("inf"))), mg).indices
            sel = torch.where(count > mg, top, torch.arange(mg, device=dev))
            vs, vt, vw, vcount = src[sel], tgt[sel], sc[sel], count.clamp(max=mg)
            verify = (vs, vt, vw, torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), vcount]))
        r = local_to_global_registration_pairs(src, tgt, sc, b, off, self.acceptance_radius, self.min_local_correspondences,
                                               self.num_refinement_steps, verify)
        T = r["transform"][0]
        if padded:
            return vs, vt, vw, T, vcount
        n = int(vcount.item())                       # the one word read back
        return vs[:n], vt[:n], vw[:n], T

    def extra_repr(self):
        return ("k=%d, radius=%g, mutual=%s, threshold=%g, use_dustbin=%s, use_global_score=%s, min_local_corr=%d, max_global_corr=%s, "
                "refinement=%d" % (self.k, self.acceptance_radius, self.mutual, self.confidence_threshold, self.use_dustbin,
                                   self.use_global_score, self.min_local_correspondences, self.max_global_correspondences,
                                   self.num_refinement_steps))


# ---------------------------------------------------------------------------------------------- spatial consistency
def _sc_batched(x):
    lead = x.shape[:-2]
    return lead, x.reshape((-1,) + tuple(x.shape[-2:]))


def cross_spatial_consistency(q_src_corr_points, q_tgt_corr_points, s_src_corr_points, s_tgt_corr_points, sigma):
    """(*, N, 3) x (*, M, 3) -> (*, N, M): max(1 - (| |p_i - p_j| - |q_i - q_j| |)^2 / sigma^2, 0)"""
    lead, qs = _sc_batched(q_src_corr_points)
    qt, ss, st = _sc_batched(q_tgt_corr_points)[1], _sc_batched(s_src_corr_points)[1], _sc_batched(s_tgt_corr_points)[1]
    B, N, M = qs.shape[0], qs.shape[1], ss.shape[1]
    if not qs.is_cuda:
        out = torch.stack([_cpu_sc(qs[b], qt[b], ss[b], st[b], sigma) for b in range(B)]) if B else qs.new_zeros(0, N, M)
        return out.reshape(lead + (N, M))
    lib.ensure_init()
    qs, qt, ss, st = [_f32(a).reshape(-1, 3) for a in (qs, qt, ss, st)]
    dev = qs.device
    out = torch.empty(B * N * M if B * N * M else 1, device=dev)
    mo = torch.arange(B + 1, device=dev, dtype=torch.int64) * (N * M)
    qo, so, status = _regular_offsets(B, N, dev), _regular_offsets(B, M, dev), _i32(dev, max(B, 1), 0)     # named: alive until the call returns
    check(_raw.dr_spatial_consistency_f32(B, B * N, ptr(qs), ptr(qt), ptr(qo), B * M, ptr(ss), ptr(st), ptr(so), None, None, float(sigma), ptr(mo),
                                          ptr(out), ptr(status), stream_of(qs)))
    return out[:B * N * M].reshape(lead + (N, M))


def spatial_consistency(src_corr_points, tgt_corr_points, sigma):
    """(*, N, 3) -> (*, N, N)"""
    return cross_spatial_consistency(src_corr_points, tgt_corr_points, src_corr_points, tgt_corr_points, sigma)


def spatial_consistency_counts(src_corr_points, tgt_corr_points, sigma, s_src_corr_points=None, s_tgt_corr_points=None):
    """the row sums of the (cross) spatial-consistency matrix without the matrix: (*, N, 3) -> (*, N)"""
    ss_in = src_corr_points if s_src_corr_points is None else s_src_corr_points
    st_in = tgt_corr_points if s_tgt_corr_points is None else s_tgt_corr_points
    lead, qs = _sc_batched(src_corr_points)
    qt, ss, st = _sc_batched(tgt_corr_points)[1], _sc_batched(ss_in)[1], _sc_batched(st_in)[1]
    B, N, M = qs.shape[0], qs.shape[1], ss.shape[1]
    if not qs.is_cuda:
        out = torch.stack([_cpu_sc(qs[b], qt[b], ss[b], st[b], sigma).double().sum(1).float() for b in range(B)]) if B else qs.new_zeros(0, N)
        return out.reshape(lead + (N,))
    lib.ensure_init()
    qs, qt, ss, st = [_f32(a).reshape(-1, 3) for a in (qs, qt, ss, st)]
    dev = qs.device
    out = torch.zeros(max(B * N, 1), device=dev)
    qo, so, status = _regular_offsets(B, N, dev), _regular_offsets(B, M, dev), _i32(dev, max(B, 1), 0)     # named: alive until the call returns
    check(_raw.dr_sc_row_sums_f32(B, B * N, ptr(qs), ptr(qt), ptr(qo), B * M, ptr(ss), ptr(st), ptr(so), None, None, float(sigma), None, ptr(out),
                                  ptr(status), stream_of(qs)))
    return out[:B * N].reshape(lead + (N,))


class SpatialConsistencyFiltering(nn.Module):
    def __init__(self, num_correspondences, sigma):
        super().__init__()
        self.sigma = sigma
        self.num_correspondences = num_correspondences

    def forward(self, src_corr_points, tgt_corr_points):
        counts = spatial_consistency_counts(src_corr_points, tgt_corr_points, self.sigma)
        return counts.topk(k=self.num_correspondences, largest=True)[1]

    def extra_repr(self):
        return "num_correspondences=%d, sigma=%g" % (self.num_correspondences, self.sigma)


def leading_eigenvector(mat_or_points, method="power", num_iterations=10, tgt_points=None, sigma=None, return_iterations=False):
    """vision3d.ops.leading_eigenvector of mat (*, M, M); with tgt_points and sigma, of the spatial-consistency matrix of the correspondences
    mat_or_points (*, M, 3) / tgt_points (*, M, 3) without building it.  method="torch" is torch.linalg.eigh.  return_iterations adds the
    iterations that ran per matrix (int32)."""
    assert method in ("power", "torch"), "Unsupported method: %s." % method
    points = tgt_points is not None
    if method == "torch":
        mat = spatial_consistency(mat_or_points, tgt_points, sigma) if points else mat_or_points
        return torch.linalg.eigh(mat)[1][..., -1]
    lead, a = _sc_batched(mat_or_points)
    B, M = a.shape[0], a.shape[1]
    if not a.is_cuda:
        t = _sc_batched(tgt_points)[1] if points else None
        res = [_cpu_power(_cpu_sc(a[b], t[b], a[b], t[b], sigma) if points else a[b], num_iterations) for b in range(B)]
        vec = torch.stack([r[0] for r in res]).reshape(lead + (M,)) if B else a.new_zeros(lead + (M,))
        its = torch.tensor([r[1] for r in res], dtype=torch.int32).reshape(lead)
        return (vec, its) if return_iterations else vec
    lib.ensure_init()
    dev = a.device
    out = torch.zeros(max(B * M, 1), device=dev)
    its, st = _i32(dev, max(B, 1), 0), _i32(dev, max(B, 1), 0)
    wsb = _raw.dr_sc_leading_eigenvector_workspace_bytes(B, B * M)
    ws = _ws(wsb, dev)
    off = _regular_offsets(B, M, dev)
    if points:
        s, t = _f32(a).reshape(-1, 3), _f32(_sc_batched(tgt_points)[1]).reshape(-1, 3)
        check(_raw.dr_sc_leading_eigenvector_f32(B, B * M, ptr(s), ptr(t), ptr(off), None, float(sigma), None, None, int(num_iterations), ptr(out),
                                                 ptr(its), ptr(st), ptr(ws), wsb, stream_of(s)))
    else:
        m = _f32(a)
        mo = torch.arange(B + 1, device=dev, dtype=torch.int64) * (M * M)
        check(_raw.dr_sc_leading_eigenvector_f32(B, B * M, None, None, ptr(off), None, 1.0, ptr(m), ptr(mo), int(num_iterations), ptr(out),
                                                 ptr(its), ptr(st), ptr(ws), wsb, stream_of(m)))
    vec = out[:B * M].reshape(lead + (M,))
    return (vec, its[:B].reshape(lead)) if return_iterations else vec


__all__ = ["weighted_procrustes", "weighted_procrustes_groups", "WeightedProcrustes", "LocalGlobalRegistration",
           "local_to_global_registration_pairs", "spatial_consistency", "cross_spatial_consistency", "spatial_consistency_counts",
           "SpatialConsistencyFiltering", "leading_eigenvector"]
