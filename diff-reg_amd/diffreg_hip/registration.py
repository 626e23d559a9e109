"""vision3d's RANSAC-free rigid estimators on the device (twentieth set after ABI 0.7.0; csrc/lgr.hip, rules in include/diffreg_hip.h):

    weighted_procrustes, WeightedProcrustes                vision3d/ops/weighted_procrustes.py, vision3d/layers/weighted_procrustes.py
    LocalGlobalRegistration                                vision3d/models/geotransformer/local_global_registration.py
    local_to_global_registration_pairs                     the same for P pairs in one call (ragged)
    spatial_consistency, cross_spatial_consistency         vision3d/ops/spatial_consistency.py
    spatial_consistency_counts, SpatialConsistencyFiltering  vision3d/models/geotransformer/spatial_consistency_filtering.py
    leading_eigenvector                                    vision3d/ops/eigenvector.py
    multi_scale_icp, icp, icp_pairs, voxel_down_sample,    vision3d/utils/open3d.py:378-396 (twenty-first set; csrc/icp.hip): the published
    IterativeClosestPoint                                  loop of Open3D's point-to-point registration_icp, stated in the header

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


# ---------------------------------------------------------------------------------------------- point-to-point ICP (twenty-first set)
# vision3d/utils/open3d.py:378-396 (multi_scale_icp) runs Open3D's registration_icp per scale.  Open3D is not part of this project's
# environment: the loop is STATED in include/diffreg_hip.h (dr_icp_p2p_f32) and both paths below are held to that statement; parity with
# Open3D itself is not claimed.
ICP_RANK_TOL = 1e-12


def _cpu_icp_evaluate(T, src, tgt, r2):
    """the float32 Evaluate(T) of the rule on CPU tensors -> (moved (n, 3), partner (n,) int64 or -1, d2 (n,))"""
    a = [((T[i, 0] * src[:, 0] + T[i, 1] * src[:, 1]) + T[i, 2] * src[:, 2]) + T[i, 3] for i in range(3)]
    moved = torch.stack(a, 1)
    n = src.shape[0]
    partner, best = torch.full((n,), -1, dtype=torch.int64), torch.zeros(n)
    if n == 0 or tgt.shape[0] == 0:
        return moved, partner, best
    for lo in range(0, n, 2048):
        m = moved[lo:lo + 2048]
        dx, dy, dz = m[:, None, 0] - tgt[None, :, 0], m[:, None, 1] - tgt[None, :, 1], m[:, None, 2] - tgt[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2 = torch.where(d2 < r2, d2, torch.full_like(d2, float("inf")))
        v = d2.min(1).values
        j = (d2 == v[:, None]).to(torch.uint8).argmax(1)          # the lowest index among equal distances
        ok = torch.isfinite(v)
        partner[lo:lo + 2048] = torch.where(ok, j, torch.full_like(j, -1))
        best[lo:lo + 2048] = torch.where(ok, v, torch.zeros_like(v))
    return moved, partner, best


def _cpu_icp_update(p, q):
    """rule 1 with unit weights and eps = 0 in double -> (4 x 4 double update, status bits)"""
    p, q = p.double(), q.double()
    pc, qc = p.mean(0), q.mean(0)
    H = (p - pc).T @ (q - qc) / p.shape[0]
    U4, flags = torch.eye(4, dtype=torch.float64), 0
    if bool(H.abs().sum() == 0):
        flags = 16
    else:
        U, S, Vh = torch.linalg.svd(H)
        if float(S[1]) <= ICP_RANK_TOL * float(S[0]):
            flags = 16
        V = Vh.T
        D = torch.diag(torch.tensor([1.0, 1.0, float(torch.sign(torch.det(V @ U.T)))], dtype=torch.float64))
        U4[:3, :3] = V @ D @ U.T
    U4[:3, 3] = qc - U4[:3, :3] @ pc
    return U4, flags


def _cpu_icp(src, tgt, init, r, max_iteration, rel_fitness, rel_rmse):
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    T = torch.eye(4) if init is None else init.float().clone()
    T[3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    r2 = f32(r) * f32(r)

    def evaluate():
        moved, partner, d2 = _cpu_icp_evaluate(T, src, tgt, r2)
        n = int((partner >= 0).sum())
        fit = f32(n / src.shape[0]) if src.shape[0] else f32(0.0)
        rmse = f32(float(torch.sqrt(d2.double().sum() / n))) if n else f32(0.0)
        return moved, partner, n, fit, rmse
    moved, partner, n, fit, rmse = evaluate()
    its, status = 0, 0
    while True:
        if n == 0:
            status |= 32
            break
        if its >= max_iteration:
            break
        keep = partner >= 0
        U4, flags = _cpu_icp_update(moved[keep], tgt[partner[keep]])
        status |= flags
        T = (U4 @ T.double()).float()
        T[3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
        its += 1
        last_fit, last_rmse = fit, rmse
        moved, partner, n, fit, rmse = evaluate()
        if bool((last_fit - fit).abs() < f32(rel_fitness)) and bool((last_rmse - rmse).abs() < f32(rel_rmse)):
            if n == 0:
                status |= 32
            break
    return T, fit, rmse, its, status, partner


def icp_pairs(src_points, tgt_points, s_offsets, t_offsets, init_transforms=None, distance_threshold=0.05, max_iteration=30,
              relative_fitness=1e-6, relative_rmse=1e-6, return_correspondence=False, host_s_offsets=None, host_t_offsets=None):
    """Point-to-point ICP (the loop of Open3D's registration_icp with TransformationEstimationPointToPoint(False), as stated for
    dr_icp_p2p_f32) for P pairs in one call: src_points (ns, 3), tgt_points (nt, 3) stacked, s_offsets / t_offsets (P + 1,) int32 on the
    device, init_transforms (P, 4, 4) or None (identity).  -> dict(transforms (P, 4, 4), fitness (P,), inlier_rmse (P,), iterations (P,)
    int32, status (P,) int32; with return_correspondence also correspondence (ns,) int32: the pair-local partner of every source row or -1).
    Nothing is read back.  A pair with status bit 4 or 8 is skipped: its rows keep what this wrapper put there (the initial transform, zeros,
    -1).  Bit 16: a fit met a rank-deficient H; bit 32: an evaluation found no correspondence."""
    src, tgt = _f32(src_points), _f32(tgt_points)
    so, to = s_offsets.to(torch.int32).contiguous(), t_offsets.to(torch.int32).contiguous()
    P, ns, nt, dev = so.numel() - 1, src.shape[0], tgt.shape[0], src.device
    init = None if init_transforms is None else _f32(init_transforms).reshape(P, 16)
    if not src.is_cuda:
        a, b = so.tolist(), to.tolist()
        res = [_cpu_icp(src[a[p]:a[p + 1]], tgt[b[p]:b[p + 1]], None if init is None else init[p].view(4, 4), distance_threshold,
                        max_iteration, relative_fitness, relative_rmse) for p in range(P)]
        out = dict(transforms=torch.stack([r[0] for r in res]) if P else torch.zeros(0, 4, 4),
                   fitness=torch.tensor([float(r[1]) for r in res]), inlier_rmse=torch.tensor([float(r[2]) for r in res]),
                   iterations=torch.tensor([r[3] for r in res], dtype=torch.int32), status=torch.tensor([r[4] for r in res], dtype=torch.int32))
        if return_correspondence:
            out["correspondence"] = torch.cat([r[5] for r in res]).to(torch.int32) if P else torch.zeros(0, dtype=torch.int32)
        return out
    lib.ensure_init()
    n = max(P, 1)
    T = torch.eye(4, device=dev).reshape(1, 16).repeat(n, 1) if init is None else init.clone()
    fit, rmse = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    its, st = _i32(dev, n, 0), _i32(dev, n, 0)
    corr = _i32(dev, max(ns, 1), -1) if return_correspondence else None
    wsb = _raw.dr_icp_p2p_workspace_bytes(P, ns, nt)
    ws = _ws(wsb, dev)
    hp = lambda h: None if h is None else h.ctypes.data
    check(_raw.dr_icp_p2p_f32(P, ns, ptr(src), ptr(so), nt, ptr(tgt), ptr(to), hp(host_s_offsets), hp(host_t_offsets), ptr(init),
                              float(distance_threshold), int(max_iteration), float(relative_fitness), float(relative_rmse), ptr(T), ptr(fit),
                              ptr(rmse), ptr(its), ptr(corr), ptr(st), ptr(ws), wsb, stream_of(src)))
    out = dict(transforms=T[:P].view(P, 4, 4), fitness=fit[:P], inlier_rmse=rmse[:P], iterations=its[:P], status=st[:P])
    if return_correspondence:
        out["correspondence"] = corr[:ns]
    return out


def icp(src_points, tgt_points, init_transform=None, distance_threshold=0.05, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6,
        return_correspondence=False):
    """icp_pairs for one pair: (N, 3), (M, 3), init_transform (4, 4) or None -> dict(transform (4, 4), fitness, inlier_rmse, iterations,
    status: 0-d tensors[, correspondence (N,)])"""
    dev = src_points.device
    so = torch.tensor([0, src_points.shape[0]], dtype=torch.int32, device=dev)
    to = torch.tensor([0, tgt_points.shape[0]], dtype=torch.int32, device=dev)
    r = icp_pairs(src_points, tgt_points, so, to, None if init_transform is None else init_transform[None], distance_threshold, max_iteration,
                  relative_fitness, relative_rmse, return_correspondence)
    out = dict(transform=r["transforms"][0], fitness=r["fitness"][0], inlier_rmse=r["inlier_rmse"][0], iterations=r["iterations"][0],
               status=r["status"][0])
    if return_correspondence:
        out["correspondence"] = r["correspondence"]
    return out


def _cpu_voxel_down_sample(points, voxel_size):
    p = points.float()
    if p.shape[0] == 0:
        return p
    v = torch.tensor(voxel_size, dtype=torch.float32)
    origin = p.min(0).values - torch.tensor(0.5, dtype=torch.float32) * v
    idx = torch.floor((p - origin) / v).to(torch.int64)
    key = (idx[:, 2] << 42) | (idx[:, 1] << 21) | idx[:, 0]
    uniq, inv = torch.unique(key, return_inverse=True)                   # ascending (iz, iy, ix)
    out = torch.zeros(uniq.shape[0], 3)
    cnt = torch.zeros(uniq.shape[0], dtype=torch.int64)
    for i in range(p.shape[0]):                                          # the float32 sum in input order
        out[inv[i]] = out[inv[i]] + p[i]
        cnt[inv[i]] += 1
    return out * (1.0 / cnt.double()).float()[:, None]


def voxel_down_sample(points, voxel_size, lengths=None, return_status=False):
    """Open3D's PointCloud.voxel_down_sample (the barycentre of every voxel of the grid that starts at min - 0.5 * voxel_size), on
    dr_grid_subsample_open3d_f32.  The rows come in this library's voxel-key order (ascending (iz, iy, ix)); Open3D's order is a hash map's
    and unspecified.  lengths None: points (N, 3) is one cloud -> (M, 3); ONE word is read back, the number of voxels, to size the result.
    lengths (nb,) int32: stacked clouds -> (buffer (N, 3), out_lengths (nb,) int32) with nothing read back; the rows of the buffer behind
    out_lengths.sum() are unspecified.  return_status appends the grid subsample's status word, a (1,) int32 tensor on the points' device
    that is not read here: non-zero when a cloud spans more voxels per axis than the 16 key bits hold (the output is then unspecified)."""
    pts = _f32(points)
    if not pts.is_cuda:
        ok = torch.zeros(1, dtype=torch.int32)
        if lengths is None:
            out = _cpu_voxel_down_sample(pts, voxel_size)
            return (out, ok) if return_status else out
        cut = [0] + torch.cumsum(lengths.to(torch.int64), 0).tolist()
        parts = [_cpu_voxel_down_sample(pts[a:b], voxel_size) for a, b in zip(cut[:-1], cut[1:])]
        buf = torch.zeros(max(pts.shape[0], 1), 3)
        got = torch.cat(parts) if parts else pts[:0]
        buf[:got.shape[0]] = got
        ol = torch.tensor([q.shape[0] for q in parts], dtype=torch.int32)
        return (buf, ol, ok) if return_status else (buf, ol)
    lib.ensure_init()
    one = lengths is None
    ln = torch.tensor([pts.shape[0]], dtype=torch.int32, device=pts.device) if one else lengths
    out, ol, tot, st = lib.grid_subsample(pts, ln, voxel_size, open3d=True)
    if one:
        out = out[:int(tot.item())]                                      # the one word read back
        return (out, st) if return_status else out
    return (out, ol, st) if return_status else (out, ol)


def _offsets_of(lengths):
    z = torch.zeros(1, dtype=torch.int64, device=lengths.device)
    return torch.cat([z, torch.cumsum(lengths.to(torch.int64), 0)]).to(torch.int32)


def multi_scale_icp(src_points, tgt_points, init_transform, multi_scale_icp_cfgs, distance_threshold, src_lengths=None, tgt_lengths=None,
                    relative_fitness=1e-6, relative_rmse=1e-6, return_status=False):
    """vision3d.utils.open3d.multi_scale_icp: for each cfg (a dict with "max_iteration" and "voxel_size") both clouds are voxel-down-sampled
    and refined by point-to-point ICP from the previous transform.  One pair: (N, 3), (M, 3), init_transform (4, 4) -> (4, 4).  A batch:
    stacked clouds with src_lengths / tgt_lengths (P,) int32 and init_transform (P, 4, 4) -> (P, 4, 4), ragged in one call per scale.  The
    offsets of every scale come from the device lengths of the down-sample, and the ICP takes the down-sample's buffers at their capacity:
    no host read per scale was needed, and none is made.  A pair that a scale skips (status bit 4 or 8) or finds without correspondence
    (bit 32) goes on with the transform it had; return_status=True returns (transforms, status) with status (P,) int32 -- () for one pair --
    the OR over the scales of icp_pairs' status words, plus bit 1 where a down-sample reported a voxel range beyond its key bits (that
    word is per call, so every pair of the batch gets it).  The status stays on the device."""
    one = src_lengths is None
    dev = src_points.device
    sl = torch.tensor([src_points.shape[0]], dtype=torch.int32, device=dev) if one else src_lengths.to(device=dev, dtype=torch.int32)
    tl = torch.tensor([tgt_points.shape[0]], dtype=torch.int32, device=dev) if one else tgt_lengths.to(device=dev, dtype=torch.int32)
    T = _f32(init_transform)[None] if one else _f32(init_transform)
    status = torch.zeros(T.shape[0], dtype=torch.int32, device=dev)
    for cfg in multi_scale_icp_cfgs:
        s, s_len, s_st = voxel_down_sample(src_points, cfg["voxel_size"], sl, True)
        t, t_len, t_st = voxel_down_sample(tgt_points, cfg["voxel_size"], tl, True)
        r = icp_pairs(s, t, _offsets_of(s_len), _offsets_of(t_len), T, distance_threshold, cfg["max_iteration"], relative_fitness,
                      relative_rmse)
        T = r["transforms"]
        status = status | r["status"] | ((s_st | t_st) != 0).to(torch.int32)
    if return_status:
        return (T[0], status[0]) if one else (T, status)
    return T[0] if one else T


class IterativeClosestPoint(nn.Module):
    """point-to-point ICP with fixed settings; forward(src_points, tgt_points, init_transform=None) is icp(...)"""

    def __init__(self, distance_threshold, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
        super().__init__()
        self.distance_threshold = distance_threshold
        self.max_iteration = max_iteration
        self.relative_fitness = relative_fitness
        self.relative_rmse = relative_rmse

    def forward(self, src_points, tgt_points, init_transform=None):
        return icp(src_points, tgt_points, init_transform, self.distance_threshold, self.max_iteration, self.relative_fitness,
                   self.relative_rmse)

    def extra_repr(self):
        return "distance_threshold=%g, max_iteration=%d, relative_fitness=%g, relative_rmse=%g" % (
            self.distance_threshold, self.max_iteration, self.relative_fitness, self.relative_rmse)


__all__ = ["weighted_procrustes", "weighted_procrustes_groups", "WeightedProcrustes", "LocalGlobalRegistration",
           "local_to_global_registration_pairs", "spatial_consistency", "cross_spatial_consistency", "spatial_consistency_counts",
           "SpatialConsistencyFiltering", "leading_eigenvector", "icp_pairs", "icp", "voxel_down_sample", "multi_scale_icp",
           "IterativeClosestPoint"]
