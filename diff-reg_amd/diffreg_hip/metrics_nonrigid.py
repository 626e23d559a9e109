"""The evaluation of the non-rigid (4DMatch) path on the HIP kernels (csrc/knn_points.hip, nineteenth set after ABI 0.7.0).

Same names and arguments as the reference's (Diff-Reg-2d3d/vision3d/ops):

    knn, knn_pack_mode                                   ops/knn.py:30-145
    knn_interpolate                                      ops/knn_interpolate.py:10-40
    compute_nonrigid_inlier_ratio, compute_nonrigid_feature_matching_recall, compute_scene_flow_accuracy,
    compute_scene_flow_outlier_ratio, compute_corr_coverage, compute_chamfer_distance            ops/metrics.py:258-372

so that a caller swaps the import.  Everything runs on the device through libdiffreg_hip.so (dr_knn_points_f32,
dr_nn_stats_f32, dr_flow_metrics_f32); there is no CPU path and no N x M matrix in memory.  Every metric is a 0-d float64 device tensor (the
kernels count and sum in double; the reference's are float32 means of the same terms) and nothing is read back.  Points are [*, 3] float32.

The search's rule (include/diffreg_hip.h): neighbours ascend by (d2, support index) with d2 = (dx dx + dy dy) + dz dz in float32; KeOps' own tie
order is not claimed.  Slots that cannot be filled hold +inf / -1 in knn_points; knn, as the reference, returns min(k, S) columns."""
import ctypes

import numpy as np
import torch

from . import lib
from .lib import check, ptr, stream_of

_raw = lib.raw()
ST_OFFSETS, ST_NONFINITE = 4, 8


def max_k():
    return int(_raw.dr_knn_points_max_k())


def _pts(name, t):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError("%s must be a float32 tensor (got %s)" % (name, getattr(t, "dtype", type(t))))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s must be [n, 3] (got %s)" % (name, tuple(t.shape)))
    if not t.is_cuda:
        raise TypeError("%s must be on the GPU (got %s); there is no CPU path" % (name, t.device))
    return t.contiguous()


def _lens(lengths, total):
    if lengths is None:
        return [int(total)]
    if torch.is_tensor(lengths):
        lengths = lengths.tolist()           # a device tensor is read back here; pass host lengths to avoid it
    lens = [int(n) for n in lengths]
    if sum(lens) != total or min(lens, default=0) < 0:
        raise ValueError("lengths %s do not add up to %d rows" % (lens, total))
    return lens


def _off(lens, dev):
    """host lengths -> (int32 device offsets [P + 1], the host mirror handed to the entry's host check, keep-alive)"""
    h = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=h[1:])
    return torch.from_numpy(h).to(dev), h.ctypes.data_as(ctypes.c_void_p), h


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


# ------------------------------------------------------------------------------------------------ the three entries
def knn_points(q_points, s_points, k, q_lengths=None, s_lengths=None, return_distance=True, return_indices=True):
    """dr_knn_points_f32 for P pairs: q_points [nq, 3] / s_points [ns, 3] stacked, *_lengths host lists (None: one pair).
    -> (distances [nq, k] float32 or None, indices [nq, k] int64 pair-local or None, status [P] int32); +inf / -1 where a slot has no support."""
    q, s = _pts("q_points", q_points), _pts("s_points", s_points)
    k = int(k)
    if not 1 <= k <= max_k():
        raise ValueError("k must be in 1 .. %d (got %s)" % (max_k(), k))
    ql, sl = _lens(q_lengths, q.shape[0]), _lens(s_lengths, s.shape[0])
    if len(ql) != len(sl):
        raise ValueError("q_lengths and s_lengths must describe the same pairs")
    lib.ensure_init()
    dev, P, nq, ns = q.device, len(ql), q.shape[0], s.shape[0]
    qo, hq, _kq = _off(ql, dev)
    so, hs, _ks = _off(sl, dev)
    dist = torch.full((nq, k), float("inf"), device=dev) if return_distance else None      # a pair the device skips keeps +inf / -1
    idx = torch.full((nq, k), -1, dtype=torch.int64, device=dev) if return_indices else None
    status = torch.zeros(P, dtype=torch.int32, device=dev)
    check(_raw.dr_knn_points_f32(P, nq, ptr(q) if nq else None, ptr(qo), ns, ptr(s) if ns else None, ptr(so), hq, hs, k,
                                 ptr(dist) if (nq and return_distance) else None, ptr(idx) if (nq and return_indices) else None, ptr(status),
                                 stream_of(q)))
    return dist, idx, status


def nn_stats(q_points, s_points, distance_limit=float("inf"), q_lengths=None, s_lengths=None, out=None):
    """dr_nn_stats_f32 -> (stats [P, 4] float64 = queries with a nearest support, sum dist, sum dist^2, count(dist < distance_limit); status [P]).
    out: (stats, status, workspace) of an earlier call of the same shapes, so that a captured graph allocates nothing."""
    q, s = _pts("q_points", q_points), _pts("s_points", s_points)
    ql, sl = _lens(q_lengths, q.shape[0]), _lens(s_lengths, s.shape[0])
    if len(ql) != len(sl):
        raise ValueError("q_lengths and s_lengths must describe the same pairs")
    lib.ensure_init()
    dev, P, nq, ns = q.device, len(ql), q.shape[0], s.shape[0]
    qo, hq, _kq = _off(ql, dev)
    so, hs, _ks = _off(sl, dev)
    wsb = _raw.dr_nn_stats_workspace_bytes(P, nq)
    if out is None:
        out = (torch.zeros(P, 4, dtype=torch.float64, device=dev), torch.zeros(P, dtype=torch.int32, device=dev), _ws(wsb, dev))
    stats, status, ws = out
    check(_raw.dr_nn_stats_f32(P, nq, ptr(q) if nq else None, ptr(qo), ns, ptr(s) if ns else None, ptr(so), hq, hs, float(distance_limit),
                               ptr(stats), ptr(status), ptr(ws), wsb, stream_of(q)))
    return stats, status


def _thr(pair):
    a, r = pair
    return (-1.0 if a is None else float(a)), (-1.0 if r is None else float(r))


def flow_metrics(pred, target, lengths=None, mask=None, rot=None, trn=None, strict=(float("inf"), float("inf")),
                 relaxed=(float("inf"), float("inf")), outlier=(None, None), eps=1e-20):
    """dr_flow_metrics_f32 -> (out [P, 6] float64 = n, sum |e|, n_strict, n_relaxed, n_outlier, n_within(|e| < strict[0]); status [P]).
    rot [P, 3, 3] / trn [P, 3]: pred is first replaced by R pred + t of its pair.  mask: bool / uint8 [n].  A None in `outlier` is the reference's."""
    a, b = _pts("pred", pred), _pts("target", target)
    if a.shape != b.shape:
        raise ValueError("pred and target must have the same shape")
    ln = _lens(lengths, a.shape[0])
    lib.ensure_init()
    dev, P, n = a.device, len(ln), a.shape[0]
    off, ho, _k = _off(ln, dev)
    m = None if mask is None else lib.mask_u8(mask)
    if m is not None and m.shape != (n,):
        raise ValueError("mask must be [n]")
    if (rot is None) != (trn is None):
        raise ValueError("rot and trn go together")
    if rot is not None:
        rot, trn = rot.to(torch.float32).reshape(P, 9).contiguous(), trn.to(torch.float32).reshape(P, 3).contiguous()
    if strict[0] is None or strict[1] is None or relaxed[0] is None or relaxed[1] is None:
        raise ValueError("the accuracy thresholds are required (only the outlier ratio takes None)")
    wsb = _raw.dr_flow_metrics_workspace_bytes(P, n)
    ws = _ws(wsb, dev)
    out = torch.zeros(P, 6, dtype=torch.float64, device=dev)
    status = torch.zeros(P, dtype=torch.int32, device=dev)
    check(_raw.dr_flow_metrics_f32(P, n, ptr(a) if n else None, ptr(b) if n else None, ptr(off), ho, ptr(m) if (m is not None and n) else None,
                                   ptr(rot), ptr(trn), float(strict[0]), float(strict[1]), float(relaxed[0]), float(relaxed[1]), *_thr(outlier),
                                   float(eps), ptr(out), ptr(status), ptr(ws), wsb, stream_of(a)))
    return out, status


# ------------------------------------------------------------------------------------------------ vision3d.ops.knn
def _needed(k, dilation, remove_nearest, num_s):
    dilated_k = (int(k) - 1) * int(dilation) + 1 + (1 if remove_nearest else 0)
    final_k = min(dilated_k, int(num_s))
    if final_k > max_k():
        raise ValueError("the search holds %d neighbours; (k - 1) * dilation + 1%s = %d" % (max_k(), " + 1" if remove_nearest else "", dilated_k))
    return final_k


def knn(q_points, s_points, k, dilation=1, distance_limit=None, return_distance=False, remove_nearest=False, transposed=False,
        padding_mode="nearest", padding_value=1e10, squeeze=False):
    """ops/knn.py:30-107.  Leading dimensions are pairs of one ragged call."""
    if transposed:
        q_points, s_points = q_points.transpose(-1, -2), s_points.transpose(-1, -2)
    if q_points.shape[:-2] != s_points.shape[:-2]:
        raise ValueError("q_points and s_points must share their leading dimensions")
    lead, N, M = tuple(q_points.shape[:-2]), q_points.shape[-2], s_points.shape[-2]
    B = int(np.prod(lead)) if lead else 1
    final_k = _needed(k, dilation, remove_nearest, M)
    q, s = q_points.reshape(B * N, -1), s_points.reshape(B * M, -1)
    if final_k == 0:
        _pts("q_points", q), _pts("s_points", s)
        dist, idx = q.new_zeros(B * N, 0), torch.zeros(B * N, 0, dtype=torch.int64, device=q.device)
    else:
        dist, idx, _ = knn_points(q, s, final_k, [N] * B, [M] * B)
    dist, idx = dist.reshape(lead + (N, final_k)), idx.reshape(lead + (N, final_k))
    if remove_nearest:
        dist, idx = dist[..., 1:], idx[..., 1:]
    if dilation > 1:
        dist, idx = dist[..., ::dilation], idx[..., ::dilation]
    dist, idx = dist.contiguous(), idx.contiguous()
    if distance_limit is not None:
        if padding_mode not in ("nearest", "empty"):
            raise ValueError("padding_mode must be 'nearest' or 'empty'")
        far = torch.ge(dist, distance_limit)
        if padding_mode == "nearest":
            dist, idx = torch.where(far, dist[..., :1], dist), torch.where(far, idx[..., :1], idx)
        else:
            dist = torch.where(far, torch.full_like(dist, padding_value), dist)
            idx = torch.where(far, torch.full_like(idx, M), idx)
    if squeeze and k == 1:
        dist, idx = dist.squeeze(-1), idx.squeeze(-1)
    return (dist, idx) if return_distance else idx


def knn_pack_mode(q_points, s_points, q_lengths, s_lengths, k, return_distance=False, inf=1e10):
    """ops/knn.py:110-145: the ragged call itself (indices are local to each cloud, as the reference's batch indices are).  The lengths are
    wanted on the host; a device tensor is read back."""
    sl = _lens(s_lengths, s_points.shape[0])
    if min(sl, default=k) < k:
        raise ValueError("The number of support points less than %d." % k)
    dist, idx, _ = knn_points(q_points, s_points, k, _lens(q_lengths, q_points.shape[0]), sl, return_distance=return_distance)
    return (dist, idx) if return_distance else idx


def _blend(dist, idx, s_feats, s_first, eps, distance_limit):
    """ops/knn_interpolate.py:33-39 on the search's outputs; idx pair-local, s_first [n, 1] the first support row of each query's pair.  A slot
    without a support (-1, +inf) weighs 0."""
    if distance_limit is not None:
        dist = dist.masked_fill(torch.gt(dist, distance_limit), 1e10)
    weights = 1.0 / (dist + eps)
    weights = weights / weights.sum(dim=1, keepdim=True)
    feats = s_feats[(idx.clamp_min(0) + s_first).reshape(-1)].reshape(idx.shape + (s_feats.shape[-1],))
    return (feats * weights.unsqueeze(-1)).sum(dim=1)


def knn_interpolate(q_points, s_points, s_feats, k=3, eps=1e-10, distance_limit=None, q_lengths=None, s_lengths=None):
    """ops/knn_interpolate.py:10-40; with *_lengths, for P pairs in one call."""
    ql, sl = _lens(q_lengths, q_points.shape[0]), _lens(s_lengths, s_points.shape[0])
    kk = min(int(k), max(sl, default=0)) if len(sl) == 1 else int(k)
    if kk == 0:
        return s_feats.new_zeros(q_points.shape[0], s_feats.shape[-1]) * float("nan")
    dist, idx, _ = knn_points(q_points, s_points, kk, ql, sl)
    first = torch.repeat_interleave(torch.tensor(np.concatenate([[0], np.cumsum(sl)[:-1]]), dtype=torch.int64, device=idx.device),
                                    torch.tensor(ql, dtype=torch.int64, device=idx.device), output_size=q_points.shape[0])[:, None]
    return _blend(dist, idx, s_feats, first, eps, distance_limit)


# ------------------------------------------------------------------------------------------------ vision3d.ops.metrics, :258-372
def _rt(transform, P=1):
    if transform is None:
        return None, None
    T = transform.to(torch.float32).reshape(P, 4, 4)
    return T[:, :3, :3].contiguous(), T[:, :3, 3].contiguous()


def compute_nonrigid_inlier_ratio(src_corr_points, tgt_corr_points, corr_scene_flows, transform=None, acceptance_radius=0.04):
    rot, trn = _rt(transform)
    o, _ = flow_metrics(src_corr_points + corr_scene_flows, tgt_corr_points, rot=rot, trn=trn, strict=(acceptance_radius, -1.0))
    return (o[0, 5] / o[0, 0]).nan_to_num_()


def compute_nonrigid_feature_matching_recall(src_corr_points, tgt_corr_points, src_points, scene_flows, test_indices, transform=None,
                                             acceptance_radius=0.04, distance_limit=0.1):
    corr_motions = tgt_corr_points - src_corr_points
    src_test = src_points[test_indices]
    if src_corr_points.shape[0] == 0 or src_test.shape[0] == 0:
        return torch.zeros((), dtype=torch.float64, device=src_points.device)
    pred = src_test + knn_interpolate(src_test, src_corr_points, corr_motions, k=3, distance_limit=distance_limit)
    rot, trn = _rt(transform)
    o, _ = flow_metrics(src_test + scene_flows[test_indices], pred, rot=rot, trn=trn, strict=(acceptance_radius, -1.0))
    return (o[0, 5] / o[0, 0]).nan_to_num_()


def compute_scene_flow_accuracy(inputs, targets, acceptance_absolute_error, acceptance_relative_error, eps=1e-20):
    o, _ = flow_metrics(inputs, targets, strict=(acceptance_absolute_error, acceptance_relative_error), eps=eps)
    return o[0, 2] / o[0, 0]


def compute_scene_flow_outlier_ratio(inputs, targets, acceptance_absolute_error, acceptance_relative_error, eps=1e-20):
    o, _ = flow_metrics(inputs, targets, outlier=(acceptance_absolute_error, acceptance_relative_error), eps=eps)
    return o[0, 4] / o[0, 0]


def compute_corr_coverage(q_points, s_points, distance_limit):
    st, _ = nn_stats(q_points, s_points, distance_limit)
    return (st[0, 3] / q_points.shape[0]).nan_to_num_() if q_points.shape[0] else torch.zeros((), dtype=torch.float64, device=q_points.device)


def compute_chamfer_distance(q_points, s_points, squared=False):
    a, _ = nn_stats(q_points, s_points)
    b, _ = nn_stats(s_points, q_points)
    c = 2 if squared else 1
    return a[0, c] / a[0, 0] + b[0, c] / b[0, 0]


# ------------------------------------------------------------------------------------------------ the pairs of a batch at once
# the fixed layout of evaluate_nonrigid_pairs' vector: per-pair terms summed over pairs and, by one all_reduce, over ranks.  The first five slots
# are shard.METRIC_NAMES (NIR in the inlier-ratio slot, NFMR in the FMR slot, 0 in the recall slot), so shard.reduce_metrics keeps working
VECTOR_NAMES = ("sum_inlier_ratio", "sum_fmr", "sum_registration_recall", "n_pairs", "sum_seconds", "sum_EPE", "sum_AccS", "sum_AccR",
                "sum_outlier", "sum_chamfer", "sum_coverage")


def reduce_pair_metrics(local_vec):
    """all_reduce(SUM) of this rank's summed evaluate_nonrigid_pairs vectors (shard.gather_metrics) -> dict with every sum under its VECTOR_NAMES
    name and the means over ALL pairs: NIR, NFMR, EPE, AccS, AccR, outlier, chamfer, coverage."""
    from . import shard
    g = shard.gather_metrics(local_vec, local_vec.device if torch.is_tensor(local_vec) else None).tolist()
    d = dict(zip(VECTOR_NAMES, g))
    n = max(d["n_pairs"], 1.0)
    d.update({"NIR": d["sum_inlier_ratio"] / n, "NFMR": d["sum_fmr"] / n})
    d.update({k: d["sum_" + k] / n for k in ("EPE", "AccS", "AccR", "outlier", "chamfer", "coverage")})
    return d


def _stack(x, lengths):
    """a list of per-pair tensors, or a stacked tensor with host lengths -> (stacked, lengths)"""
    if isinstance(x, (list, tuple)):
        return torch.cat(list(x)), [int(t.shape[0]) for t in x]
    return x, _lens(lengths, x.shape[0])


def evaluate_nonrigid_pairs(src_points, warped_src, scene_flows, tgt_points, gt_transform=None, matches=None, test_indices=None, *, strict,
                            relaxed, outlier, acceptance_radius=0.04, distance_limit=0.1, chamfer=True, coverage_limit=None, src_lengths=None,
                            tgt_lengths=None):
    """P pairs in ragged calls, nothing read back.  Lists of per-pair tensors, or stacked tensors with src_lengths / tgt_lengths (host lists).
    The predicted flow is warped_src - src_points, the target apply_transform(src + scene_flows, gt_transform) - src_points (gt_transform
    [P, 4, 4] or a list; None: identity), so warped_src lives in the target's frame.  strict / relaxed / outlier: the (absolute, relative)
    thresholds of compute_scene_flow_accuracy (twice) and compute_scene_flow_outlier_ratio -- the reference gives no defaults.
    matches: per pair int64 [m, 2] (source row, target row): NIR over them, and with test_indices (per pair int64 rows of the source cloud) NFMR;
    with coverage_limit the share of source points within it of a matched source point (compute_corr_coverage).  chamfer: compute_chamfer_distance
    of warped_src and tgt_points.
    -> dict of per-pair float64 device tensors [P] (EPE, AccS, AccR, outlier, NIR, NFMR, chamfer, coverage; 0 where not asked for) and "vector",
    float64 [len(VECTOR_NAMES)], the sums over the pairs."""
    src, pl = _stack(src_points, src_lengths)
    warped, _ = _stack(warped_src, pl)
    flows, _ = _stack(scene_flows, pl)
    tgt, tl = _stack(tgt_points, tgt_lengths)
    src, warped, flows, tgt = _pts("src_points", src), _pts("warped_src", warped), _pts("scene_flows", flows), _pts("tgt_points", tgt)
    P, dev = len(pl), src.device
    if len(tl) != P or warped.shape != src.shape or flows.shape != src.shape:
        raise ValueError("one source cloud, warped cloud, flow and target cloud per pair")
    rot = trn = None
    if gt_transform is not None:
        T = torch.stack(list(gt_transform)) if isinstance(gt_transform, (list, tuple)) else gt_transform
        rot, trn = _rt(T.to(dev), P)
    zeros = torch.zeros(P, dtype=torch.float64, device=dev)
    first = lambda lens: np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    rep = lambda vals, lens: torch.repeat_interleave(torch.as_tensor(vals, device=dev), torch.as_tensor(lens, device=dev), output_size=int(sum(lens)))
    moved = src + flows
    if rot is not None:
        R = rep(torch.arange(P), pl)
        moved = torch.bmm(rot[R], moved[:, :, None])[:, :, 0] + trn[R]
    fm, _ = flow_metrics(warped - src, moved - src, lengths=pl, strict=strict, relaxed=relaxed, outlier=outlier)
    n = fm[:, 0]
    out = {"EPE": fm[:, 1] / n, "AccS": fm[:, 2] / n, "AccR": fm[:, 3] / n, "outlier": fm[:, 4] / n, "NIR": zeros, "NFMR": zeros, "chamfer": zeros,
           "coverage": zeros}
    if matches is not None:
        mat = list(matches)
        if len(mat) != P:
            raise ValueError("one match list per pair")
        ml = [int(m.shape[0]) for m in mat]
        srow = torch.cat([m[:, 0] for m in mat]) + rep(first(pl), ml)
        trow = torch.cat([m[:, 1] for m in mat]) + rep(first(tl), ml)
        src_c, tgt_c = src[srow], tgt[trow]
        o, _ = flow_metrics(src_c + flows[srow], tgt_c, lengths=ml, rot=rot, trn=trn, strict=(acceptance_radius, -1.0))
        out["NIR"] = (o[:, 5] / o[:, 0]).nan_to_num_()
        if test_indices is not None:
            tst = list(test_indices)
            tlens = [int(t.shape[0]) for t in tst]
            rows = torch.cat(tst) + rep(first(pl), tlens)
            src_t = src[rows]
            dist, idx, _ = knn_points(src_t, src_c, 3, tlens, ml)
            pred = src_t + _blend(dist, idx, tgt_c - src_c, rep(first(ml), tlens)[:, None], 1e-10, distance_limit)
            o, _ = flow_metrics(src_t + flows[rows], pred, lengths=tlens, rot=rot, trn=trn, strict=(acceptance_radius, -1.0))
            out["NFMR"] = (o[:, 5] / o[:, 0]).nan_to_num_()
        if coverage_limit is not None:
            st, _ = nn_stats(src, src_c, coverage_limit, pl, ml)
            out["coverage"] = (st[:, 3] / torch.as_tensor(pl, dtype=torch.float64, device=dev)).nan_to_num_()
    if chamfer:
        a, _ = nn_stats(warped, tgt, q_lengths=pl, s_lengths=tl)
        b, _ = nn_stats(tgt, warped, q_lengths=tl, s_lengths=pl)
        out["chamfer"] = a[:, 1] / a[:, 0] + b[:, 1] / b[:, 0]
    s = lambda k: out[k].sum()
    z = torch.zeros((), dtype=torch.float64, device=dev)
    out["vector"] = torch.stack([s("NIR"), s("NFMR"), z, z + P, z, s("EPE"), s("AccS"), s("AccR"), s("outlier"), s("chamfer"), s("coverage")])
    return out
