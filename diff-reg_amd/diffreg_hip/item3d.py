"""The 3D / 4D dataset item on the device: what _3DMatch.__getitem__ (3D/datasets/_3dmatch.py:55-135) and _4DMatch.__getitem__
(3D/datasets/_4dmatch.py:58-146) compute behind their file reads, with the reference's names:

    prepare_item_3dmatch, prepare_item_4dmatch     the body of __getitem__ behind torch.load / np.load -> the reference's positional tuple
    prepare_batch                                  the same for a list of raw items in two library calls -> the pair dicts of collate_fn_device
    get_correspondences                            3D/lib/benchmark_utils.py:166-185

The subsample, the rotation, the jitter, the recomputed scene flow and the composed rot / trans run in dr_item3d_prepare_f32, the pair list in
dr_radius_pairs_ragged_f32 (csrc/item3d.hip); there is no CPU path.  A batch reads ONE word list back, the pair counts of all its pairs.
Differences a maintainer should know: a row's partners come in ascending target index where Open3D returns ascending
distance; np.random's draws cannot be reproduced, so they are replayed from `draws` or drawn by torch from `generator` (a replayed
permutation passed as a numpy array is checked before any launch; one passed as a device tensor is checked by the kernel's status bit); 4DMatch's subsample
indexes src_pcd only, so with max_points below the cloud and no augmentation s2t_flow comes back unselected, and with augmentation the call is
refused where the reference raises."""
import math

import numpy as np
import torch

from . import lib


def euler_zyx_matrix(angles):
    """Rotation.from_euler('zyx', angles).as_matrix() for angles [..., 3] (float64, any device) -> [..., 3, 3]: Rx(c) Ry(b) Rz(a)"""
    a, b, c = angles[..., 0], angles[..., 1], angles[..., 2]
    ca, sa, cb, sb, cc, sc = torch.cos(a), torch.sin(a), torch.cos(b), torch.sin(b), torch.cos(c), torch.sin(c)
    rows = [cb * ca, -cb * sa, sb,
            sc * sb * ca + cc * sa, cc * ca - sc * sb * sa, -sc * cb,
            sc * sa - cc * sb * ca, cc * sb * sa + sc * ca, cc * cb]
    return torch.stack(rows, dim=-1).reshape(angles.shape[:-1] + (3, 3))


_KEYS = {"3dmatch": ("src_pcd", "tgt_pcd"), "4dmatch": ("s_pc", "t_pc")}


def _cloud(a, name, device):
    t = torch.as_tensor(a)
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("item3d: %s must be a float32 [n, 3] cloud (got %s %s)" % (name, t.dtype, tuple(t.shape)))
    return t.to(device).contiguous()


def _selection(perm, n, max_points, generator, device, name):
    """the first max_points entries of a permutation of n as an int64 device vector.  A replayed one given as a numpy array is range-checked on
    the host, before any launch; one given as a device tensor is not read here (that would be a host read per cloud): the kernel writes a row
    whose index is out of range as zero and sets the pair's status bit, which prepare_batch raises on after its one read."""
    if perm is None:
        gen_dev = generator.device if generator is not None else device
        return torch.randperm(n, generator=generator, device=gen_dev)[:max_points].to(device)
    if torch.is_tensor(perm):
        if perm.dtype != torch.int64 or not perm.is_contiguous():
            raise ValueError("item3d: %s must be a contiguous int64 vector" % name)
        sel = perm[:max_points]
        if not sel.is_cuda:
            lo, hi = (int(sel.min()), int(sel.max())) if sel.numel() else (0, 0)
        else:
            lo, hi = 0, 0
    else:
        sel = np.asarray(perm)
        if sel.dtype != np.int64 or sel.ndim != 1 or not sel.flags.c_contiguous:
            raise ValueError("item3d: %s must be a contiguous int64 vector" % name)
        sel = sel[:max_points]
        lo, hi = (int(sel.min()), int(sel.max())) if sel.size else (0, 0)
        sel = torch.from_numpy(sel)
    if sel.shape[0] != min(n, max_points):
        raise ValueError("item3d: %s holds %d entries, %d are needed" % (name, sel.shape[0], min(n, max_points)))
    if lo < 0 or hi >= n:
        raise ValueError("item3d: %s addresses row %d of a cloud of %d" % (name, lo if lo < 0 else hi, n))
    return sel.to(device).contiguous()


def _to_device(a, device):
    return (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(device)


def _offsets(counts, device):
    return torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32).to(device)


def prepare_batch(items, *, kind="3dmatch", max_points=30000, data_augmentation=True, rot_factor=1.0, augment_noise=0.005,
                  overlap_radius=0.0375, generator=None, draws=None, device="cuda"):
    """`items`: raw dataset entries after their file reads -- 3dmatch: dict(src_pcd, tgt_pcd [n, 3] float32, rot [3, 3], trans [3] or [3, 1][,
    gt_cov]); 4dmatch: the .npz entry's keys (s_pc, t_pc, rot, trans, s2t_flow, correspondences[, metric_index]), numpy or torch.
    -> a list of pair dicts for collate_fn_device (3dmatch: `correspondences` [C, 2] int64 built on the device) / collate_fn_device_4dmatch, all
    device tensors, rot [3, 3] / trn [3, 1] float32.  The whole batch is one dr_item3d_prepare_f32 call and, for 3dmatch, two
    dr_radius_pairs_ragged_f32 calls (count, then write into room of exactly the counted size) around the ONE host read.  The second call
    repeats the first one's sort and count sweep: the price of a list of exactly the found size without a second read (a caller who knows a
    bound calls lib.radius_pairs_ragged once with that room).
    draws: None, or one dict per item replaying recorded np.random draws: src_perm / tgt_perm (int64, at least max_points entries), euler [3]
    (the angles), coin, src_jitter / tgt_jitter ([n, 3] in [0, 1)); entries not given are drawn by torch from `generator`."""
    if kind not in _KEYS:
        raise ValueError("item3d: kind is '3dmatch' or '4dmatch'")
    P = len(items)
    draws = [{} for _ in items] if draws is None else [dict(d) for d in draws]
    ks, kt = _KEYS[kind]
    gen_dev = generator.device if generator is not None else device
    f64 = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device=device, dtype=torch.float64)
    src_raw = [_cloud(it[ks], ks, device) for it in items]
    tgt_raw = [_cloud(it[kt], kt, device) for it in items]
    flows = [_cloud(it["s2t_flow"], "s2t_flow", device) for it in items] if kind == "4dmatch" else None
    sel = {"src": [None] * P, "tgt": [None] * P}
    for p in range(P):
        for side, raw in (("src", src_raw), ("tgt", tgt_raw)):
            n = raw[p].shape[0]
            if n > max_points:                                               # _3dmatch.py:71-76
                sel[side][p] = _selection(draws[p].get(side + "_perm"), n, max_points, generator, device, side + "_perm")
        if flows is not None:
            if flows[p].shape != src_raw[p].shape:
                raise ValueError("item3d: s2t_flow has one row per source point")
            if data_augmentation and sel["src"][p] is not None:
                raise ValueError("item3d: pair %d subsamples the source (%d > max_points = %d) with augmentation and a flow: the reference raises "
                                 "there (`src_pcd_deformed - src_pcd`, _4dmatch.py:124, shapes differ)" % (p, src_raw[p].shape[0], max_points))

    def stacked_selection(side, raw):
        if all(s is None for s in sel[side]):
            return None, [r.shape[0] for r in raw]
        parts = [torch.arange(r.shape[0], device=device) if s is None else s for s, r in zip(sel[side], raw)]
        return torch.cat(parts).contiguous(), [x.shape[0] for x in parts]

    s_sel, ns = stacked_selection("src", src_raw)
    t_sel, nt = stacked_selection("tgt", tgt_raw)
    aug = {}
    if data_augmentation:
        draw = lambda *shape: torch.rand(*shape, generator=generator, dtype=torch.float64, device=gen_dev).to(device)
        pick = lambda p, name, make: f64(draws[p][name]) if name in draws[p] else make()
        euler = torch.stack([pick(p, "euler", lambda: draw(3) * (math.pi * 2 / rot_factor)).reshape(3) for p in range(P)])
        aug["rot_ab"] = euler_zyx_matrix(euler)
        aug["coin"] = torch.stack([pick(p, "coin", lambda: draw(1)).reshape(()) for p in range(P)])
        aug["src_jitter"] = torch.cat([pick(p, "src_jitter", lambda: draw(ns[p], 3)) for p in range(P)])
        aug["tgt_jitter"] = torch.cat([pick(p, "tgt_jitter", lambda: draw(nt[p], 3)) for p in range(P)])
        aug["noise"] = augment_noise
    out = lib.item3d_prepare(torch.cat(src_raw), _offsets([r.shape[0] for r in src_raw], device), torch.cat(tgt_raw),
                             _offsets([r.shape[0] for r in tgt_raw], device), torch.stack([f64(it["rot"]).reshape(3, 3) for it in items]),
                             torch.stack([f64(it["trans"]).reshape(3) for it in items]), s_offsets=_offsets(ns, device),
                             t_offsets=_offsets(nt, device), src_sel=s_sel, tgt_sel=t_sel, flow_raw=None if flows is None else torch.cat(flows),
                             recompute_flow=bool(data_augmentation), **aug)
    s_off, t_off = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(nt)])
    r_off = np.concatenate([[0], np.cumsum([r.shape[0] for r in src_raw])])
    corr = None
    if kind == "3dmatch":
        so, to = _offsets(ns, device), _offsets(nt, device)
        _, _, counts, p_status = lib.radius_pairs_ragged(out["src"], so, out["tgt"], to, out["tsfm"], overlap_radius)
        host = torch.cat([counts[:, 1], out["status"], p_status]).cpu().tolist()    # the one host read, for all pairs
        found, status = host[:P], host[P:2 * P]
        if any(host[2 * P:]):           # (the write call's status is the same function of the same offsets)
            raise RuntimeError("item3d: the pair list reported status %s (2: offsets)" % host[2 * P:])
        if any(f >= 2 ** 31 - 1 for f in found):
            raise RuntimeError("item3d: 2^31 - 1 correspondences or more in one pair")
        c_host = np.concatenate([[0], np.cumsum(found)]).astype(np.int64)
        c_off = torch.from_numpy(c_host).to(device)
        o_src, o_tgt, _, _ = lib.radius_pairs_ragged(out["src"], so, out["tgt"], to, out["tsfm"], overlap_radius, c_off, int(c_host[-1]))
        corr = [torch.stack([o_src[c_host[p]:c_host[p + 1]], o_tgt[c_host[p]:c_host[p + 1]]], dim=1) for p in range(P)]
    else:
        status = out["status"].cpu().tolist()
    if any(status):
        raise RuntimeError("item3d: the prepare kernel reported status %s (2: offsets, 4: selection index out of range, 8: flow rows)" % status)
    pairs = []
    for p, it in enumerate(items):
        d = dict(src_pcd=out["src"][s_off[p]:s_off[p + 1]], tgt_pcd=out["tgt"][t_off[p]:t_off[p + 1]], rot=out["rot"][p],
                 trn=out["trans"][p].reshape(3, 1))
        if kind == "3dmatch":
            d["correspondences"] = corr[p]
            gt_cov = it.get("gt_cov") if isinstance(it, dict) else None
            d["gt_cov"] = None if gt_cov is None else torch.as_tensor(gt_cov).to(device)
        else:
            d["correspondences"] = _to_device(it["correspondences"], device)
            d["s2t_flow"] = out["flow"][r_off[p]:r_off[p + 1]]
            mi = it["metric_index"] if "metric_index" in it else None
            d["metric_index"] = None if mi is None else _to_device(mi, device).squeeze()
        pairs.append(d)
    return pairs


def _features(cloud):
    return torch.ones(cloud.shape[0], 1, dtype=torch.float32, device=cloud.device)


def prepare_item_3dmatch(raw, *, max_points, data_augmentation, rot_factor, augment_noise, overlap_radius, generator=None, draws=None,
                         device="cuda"):
    """-> (src_pcd, tgt_pcd, src_feats, tgt_feats, correspondences, rot, trans, gt_cov), _3dmatch.py:135, as device tensors: clouds float32,
    features ones, correspondences [C, 2] int64 in ascending (i, j), rot [3, 3] / trans [3, 1] float32"""
    d = prepare_batch([raw], kind="3dmatch", max_points=max_points, data_augmentation=data_augmentation, rot_factor=rot_factor,
                      augment_noise=augment_noise, overlap_radius=overlap_radius, generator=generator,
                      draws=None if draws is None else [draws], device=device)[0]
    return (d["src_pcd"], d["tgt_pcd"], _features(d["src_pcd"]), _features(d["tgt_pcd"]), d["correspondences"], d["rot"], d["trn"], d["gt_cov"])


def prepare_item_4dmatch(raw, *, max_points, data_augmentation, rot_factor, augment_noise, overlap_radius=0.0375, generator=None, draws=None,
                         device="cuda"):
    """-> (src_pcd, tgt_pcd, src_feats, tgt_feats, correspondences, rot, trans, s2t_flow, metric_index), _4dmatch.py:146; correspondences and
    metric_index are the entry's own (overlap_radius is not read, as in the reference)"""
    d = prepare_batch([raw], kind="4dmatch", max_points=max_points, data_augmentation=data_augmentation, rot_factor=rot_factor,
                      augment_noise=augment_noise, overlap_radius=overlap_radius, generator=generator,
                      draws=None if draws is None else [draws], device=device)[0]
    return (d["src_pcd"], d["tgt_pcd"], _features(d["src_pcd"]), _features(d["tgt_pcd"]), d["correspondences"], d["rot"], d["trn"],
            d["s2t_flow"], d["metric_index"])


def get_correspondences(src_pcd, tgt_pcd, trans, search_voxel_size, K=None):
    """benchmark_utils.py:166-185 for device tensors: src_pcd [n, 3], tgt_pcd [m, 3] float32, trans [4, 4] -> [C, 2] int64, every (i, j) with
    |trans src_i - tgt_j| < search_voxel_size in ascending (i, j).  One host read (the count)."""
    if K is not None:
        raise NotImplementedError("get_correspondences: K is refused (the reference passes K=None on to KDTree_corr, whatever it is given)")
    dev = src_pcd.device
    src, tgt = _cloud(src_pcd, "src_pcd", dev), _cloud(tgt_pcd, "tgt_pcd", dev)
    T = torch.as_tensor(trans).to(device=dev, dtype=torch.float32)[:3, :4].reshape(1, 3, 4).contiguous()
    so = torch.tensor([0, src.shape[0]], dtype=torch.int32, device=dev)
    to = torch.tensor([0, tgt.shape[0]], dtype=torch.int32, device=dev)
    _, _, counts, status = lib.radius_pairs_ragged(src, so, tgt, to, T, search_voxel_size)
    found, st = torch.cat([counts[0, 1:], status]).tolist()
    if st:
        raise RuntimeError("get_correspondences: the pair list reported status %d" % st)
    if found >= 2 ** 31 - 1:
        raise RuntimeError("get_correspondences: 2^31 - 1 pairs or more")
    c_off = torch.tensor([0, found], dtype=torch.int64, device=dev)
    o_src, o_tgt, _, _ = lib.radius_pairs_ragged(src, so, tgt, to, T, search_voxel_size, c_off, found)
    return torch.stack([o_src, o_tgt], dim=1)
