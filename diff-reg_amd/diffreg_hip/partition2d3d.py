"""The patch partition and the ground-truth patch overlaps of the 2D-3D model on the device (csrc/partition2d3d.hip), under the reference's
function names, argument orders, dtypes and return tuples, so that `overlay2d3d.accelerate(model, partition=True)` can bind them in place of

    point_to_node_partition          vision3d/ops/point_cloud_partition.py:41-104      (EXP/model.py:403-409)
    patchify                         EXP/utils.py:28-56                                 (model.py:447-458)
    get_2d3d_node_correspondences    EXP/utils.py:59-175                                (model.py:480-495)
    multual_nn_correspondence        EXP/utils.py:234-252  (sic)                        (utils.py:104)
    get_correspondences, to_o3d_pcd  EXP/utils.py:409-432                               (model.py:569, training only)

EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.  Device tensors only (no CPU path).  Where the reference returns a
tensor whose length is data dependent the wrapper reads ONE small count from the device to size the views; `point_to_node_partition(...,
width=K)` reads nothing.  `coarse_match_gt` and the pairs of get_correspondences are device tensors (the reference builds them on the host).
get_correspondences is PARITY UNPINNED against Open3D's KD-tree: it returns the pairs of the definition |T s_i - t_j| < r in ascending
(i, j) order; the reference's per-query KD-tree order is read by nothing downstream (model.py:574-577, 603-604 scatter ones).
"""
import numpy as np
import torch

from . import lib
from .lib import check, ensure_init, mask_u8, ptr, stream_of

_raw = lib.raw()
MAX_POINT_LIMIT = 128


def _f32(x):
    return x.detach().contiguous().float()


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def point_to_node_partition(points, nodes, point_limit=None, return_count=False, gather_points=True, inf=1e12, width=None):
    """-> (point_to_node [Nf] int64[, node_sizes [Nc] int64][, node_masks [Nc] bool, node_knn_indices [Nc, W] int64 (padding = Nf), node_knn_masks [Nc, W] bool])
    with W = min(largest node, point_limit) as the reference's (one 4-byte host read), or W = `width` (<= point_limit) given by the caller: no host read at
    all.  point_limit None = 128, the largest the kernel serves: a node larger than that raises instead of being cut silently."""
    ensure_init()
    points, nodes = _f32(points), _f32(nodes)
    Nf, Nc = points.shape[0], nodes.shape[0]
    K = MAX_POINT_LIMIT if point_limit is None else int(point_limit)
    dev = points.device
    p2n = torch.empty(Nf, dtype=torch.int64, device=dev)
    sizes = torch.empty(Nc, dtype=torch.int64, device=dev)
    masks = torch.empty(Nc, dtype=torch.bool, device=dev)
    knn_idx = torch.empty(Nc, K, dtype=torch.int64, device=dev)
    knn_masks = torch.empty(Nc, K, dtype=torch.bool, device=dev)
    mx = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = _raw.dr_point_to_node_partition_workspace_bytes(Nf)
    ws = _ws(wsb, dev)
    check(_raw.dr_point_to_node_partition_f32(Nf, Nc, K, ptr(points), ptr(nodes), ptr(p2n), ptr(sizes), ptr(mask_u8(masks)), ptr(knn_idx),
                                              ptr(mask_u8(knn_masks)), ptr(mx), ptr(ws), wsb, stream_of(points)))
    out = [p2n]
    if return_count:
        out.append(sizes)
    if gather_points:
        if width is None:
            largest = int(mx.item())
            assert largest > 0, "All nodes are empty."
            if point_limit is None and largest > K:
                raise RuntimeError("point_to_node_partition: a node holds %d points; without point_limit at most %d are served" % (largest, K))
            width = min(largest, K)
        elif not 0 < int(width) <= K:
            raise ValueError("width must lie in 1 .. point_limit")
        width = int(width)
        out += [masks, knn_idx if width == K else knn_idx[:, :width].contiguous(), knn_masks if width == K else knn_masks[:, :width].contiguous()]
    return tuple(out)


def patchify(img_points, img_points_da, img_pixels, img_masks, img_masks_da, img_h_f, img_w_f, img_h_c, img_w_c, stride=1):
    """-> (knn_points [M,Ki,3], knn_points_da [M,Ki,3], knn_pixels [M,Ki,2], knn_indices [M,Ki] int64, knn_masks, knn_masks_da [M,Ki] bool, masks, masks_da [M] bool)"""
    ensure_init()
    assert img_h_f % img_h_c == 0, f"Image height must be divisible by patch height ({img_h_f} vs {img_h_c})."
    assert img_w_f % img_w_c == 0, f"Image width must be divisible by patch width ({img_w_f} vs {img_w_c})."
    pts, pts_da, pix = _f32(img_points).view(-1, 3), _f32(img_points_da).view(-1, 3), _f32(img_pixels).view(-1, 2)
    m, m_da = mask_u8(img_masks.reshape(-1)), mask_u8(img_masks_da.reshape(-1))
    n = img_h_f * img_w_f
    assert pts.shape[0] == n and pts_da.shape[0] == n and pix.shape[0] == n and m.numel() == n and m_da.numel() == n
    M = img_h_c * img_w_c
    Ki = -(-(img_h_f // img_h_c) // stride) * -(-(img_w_f // img_w_c) // stride)
    dev = pts.device
    o_pts, o_da, o_pix = torch.empty(M, Ki, 3, device=dev), torch.empty(M, Ki, 3, device=dev), torch.empty(M, Ki, 2, device=dev)
    o_idx = torch.empty(M, Ki, dtype=torch.int64, device=dev)
    o_m, o_mda = torch.empty(M, Ki, dtype=torch.bool, device=dev), torch.empty(M, Ki, dtype=torch.bool, device=dev)
    nm, nm_da = torch.empty(M, dtype=torch.bool, device=dev), torch.empty(M, dtype=torch.bool, device=dev)
    check(_raw.dr_patchify_f32(img_h_f, img_w_f, img_h_c, img_w_c, int(stride), ptr(pts), ptr(pts_da), ptr(pix), ptr(m), ptr(m_da), ptr(o_pts), ptr(o_da),
                               ptr(o_pix), ptr(o_idx), ptr(mask_u8(o_m)), ptr(mask_u8(o_mda)), ptr(mask_u8(nm)), ptr(mask_u8(nm_da)), stream_of(pts)))
    return o_pts, o_da, o_pix, o_idx, o_m, o_mda, nm, nm_da


def _transform_f32(transform, dev):
    return torch.as_tensor(np.asarray(transform) if not torch.is_tensor(transform) else transform).detach().to(device=dev, dtype=torch.float32).reshape(4, 4).contiguous()


def multual_nn_correspondence(src_pcd_deformed, tgt_pcd, search_radius=0.3, knn=1):
    """-> (2, C) int64 device tensor: row 0 the sources, row 1 their targets, ascending source index (the reference returns this array on the host)"""
    if knn != 1:
        raise NotImplementedError("multual_nn_correspondence: knn = 1 only (the reference reads column 0 of its k-NN whatever knn is)")
    ensure_init()
    src, tgt = _f32(src_pcd_deformed), _f32(tgt_pcd)
    ns, nt = src.shape[0], tgt.shape[0]
    dev = src.device
    out = torch.empty(2, max(ns, 1), dtype=torch.int64, device=dev)
    cnt = torch.empty(1, dtype=torch.int32, device=dev)
    wsb = _raw.dr_mutual_nn_radius_workspace_bytes(ns, nt)
    ws = _ws(wsb, dev)
    check(_raw.dr_mutual_nn_radius_f32(ns, nt, ptr(src), ptr(tgt), float(search_radius), ptr(out[0]), ptr(out[1]), ptr(cnt), ptr(ws), wsb, stream_of(src)))
    return out[:, :int(cnt.item())]


def node_correspondences_raw(img_masks, img_knn_points, img_knn_points_da, img_knn_pixels, img_knn_masks, img_knn_masks_da, pcd_masks, pcd_knn_points,
                             pcd_knn_pixels, pcd_knn_masks, transform, pos_radius_2d, pos_radius_3d, capacity=None, out=None):
    """dr_node_correspondences_2d3d_f32 without a host read -> dict(img_corr_indices, pcd_corr_indices, img_corr_overlaps, pcd_corr_overlaps: `capacity` rows
    each, counts int32 [3] = (pairs written, candidates kept, candidates found), pcd_centers, img_centers, img_centers_da).  `out`: the four lists, preallocated."""
    ensure_init()
    ip, ipd, ix = _f32(img_knn_points), _f32(img_knn_points_da), _f32(img_knn_pixels)
    pp, px = _f32(pcd_knn_points), _f32(pcd_knn_pixels)
    M, Ki = ip.shape[:2]
    N, Kc = pp.shape[:2]
    dev = ip.device
    capacity = int(capacity) if capacity is not None else M * N
    T = _transform_f32(transform, dev)
    if out is None:
        out = (torch.empty(capacity, dtype=torch.int64, device=dev), torch.empty(capacity, dtype=torch.int64, device=dev),
               torch.empty(capacity, device=dev), torch.empty(capacity, device=dev))
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    pc, ic, icd = torch.empty(N, 3, device=dev), torch.empty(M, 3, device=dev), torch.empty(M, 3, device=dev)
    wsb = _raw.dr_node_correspondences_2d3d_workspace_bytes(M, N, Kc, capacity)
    ws = _ws(wsb, dev)
    check(_raw.dr_node_correspondences_2d3d_f32(M, Ki, N, Kc, ptr(mask_u8(img_masks)), ptr(ip), ptr(ipd), ptr(ix), ptr(mask_u8(img_knn_masks)),
                                                ptr(mask_u8(img_knn_masks_da)), ptr(mask_u8(pcd_masks)), ptr(pp), ptr(px), ptr(mask_u8(pcd_knn_masks)), ptr(T),
                                                float(pos_radius_2d), float(pos_radius_3d), capacity, ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]),
                                                ptr(counts), ptr(pc), ptr(ic), ptr(icd), ptr(ws), wsb, stream_of(ip)))
    return dict(img_corr_indices=out[0], pcd_corr_indices=out[1], img_corr_overlaps=out[2], pcd_corr_overlaps=out[3], counts=counts, pcd_centers=pc,
                img_centers=ic, img_centers_da=icd)


def get_2d3d_node_correspondences(img_masks, img_masks_da, img_knn_points, img_knn_points_da, img_knn_pixels, img_knn_masks, img_knn_masks_da, pcd_masks,
                                  pcd_knn_points, pcd_knn_pixels, pcd_knn_masks, transform, pos_radius_2d, pos_radius_3d, capacity=None):
    """-> the reference's 8-tuple (img_corr_indices, pcd_corr_indices, img_corr_overlaps, pcd_corr_overlaps, pcd_centers, img_centers, img_centers_da,
    coarse_match_gt).  `capacity`: room for candidate patch pairs (default: every pair, M x N); more candidates than that raise RuntimeError."""
    r = node_correspondences_raw(img_masks, img_knn_points, img_knn_points_da, img_knn_pixels, img_knn_masks, img_knn_masks_da, pcd_masks, pcd_knn_points,
                                 pcd_knn_pixels, pcd_knn_masks, transform, pos_radius_2d, pos_radius_3d, capacity)
    coarse_match_gt = multual_nn_correspondence(r["pcd_centers"], r["img_centers"], search_radius=0.06)      # (utils.py:104; its host read orders the stream)
    n, kept, found = r["counts"].tolist()
    if found > kept:
        raise RuntimeError("get_2d3d_node_correspondences: %d candidate patch pairs, room for %d: pass a larger capacity" % (found, kept))
    return (r["img_corr_indices"][:n], r["pcd_corr_indices"][:n], r["img_corr_overlaps"][:n], r["pcd_corr_overlaps"][:n], r["pcd_centers"], r["img_centers"],
            r["img_centers_da"], coarse_match_gt)


def radius_pairs_raw(src, tgt, transform, radius, capacity=None, out=None):
    """dr_radius_pairs_f32 without a host read -> (out_src, out_tgt int64 [capacity], counts int32 [2] = (written, found))"""
    ensure_init()
    src, tgt = _f32(src), _f32(tgt)
    ns, nt = src.shape[0], tgt.shape[0]
    dev = src.device
    capacity = int(capacity) if capacity is not None else ns * nt
    T = None if transform is None else _transform_f32(transform, dev)
    if out is None:
        out = (torch.empty(max(capacity, 1), dtype=torch.int64, device=dev), torch.empty(max(capacity, 1), dtype=torch.int64, device=dev))
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    wsb = _raw.dr_radius_pairs_workspace_bytes(ns, nt)
    ws = _ws(wsb, dev)
    check(_raw.dr_radius_pairs_f32(ns, nt, ptr(src), ptr(tgt), ptr(T), float(radius), capacity, ptr(out[0]), ptr(out[1]), ptr(counts), ptr(ws), wsb,
                                   stream_of(src)))
    return out[0], out[1], counts


def to_o3d_pcd(xyz):
    """identity on tensors: get_correspondences below takes the points themselves (EXP/utils.py:409-416 wraps them for Open3D)"""
    return xyz


def get_correspondences(src_pcd, tgt_pcd, trans, search_voxel_size, K=None, capacity=None):
    """-> (C, 2) int64 device tensor of the pairs (i, j) with |trans src_i - tgt_j| < search_voxel_size, ascending (i, j).  K is ignored, as the reference
    ignores it (it passes K=None on, utils.py:430)."""
    i, j, counts = radius_pairs_raw(src_pcd, tgt_pcd, trans, search_voxel_size, capacity)
    n, found = counts.tolist()
    if found > n:
        raise RuntimeError("get_correspondences: %d pairs, room for %d: pass a larger capacity" % (found, n))
    return torch.stack([i[:n], j[:n]], dim=1)
