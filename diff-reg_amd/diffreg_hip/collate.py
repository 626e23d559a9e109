"""Host-side mirror of the reference's collate-time index construction on the HIP kernels.

Same names and argument meaning as the helpers of `3D/datasets/dataloader.py:13-68` -- which call the C++ extensions
cpp_subsampling / cpp_neighbors on the data-loader's CPU workers -- and the level loop of `collate_fn_3dmatch`
(`dataloader.py:120-211`) that builds `points / neighbors / pools / upsamples / stack_lengths` for the KPFCN backbone.
Everything runs on the device through libdiffreg_hip.so (dr_grid_subsample_f32, dr_radius_neighbors_f32); there is no CPU path.
The reference-shaped helpers synchronise once to cut their result to its data-dependent shape, as the reference's return values
require; `build_kpfcn_inputs` does so once per level of `encoder_levels(architecture)`.
The ground-truth products of the training collate -- `coarse_matches`, 4DMatch's `coarse_flow`, the fine-level subsampling -- and the neighbour
calibration (`dataloader.py:232-259, 495-523, 563-591`) are built on dr_coarse_gt_matches_f32, dr_blend_flow_knn3_f32 and dr_radius_count_hist_f32:
`collate_fn_device(training=True)`, `collate_fn_device_4dmatch`, `calibrate_neighbors_device`.
"""
import torch

from . import lib


def _check(status):
    if int(status.item()) != 0:
        raise RuntimeError("collate: a cloud spans more than 65533 cells on an axis (unsupported extent / cell size)")


def batch_grid_subsampling_kpconv(points, batches_len, features=None, labels=None, sampleDl=0.1, max_p=0, verbose=0,
                                  random_grid_orient=True):
    """-> (s_points [m,3] float32, s_len [B] int32); points only (the collate never passes features / labels), max_p = 0.
    Points come per cloud in ascending (iz, iy, ix) voxel order (the reference: std::unordered_map order)."""
    if features is not None or labels is not None or max_p != 0:
        raise NotImplementedError("device grid subsampling: points only, max_p = 0 (what collate_fn_3dmatch uses)")
    out, ol, tot, status = lib.grid_subsample(points, batches_len, sampleDl)
    m = int(tot.item())
    _check(status)
    return out[:m], ol


def batch_neighbors_kpconv(queries, supports, q_batches, s_batches, radius, max_neighbors):
    """-> int64 [nq, min(max_count, max_neighbors)] neighbour indices into the stacked supports, padded with len(supports)"""
    limit = max_neighbors if max_neighbors > 0 else 64
    out, mc, status = lib.radius_neighbors(queries, supports, q_batches, s_batches, radius, limit)
    w = min(int(mc.item()), limit)
    _check(status)
    if max_neighbors <= 0 and int(mc.item()) > limit:
        raise RuntimeError("collate: %d neighbours in one ball, more than the 64 an untruncated query supports" % int(mc.item()))
    return out[:, :w]


def encoder_levels(architecture):
    """The encoder half of a KPFCN architecture string list as resolution levels: [(wide_conv, down, wide_down), ...].
    A level is the run of convolution blocks at one point density; it ends at the block that changes the density (a 'pool' or
    'strided' block: `down` = True) or where the decoder starts ('upsample', or the end of the list; convolutions in front of a
    'global' block are dropped, as the reference's loop drops them).
    wide_conv: the level's convolutions search the deformable radius -- the case when a block BEFORE the level's last convolution
    is deformable (the rule of 3D/datasets/dataloader.py:141-146); wide_down: the density-changing block itself is deformable.
    A level without convolution blocks (two density changes in a row) has wide_conv = None: it gets no neighbour matrix."""
    levels, convs = [], []
    for name in architecture:
        if "global" in name:
            # the reference's loop `continue`s over the convolutions in front of a 'global' block (their successor is not an
            # 'upsample') and then breaks on it: that trailing level is never emitted (dataloader.py:137-146)
            convs = []
            break
        if "upsample" in name:
            break
        if "pool" in name or "strided" in name:
            levels.append((any("deformable" in c for c in convs[:-1]) if convs else None, True, "deformable" in name))
            convs = []
        else:
            convs.append(name)
    if convs:
        levels.append((any("deformable" in c for c in convs[:-1]), False, False))
    return levels


def build_kpfcn_inputs(points, lengths, config, neighborhood_limits):
    """KPFCN index arrays on device (what the level loop of collate_fn_3dmatch builds, dataloader.py:120-211): stacked points
    [n,3] + lengths [2 B] -> dict(points, neighbors, pools, upsamples, stack_lengths) with the reference's dtypes (float32 /
    int64 / int32).  Per level L of encoder_levels(): cell size dl0 2^L, ball radius dl0 conv_radius 2^L (deform_radius in its
    place where the level searches wide); neighbours of the level's cloud in itself; when the level ends in a density change, the
    next cloud = grid subsampling at twice the cell size, `pools` = the next cloud's neighbours in this one, `upsamples` = this
    cloud's neighbours in the next one at twice the radius.
    config: architecture, first_subsampling_dl, conv_radius, deform_radius (attribute or item access)."""
    get = (lambda k: config[k]) if isinstance(config, dict) else (lambda k: getattr(config, k))
    dl0, k_conv, k_deform = get("first_subsampling_dl"), get("conv_radius"), get("deform_radius")
    dev = points.device
    cloud = points.to(torch.float32).contiguous()
    lens = lengths.to(device=dev, dtype=torch.int32)
    no_index = lambda: torch.zeros((0, 1), dtype=torch.int64, device=dev)
    out = dict(points=[], neighbors=[], pools=[], upsamples=[], stack_lengths=[])
    for L, (wide_conv, down, wide_down) in enumerate(encoder_levels(get("architecture"))):
        cell = dl0 * 2 ** L                       # (the reference doubles a running radius: the same float64 values)
        radius = lambda wide: cell * k_conv * k_deform / k_conv if wide else cell * k_conv
        limit = neighborhood_limits[L]
        out["points"].append(cloud)
        out["stack_lengths"].append(lens)
        out["neighbors"].append(no_index() if wide_conv is None else batch_neighbors_kpconv(cloud, cloud, lens, lens, radius(wide_conv), limit))
        if not down:
            out["pools"].append(no_index())
            out["upsamples"].append(no_index())
            cloud, lens = torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0,), dtype=torch.int32, device=dev)
            continue
        coarse, coarse_lens = batch_grid_subsampling_kpconv(cloud, lens, sampleDl=2 * cell * k_conv / k_conv)
        r = radius(wide_down)
        out["pools"].append(batch_neighbors_kpconv(coarse, cloud, coarse_lens, lens, r, limit))
        out["upsamples"].append(batch_neighbors_kpconv(cloud, coarse, lens, coarse_lens, 2 * r, limit))
        cloud, lens = coarse, coarse_lens
    return out


_PAIR_KEYS = ("src_pcd", "tgt_pcd", "rot", "trn", "correspondences", "gt_cov", "s2t_flow", "metric_index")


def _pair_fields(pair):
    """one entry of `pairs` as a dict over _PAIR_KEYS: either the positional (src_pcd, tgt_pcd[, rot, trn]) or, for everything behind those
    four, a dict with these keys (src_pcd and tgt_pcd required) -- the positional form does not grow"""
    if isinstance(pair, dict):
        unknown = [k for k in pair if k not in _PAIR_KEYS]
        if unknown or "src_pcd" not in pair or "tgt_pcd" not in pair:
            raise ValueError("collate: a pair dict has src_pcd, tgt_pcd and optionally %s (got %s)" % (", ".join(_PAIR_KEYS[2:]), sorted(pair)))
        return {k: pair.get(k) for k in _PAIR_KEYS}
    if len(pair) not in (2, 4):
        raise ValueError("collate: a positional pair is (src_pcd, tgt_pcd) or (src_pcd, tgt_pcd, rot, trn); pass a dict with the keys %s for "
                         "anything more" % (_PAIR_KEYS,))
    f = dict.fromkeys(_PAIR_KEYS)
    f.update(zip(_PAIR_KEYS, pair))
    return f


def _config_get(config):
    return (lambda k: config[k]) if isinstance(config, dict) else (lambda k: getattr(config, k))


def _offsets(counts):
    """[P] counts (device) -> int32 [P + 1] exclusive prefix sums on the same device, no host read"""
    o = torch.zeros(counts.shape[0] + 1, dtype=torch.int32, device=counts.device)
    o[1:] = torch.cumsum(counts, 0)
    return o


def _coarse_ground_truth(d, fields, config, coarse_level, flows=None):
    """the `get match at coarse level` block of dataloader.py:253-257 (3D) / 512-520 (4D, `flows` = the pairs' s2t_flow) for all pairs in two
    (4D: three) library calls and ONE host read: -> (coarse_matches, coarse_flow or None), lists over the pairs"""
    get = _config_get(config)
    dev = d["features"].device
    coarse = d["points"][coarse_level]
    cnt = d["stack_lengths"][coarse_level].view(-1, 2)
    P = cnt.shape[0]
    src_c, tgt_c = coarse[d["src_ind_coarse"]], coarse[d["tgt_ind_coarse"]]
    s_off, t_off = _offsets(cnt[:, 0]), _offsets(cnt[:, 1])
    flow_c = bstat = None
    if flows is not None:
        raw = torch.cat([f["src_pcd"].to(device=dev, dtype=torch.float32) for f in fields])      # batched_points_list[2 * entry]
        r_off = torch.tensor([0] + [f["src_pcd"].shape[0] for f in fields], dtype=torch.int64).cumsum(0).to(device=dev, dtype=torch.int32)
        flow_c, bstat = lib.blend_flow_knn3(src_c, s_off, raw, torch.cat(flows), r_off)
    o_src, o_tgt, counts, status = lib.coarse_gt_matches(src_c, s_off, tgt_c, t_off, d["batched_rot"], d["batched_trn"],
                                                         get("coarse_match_radius"), src_flow=flow_c)
    words = [counts, status, s_off] + ([bstat] if bstat is not None else [])
    host = torch.cat(words).cpu().tolist()                                                          # the one host read, for all pairs
    counts_h, status_h, off_h = host[:P], host[P:2 * P], host[2 * P:3 * P + 1]
    for p in range(P):
        if bstat is not None and host[3 * P + 1 + p]:
            raise ValueError("collate: pair %d has fewer than 4 source points to blend the scene flow from (np.argpartition(kth=3) raises "
                             "in the reference)" % p)
        if status_h[p]:
            raise ValueError("collate: pair %d has fewer than 2 source or target points at the coarse level (np.argpartition(kth=1) raises "
                             "in the reference)" % p)
    matches = [torch.stack([o_src[off_h[p]:off_h[p] + counts_h[p]], o_tgt[off_h[p]:off_h[p] + counts_h[p]]]) for p in range(P)]
    flow_list = None if flow_c is None else [flow_c[off_h[p]:off_h[p + 1]] for p in range(P)]
    return matches, flow_list


def _stack_or_none(items):
    if any(x is None for x in items):
        return None
    if all(torch.is_tensor(x) for x in items):
        return torch.stack(items)
    import numpy as np
    return np.stack([x.cpu().numpy() if torch.is_tensor(x) else x for x in items], axis=0)


def collate_fn_device(pairs, config, neighborhood_limits, coarse_level=-2, training=True):
    """collate_fn_3dmatch (dataloader.py:70-325) on device: `pairs` = [(src_pcd [n,3], tgt_pcd [m,3][, rot [3,3], trn [3,1]]), ...] (device
    tensors), or dicts with the keys src_pcd, tgt_pcd, rot, trn, correspondences, gt_cov (the positional form stops at trn) -> the input dict
    of Pipeline.forward: the KPFCN index arrays (build_kpfcn_inputs), `features` = ones, and the coarse-level masks / split indices of
    dataloader.py:213-262.
    With `training` and rot / trn present it also carries the collate's ground-truth products: `coarse_matches` (per pair a [2, C_p] int64
    device tensor: dataloader.py:253-257 on dr_coarse_gt_matches_f32, one host read for all pairs; config needs `coarse_match_radius`),
    `fine_pts` / `fine_length` / `fine_ind` (dataloader.py:232-233 on the grid subsampling and the radius search; fine_ind is always 1-D, where
    the reference's squeeze() makes a single fine point 0-D), `src_pcd_list` / `tgt_pcd_list`, and `correspondences_list` / `gt_cov` as the
    pairs carry them (gt_cov: None when a pair has none).  training=False returns the inference half alone."""
    fields = [_pair_fields(p) for p in pairs]
    dev = fields[0]["src_pcd"].device
    pts, lens = [], []
    for f in fields:
        pts += [f["src_pcd"].to(torch.float32), f["tgt_pcd"].to(torch.float32)]
        lens += [f["src_pcd"].shape[0], f["tgt_pcd"].shape[0]]
    points = torch.cat(pts)
    lengths = torch.tensor(lens, dtype=torch.int32, device=dev)
    d = build_kpfcn_inputs(points, lengths, config, neighborhood_limits)
    d["features"] = torch.ones(points.shape[0], 1, device=dev)                    # in_feats_dim = 1 (3DMatch: occupancy)
    cnt = d["stack_lengths"][coarse_level].view(-1, 2).to(torch.int64)            # [B, 2] points of src / tgt at the coarse level
    B = cnt.shape[0]
    smax, tmax = int(cnt[:, 0].max()), int(cnt[:, 1].max())                       # one sync: the padded extents are shapes
    ar_s, ar_t = torch.arange(smax, device=dev), torch.arange(tmax, device=dev)
    d["src_mask"] = ar_s[None, :] < cnt[:, :1]
    d["tgt_mask"] = ar_t[None, :] < cnt[:, 1:]
    start = torch.cumsum(cnt.sum(1), 0) - cnt.sum(1)                               # first coarse row of every pair
    rows = torch.arange(B, device=dev)[:, None]
    d["src_ind_coarse_split"] = (ar_s[None, :] + rows * smax)[d["src_mask"]]
    d["tgt_ind_coarse_split"] = (ar_t[None, :] + rows * tmax)[d["tgt_mask"]]
    d["src_ind_coarse"] = (ar_s[None, :] + start[:, None])[d["src_mask"]]
    d["tgt_ind_coarse"] = (ar_t[None, :] + (start + cnt[:, 0])[:, None])[d["tgt_mask"]]
    if fields[0]["rot"] is not None:
        d["batched_rot"] = torch.stack([f["rot"].to(torch.float32) for f in fields])
        d["batched_trn"] = torch.stack([f["trn"].to(torch.float32).reshape(3, 1) for f in fields])
    if not training or fields[0]["rot"] is None:
        return d
    get = _config_get(config)
    try:
        get("coarse_match_radius")
    except (KeyError, AttributeError):
        raise ValueError("collate_fn_device: the ground-truth matches need config['coarse_match_radius'] (pass training=False for the inference "
                         "half alone)") from None
    d["src_pcd_list"] = [f["src_pcd"] for f in fields]
    d["tgt_pcd_list"] = [f["tgt_pcd"] for f in fields]
    d["coarse_matches"], _ = _coarse_ground_truth(d, fields, config, coarse_level)
    d["gt_cov"] = _stack_or_none([f["gt_cov"] for f in fields])
    d["correspondences_list"] = [f["correspondences"] for f in fields]
    # dataloader.py:232-233: `dl` there is the cell size the level loop's LAST density change left behind
    downs = [L for L, (_, down, _) in enumerate(encoder_levels(get("architecture"))) if down]
    if not downs:
        raise ValueError("collate_fn_device: the fine-level subsampling takes its cell size from a pool / strided block; this architecture "
                         "has none (the reference's `dl` is undefined there)")
    cell, k_conv = get("first_subsampling_dl") * 2 ** downs[-1], get("conv_radius")
    fine_dl = (2 * cell * k_conv / k_conv) * 0.5 * 0.85
    p0, l0 = d["points"][0], d["stack_lengths"][0]
    d["fine_pts"], d["fine_length"] = batch_grid_subsampling_kpconv(p0, l0, sampleDl=fine_dl)
    ind, _, _ = lib.radius_neighbors(d["fine_pts"], p0, d["fine_length"], l0, fine_dl, 1)
    d["fine_ind"] = ind[:, 0]
    return d


def collate_fn_device_4dmatch(pairs, config, neighborhood_limits, coarse_level=-2):
    """collate_fn_4dmatch (dataloader.py:331-559) on device: `pairs` = dicts with src_pcd, tgt_pcd, rot, trn, s2t_flow [n, 3] and optionally
    correspondences, metric_index (device tensors) -> the dict of dataloader.py:536-557: the inference half of collate_fn_device plus
    `coarse_flow` (per pair [n_s, 3] float32: blend_scene_flow of the coarse source points in the pair's RAW source cloud, knn = 3, on
    dr_blend_flow_knn3_f32), `coarse_matches` (the coarse sources moved by that flow, then warped, then the mutual nearest neighbours inside
    coarse_match_radius), `src_pcd_list`, `tgt_pcd_list`, `correspondences_list`, `sflow_list` and `metric_index_list` (None when any pair has
    none).  One host read serves all pairs."""
    fields = [_pair_fields(p) for p in pairs]
    for k in ("rot", "trn", "s2t_flow"):
        if any(f[k] is None for f in fields):
            raise ValueError("collate_fn_device_4dmatch: every pair needs %s" % k)
    for f in fields:
        if f["s2t_flow"].shape != f["src_pcd"].shape:
            raise ValueError("collate_fn_device_4dmatch: s2t_flow has one row per source point")
    d = collate_fn_device([{k: f[k] for k in ("src_pcd", "tgt_pcd", "rot", "trn")} for f in fields], config, neighborhood_limits,
                          coarse_level=coarse_level, training=False)
    dev = d["features"].device
    d["sflow_list"] = [f["s2t_flow"].to(device=dev, dtype=torch.float32) for f in fields]
    d["coarse_matches"], d["coarse_flow"] = _coarse_ground_truth(d, fields, config, coarse_level, flows=d["sflow_list"])
    d["src_pcd_list"] = [f["src_pcd"] for f in fields]
    d["tgt_pcd_list"] = [f["tgt_pcd"] for f in fields]
    d["correspondences_list"] = [f["correspondences"] for f in fields]
    d["metric_index_list"] = None if any(f["metric_index"] is None for f in fields) else [f["metric_index"] for f in fields]
    return d


def _sample_clouds(sample, device):
    """a calibration sample -> (src [n,3], tgt [m,3]) float32 on the device: a pair dict, or any sequence whose first two entries are the clouds
    (a dataset's __getitem__ tuple), numpy or torch"""
    src, tgt = (sample["src_pcd"], sample["tgt_pcd"]) if isinstance(sample, dict) else (sample[0], sample[1])
    to = lambda a: torch.as_tensor(a, dtype=torch.float32).to(device)
    return to(src), to(tgt)


def neighbor_histograms_device(samples, config, samples_threshold=2000, device="cuda"):
    """the accumulation half of calibrate_neighbors (dataloader.py:566-583) on device -> int32 [num_layers, hist_n] device histogram of the
    per-point neighbour counts below hist_n = ceil(4/3 pi (deform_radius + 1)^3).  Per sample the level loop's conv_i geometry (the levels and
    radii of build_kpfcn_inputs, wide-radius rule included) is run with dr_radius_count_hist_f32 in place of the neighbour search: no neighbour
    matrix is built.  Stops after the sample that brings every layer above samples_threshold queries, like the reference (one host read per
    sample)."""
    import numpy as np
    get = _config_get(config)
    dl0, k_conv, k_deform, num_layers = get("first_subsampling_dl"), get("conv_radius"), get("deform_radius"), int(get("num_layers"))
    hist_n = int(np.ceil(4 / 3 * np.pi * (k_deform + 1) ** 3))
    if hist_n > 4096:
        raise ValueError("calibrate_neighbors_device: hist_n = %d bins (deform_radius %g) exceed the 4096 dr_radius_count_hist_f32 keeps on chip"
                         % (hist_n, k_deform))
    levels = encoder_levels(get("architecture"))
    if len(levels) != num_layers:
        raise ValueError("calibrate_neighbors_device: the architecture has %d resolution levels, config.num_layers is %d (the reference's "
                         "histogram update raises there)" % (len(levels), num_layers))
    hist = None
    for sample in samples:
        src, tgt = _sample_clouds(sample, device)
        if hist is None:
            hist = torch.zeros(num_layers, hist_n, dtype=torch.int32, device=src.device)
        cloud = torch.cat([src, tgt])
        lens = torch.tensor([src.shape[0], tgt.shape[0]], dtype=torch.int32, device=src.device)
        status = None
        for L, (wide_conv, down, _) in enumerate(levels):
            cell = dl0 * 2 ** L
            if wide_conv is not None:
                radius = cell * k_conv * k_deform / k_conv if wide_conv else cell * k_conv
                status = lib.radius_count_hist(cloud, cloud, lens, lens, radius, hist[L])
            if not down:
                break
            cloud, lens = batch_grid_subsampling_kpconv(cloud, lens, sampleDl=2 * cell * k_conv / k_conv)
        if status is not None:
            _check(status)
        if int(hist.sum(1).min().item()) > samples_threshold:
            break
    if hist is None:
        raise ValueError("calibrate_neighbors_device: no samples")
    return hist


def calibrate_neighbors_device(samples, config, keep_ratio=0.8, samples_threshold=2000, device="cuda"):
    """calibrate_neighbors (dataloader.py:563-591) on device -> the neighbourhood limits as a numpy int array [num_layers].  `samples`: any
    iterable of source / target clouds (pair dicts, (src, tgt, ...) sequences, a dataset's items); the histogram is neighbor_histograms_device's,
    the limits the percentile of dataloader.py:585-588."""
    import numpy as np
    neighb_hists = neighbor_histograms_device(samples, config, samples_threshold, device).cpu().numpy()
    cumsum = np.cumsum(neighb_hists.T, axis=0)
    return np.sum(cumsum < (keep_ratio * cumsum[neighb_hists.shape[1] - 1, :]), axis=0)
