"""The 2D-3D loader's graph pyramid and the calibration of its neighbour limits on the device.

Same names and argument meaning as vision3d's collate-time helpers, on device tensors instead of numpy arrays:

    grid_subsample_pack_mode                         vision3d/array_ops/grid_subsample.py:7-22   (csrc/cpu/grid_subsampling)
    radius_search_pack_mode                          vision3d/array_ops/radius_search.py:7-27    (csrc/cpu/radius_neighbors, nanoflann)
    build_grid_and_radius_graph_pyramid_pack_mode    vision3d/array_ops/graph_pyramid.py:9-70
    pyramidless_pack_mode                            what the loader's collate calls instead, so that it leaves `points` a tensor
    GraphPyramid2D3DCollate                          step 3 of GraphPyramid2D3DRegistrationCollateFn, vision3d/utils/collate.py:265-310
    calibrate_neighbors_pack_mode                    vision3d/utils/dataloader.py:42-67

Everything runs through libdiffreg_hip.so (dr_grid_subsample_vision3d_f32, dr_radius_neighbors_f32, dr_radius_count_hist_f32); there is no CPU
path.  Lengths are int64 in and out, as the reference's are.  Stage points come per cloud in ascending (iz, iy, ix) voxel order where the reference
emits std::unordered_map order; the index matrices refer to that order.  Every function that returns a data-dependent shape synchronises once for it.
"""
import math

import torch

from . import lib

MAX_NEIGHBOR_LIMIT = 64          # dr_radius_neighbors_f32 keeps at most 64 candidates per query


def _check(status):
    if int(status.item()) != 0:
        raise RuntimeError("pyramid2d3d: a cloud spans more than 65533 cells on an axis (unsupported extent / cell size)")


def _check_limits(neighbor_limits):
    for limit in neighbor_limits:
        if int(limit) > MAX_NEIGHBOR_LIMIT:
            raise NotImplementedError("pyramid2d3d: neighbour limit %d is above the %d the device radius search keeps per query"
                                      % (int(limit), MAX_NEIGHBOR_LIMIT))
        if int(limit) < 1:
            raise NotImplementedError("pyramid2d3d: neighbour limit %d: an uncut search (limit <= 0) has no device form" % int(limit))


def grid_subsample_pack_mode(points, lengths, voxel_size):
    """-> (s_points [M, 3] float32, s_lengths [B] int64): the barycentre of every occupied voxel of every cloud"""
    out, ol, tot, status = lib.grid_subsample(points, lengths, voxel_size, vision3d=True)
    m = int(tot.item())
    _check(status)
    return out[:m], ol.to(torch.int64)


def radius_search_pack_mode(q_points, s_points, q_lengths, s_lengths, radius, neighbor_limit):
    """-> int64 [N, min(max_count, neighbor_limit)]: per query the supports of its own cloud with d^2 < radius^2, nearest first, padded with M"""
    _check_limits([neighbor_limit])
    out, mc, status = lib.radius_neighbors(q_points, s_points, q_lengths, s_lengths, radius, int(neighbor_limit))
    w = min(int(mc.item()), int(neighbor_limit))
    _check(status)
    return out[:, :w]


def build_grid_and_radius_graph_pyramid_pack_mode(points, lengths, num_stages, voxel_size, radius, neighbor_limits):
    """-> dict(points, lengths, neighbors, subsampling, upsampling): lists of device tensors with the reference's dtypes (float32 / int64)"""
    assert num_stages is not None and voxel_size is not None and radius is not None and neighbor_limits is not None
    assert num_stages == len(neighbor_limits)
    _check_limits(neighbor_limits)
    points = points.to(torch.float32).contiguous()
    lengths = lengths.to(device=points.device, dtype=torch.int64)
    points_list, lengths_list, neighbors_list, subsampling_list, upsampling_list = [], [], [], [], []
    for i in range(num_stages):
        if i > 0:
            points, lengths = grid_subsample_pack_mode(points, lengths, voxel_size)
        points_list.append(points)
        lengths_list.append(lengths)
        voxel_size *= 2
    for i in range(num_stages):
        cur_points, cur_lengths = points_list[i], lengths_list[i]
        neighbors_list.append(radius_search_pack_mode(cur_points, cur_points, cur_lengths, cur_lengths, radius, neighbor_limits[i]))
        if i < num_stages - 1:
            sub_points, sub_lengths = points_list[i + 1], lengths_list[i + 1]
            subsampling_list.append(radius_search_pack_mode(sub_points, cur_points, sub_lengths, cur_lengths, radius, neighbor_limits[i]))
            upsampling_list.append(radius_search_pack_mode(cur_points, sub_points, cur_lengths, sub_lengths, radius * 2, neighbor_limits[i + 1]))
        radius *= 2
    return {"points": points_list, "lengths": lengths_list, "neighbors": neighbors_list, "subsampling": subsampling_list,
            "upsampling": upsampling_list}


def pyramidless_pack_mode(points, lengths, *args, **kwargs):
    """Stands in for build_grid_and_radius_graph_pyramid_pack_mode inside the reference's collate classes (bind it to that name in
    vision3d.utils.collate): the stacked points and their lengths go through as they are, so the collate's own tensor conversion and the training
    loop's device transfer deliver the dict GraphPyramid2D3DCollate and accelerate(model, pyramid=...) take."""
    return {"points": points, "lengths": lengths}


class GraphPyramid2D3DCollate:
    """The pyramid step of GraphPyramid2D3DRegistrationCollateFn on the device: __call__(data_dict) takes the dict of a pyramid-less collate
    (`points` a [N, 3] tensor and `lengths`, already on the device) and replaces the two with the five lists."""

    def __init__(self, num_stages, voxel_size, search_radius, neighbor_limits):
        assert num_stages == len(neighbor_limits)
        _check_limits(neighbor_limits)
        self.num_stages, self.voxel_size, self.search_radius = num_stages, voxel_size, search_radius
        self.neighbor_limits = [int(x) for x in neighbor_limits]

    def __call__(self, data_dict):
        points = data_dict.pop("points")
        lengths = data_dict.pop("lengths", None)
        if lengths is None:
            lengths = torch.tensor([points.shape[0]], dtype=torch.int64, device=points.device)
        data_dict.update(build_grid_and_radius_graph_pyramid_pack_mode(points, torch.as_tensor(lengths), self.num_stages, self.voxel_size,
                                                                       self.search_radius, self.neighbor_limits))
        return data_dict


def _sample_points(item, device):
    """a sample of the calibration's dataset: a point tensor [n, 3], a dict with `points` (and optionally `lengths`), or (points, lengths)"""
    lengths = None
    if isinstance(item, dict):
        item, lengths = item["points"], item.get("lengths")
    elif isinstance(item, (tuple, list)):
        item, lengths = item
    points = torch.as_tensor(item, dtype=torch.float32)
    points = points.to(device if device is not None else (points.device if points.is_cuda else "cuda"))
    if lengths is None:
        lengths = torch.tensor([points.shape[0]], dtype=torch.int64)
    return points, torch.as_tensor(lengths).to(points.device)


def neighbor_histograms(points, lengths, num_stages, voxel_size, search_radius, hist):
    """adds one sample's neighbour-count histograms to hist int32 [num_stages, hist_n] (device): the subsample chain, then one count launch per
    stage (the stage's points in themselves at radius search_radius 2^stage) -- no neighbour matrix is built, so no limit applies"""
    for i in range(num_stages):
        if i > 0:
            points, lengths = grid_subsample_pack_mode(points, lengths, voxel_size)
        _check(lib.radius_count_hist(points, points, lengths, lengths, search_radius, hist[i]))
        voxel_size *= 2
        search_radius *= 2


def calibrate_neighbors_pack_mode(dataset, num_stages, voxel_size, search_radius, keep_ratio=0.8, sample_threshold=2000, device=None):
    """-> int64 numpy array [num_stages]: the neighbour limits the reference's calibration returns.  Histogram of the per-query neighbour counts
    below hist_n = ceil(4/3 pi (r / v + 1)^3) per stage, accumulated sample after sample until every stage holds more than sample_threshold
    queries; limit = the number of bins whose cumulative sum lies below keep_ratio of the total."""
    import numpy as np
    hist_n = int(math.ceil(4 / 3 * math.pi * (search_radius / voxel_size + 1) ** 3))
    hist = None
    indexed = hasattr(dataset, "__getitem__") and hasattr(dataset, "__len__")          # a torch Dataset need not stop an iteration itself
    for item in ((dataset[i] for i in range(len(dataset))) if indexed else dataset):
        points, lengths = _sample_points(item, device)
        if hist is None:
            hist = torch.zeros(num_stages, hist_n, dtype=torch.int32, device=points.device)
        neighbor_histograms(points, lengths, num_stages, voxel_size, search_radius, hist)
        if int(hist.sum(1).min().item()) > sample_threshold:
            break
    if hist is None:
        raise ValueError("calibrate_neighbors_pack_mode: the dataset is empty")
    neighbor_hists = hist.cpu().numpy()
    cum_sum = np.cumsum(neighbor_hists.T, axis=0)
    return np.sum(cum_sum < (keep_ratio * cum_sum[hist_n - 1, :]), axis=0)
