"""The 2D-3D dataset item on the device: what SevenScenes2D3DHardPairDataset.__getitem__ / RGBDScenes2D3DHardPairDataset.__getitem__ compute
behind their file reads (2D-3D vision3d/datasets/registration/sevenscenes/sevenscenes_hard.py:128-206, rgbdscenes/rgbdscenes.py), with the
reference's names:

    get_2d3d_correspondences_mutual, get_2d3d_correspondences_radius      vision3d/array_ops/registration_utils.py:30-60, 63-89
    prepare_item                                                           the body of __getitem__ from `data_dict["image_h"]` on

The correspondences run on dr_corr_2d3d_mutual_f64 / dr_corr_2d3d_radius_f64 / dr_overlap_2d3d_f64 (csrc/item2d3d.hip) in float64; there is no
CPU path.  The two functions read ONE 4-byte word back, for the data-dependent length of their result; prepare_item reads once per list it returns.
The point selection, the small transform about the centroid, the composed transform and the uniform noise are a few tiny torch float64 operations
on the device.  Differences a maintainer should know: equal distances go to the lowest index; np.random's draws
cannot be reproduced, so they are passed in or drawn from a torch generator; scale augmentation is refused; where the reference raises on an
empty pair list (registration_utils.py:24-25) the result is the empty list."""
import math

import torch

from . import lib


def correspondences(depth_img, pcd_points, intrinsic, transform, matching_radius_2d, matching_radius_3d, depth_limit=6.0,
                    method="mutual_nearest", cap=None):
    """both variants with the room for the result in the caller's hand: -> (img_corr_pixels [C, 2] int64, pcd_corr_indices [C] int64).  cap =
    rows of room: None takes min(H W, N) for the mutual variant (always enough) and counts first for the radius variant (a launch sequence
    with room for none; the read of its count is the only one).  More rows found than `cap` raises; nothing is written behind the room given.
    ONE 4-byte host read: the number found."""
    args = (depth_img, pcd_points, intrinsic, transform, matching_radius_2d, matching_radius_3d, depth_limit)
    if cap is None and method == "radius":
        _, _, counts = lib.corr_2d3d(*args, method=method, cap=0)
        found = int(counts[1].item())
        if found >= 2 ** 31 - 1:
            raise RuntimeError("get_2d3d_correspondences_radius: 2^31 - 1 pairs or more")
        pix, idx, _ = lib.corr_2d3d(*args, method=method, cap=found)
        return pix, idx
    pix, idx, counts = lib.corr_2d3d(*args, method=method, cap=cap)
    found = int(counts[1].item())
    if found > pix.shape[0]:
        raise RuntimeError("2D-3D correspondences (%s): %d pairs found, room for %d" % (method, found, pix.shape[0]))
    return pix[:found], idx[:found]


def get_2d3d_correspondences_mutual(depth_img, pcd_points, intrinsic, transform, matching_radius_2d, matching_radius_3d, depth_limit=6.0):
    """-> (img_corr_pixels [C, 2] int64 (h, w), pcd_corr_indices [C] int64) on depth_img's device: the mutually nearest (pixel, point) pairs that
    are closer than matching_radius_3d in space and than matching_radius_2d on the image, in ascending pixel order."""
    return correspondences(depth_img, pcd_points, intrinsic, transform, matching_radius_2d, matching_radius_3d, depth_limit, "mutual_nearest")


def get_2d3d_correspondences_radius(depth_img, pcd_points, intrinsic, transform, matching_radius_2d, matching_radius_3d, depth_limit=6.0):
    """-> (img_corr_pixels [C, 2] int64 (h, w), pcd_corr_indices [C] int64): every (pixel, point) pair inside both radii, in ascending (pixel,
    point) order."""
    return correspondences(depth_img, pcd_points, intrinsic, transform, matching_radius_2d, matching_radius_3d, depth_limit, "radius")


def get_2d3d_overlap_indices(depth_img, pcd_points, intrinsic, transform, matching_radius_2d, matching_radius_3d, depth_limit=6.0):
    """-> (img_overlap_indices int64, pcd_overlap_indices int64): np.unique of the radius variant's pixel indices h W + w and point indices
    (sevenscenes_hard.py:185-190) without the pair list; one host read"""
    img, pcd, counts = lib.overlap_2d3d(depth_img, pcd_points, intrinsic, transform, matching_radius_2d, matching_radius_3d, depth_limit)
    c = counts.tolist()                       # one read for both lengths
    return img[:c[1]], pcd[:c[3]]


def random_small_transform(generator=None, device="cuda", scale=0.1):
    """random_sample_small_transform (vision3d/array_ops/point_cloud_utils.py:246-261) from a torch generator -> [4, 4] float64 on the device
    (an axis uniform on the sphere, an angle in [0, scale pi / sqrt 3), a normal translation of deviation scale / sqrt 3)"""
    draw = lambda f, *s: f(*s, generator=generator, dtype=torch.float64, device=generator.device if generator is not None else device).to(device)
    axis = draw(torch.randn, 3)
    axis = axis / axis.norm()
    theta = draw(torch.rand, 1) * scale * math.pi / math.sqrt(3.0)
    zero = torch.zeros((), dtype=torch.float64, device=device)
    K = torch.stack([zero, -axis[2], axis[1], axis[2], zero, -axis[0], -axis[1], axis[0], zero]).view(3, 3)
    T = torch.eye(4, dtype=torch.float64, device=device)
    T[:3, :3] = torch.eye(3, dtype=torch.float64, device=device) + torch.sin(theta) * K + (1.0 - torch.cos(theta)) * (K @ K)
    T[:3, 3] = draw(torch.randn, 3) * scale / math.sqrt(3.0)
    return T


_META = ("scene_name", "image_file", "depth_file", "cloud_file", "overlap", "image_id", "cloud_id")


def prepare_item(raw, *, max_points, use_augmentation, augmentation_noise, return_corr_indices, matching_method, matching_radius_2d,
                 matching_radius_3d, return_overlap_indices, scale_augmentation=False, mean_key="image", device="cuda", crop=None,
                 generator=None, aug_transform=None, noise=None, sel_indices=None):
    """the reference's data_dict (same keys, dtypes and shapes) as device tensors, from `raw` = what the dataset holds after its file reads:
    depth [H, W], image [H, W, 3], image_gray [H, W], ori_image [H, W, 3], points [n, 3], intrinsics [3, 3], cloud_to_image [4, 4] (numpy or
    torch) and the metadata entries (scene_name, image_file, depth_file, cloud_file, overlap, image_id, cloud_id: passed through).
    crop = (height, width): the reference's topleft_crop of the four images (476 x 630 there).  mean_key: the image whose mean is removed --
    "image" (7Scenes, sevenscenes_hard.py:167) or "image_gray" (RGB-D Scenes).
    The draws np.random makes in the reference are arguments: sel_indices [max_points] int64 (the head of a permutation), aug_transform [4, 4]
    (random_sample_small_transform), noise [n, 3] uniform in [0, 1) (np.random.rand); those not passed are drawn from `generator`."""
    if scale_augmentation:
        raise NotImplementedError("prepare_item: scale augmentation needs cv2.resize (INTER_LINEAR) of the image and the depth, which is not "
                                  "restated here; neither 2D-3D experiment turns it on")
    if matching_method not in ("mutual_nearest", "radius"):
        raise ValueError("Bad matching method: %s" % matching_method)
    if mean_key not in ("image", "image_gray"):
        raise ValueError("prepare_item: mean_key is 'image' or 'image_gray'")
    f64 = lambda a: torch.as_tensor(a).to(device=device, dtype=torch.float64)
    out = {k: raw[k] for k in _META if k in raw}
    imgs = {k: torch.as_tensor(raw[k]).to(device) for k in ("depth", "image", "image_gray", "ori_image")}
    if crop is not None:
        ch, cw = crop
        if imgs["image"].shape[0] < ch or imgs["image"].shape[1] < cw:
            raise ValueError("Crop size exceeds image dimensions!")
        imgs = {k: v[:ch, :cw] for k, v in imgs.items()}
    H, W = imgs["image"].shape[:2]
    out["image_h"], out["image_w"] = H, W
    intrinsics, transform = f64(raw["intrinsics"]).reshape(3, 3), f64(raw["cloud_to_image"]).reshape(4, 4)
    points = torch.as_tensor(raw["points"]).to(device)
    gen_dev = generator.device if generator is not None else device
    if max_points is not None and points.shape[0] > max_points:
        if sel_indices is None:
            sel_indices = torch.randperm(points.shape[0], generator=generator, device=gen_dev)[:max_points]
        points = points[torch.as_tensor(sel_indices).to(device=device, dtype=torch.int64)]
    if use_augmentation:
        if aug_transform is None:
            aug_transform = random_small_transform(generator, device)
        if noise is None:
            noise = torch.rand(points.shape[0], 3, generator=generator, dtype=torch.float64, device=gen_dev)
        # numpy adds the rows of a float32 cloud one after the other; a float64 cloud's mean is insensitive to the order at float32 precision
        center = (lib.column_mean_seq(points) if points.dtype == torch.float32 else points.mean(dim=0)).to(torch.float64)
        eye = torch.eye(4, dtype=torch.float64, device=device)
        sub, add = eye.clone(), eye.clone()
        sub[:3, 3], add[:3, 3] = -center, center
        aug = add @ (f64(aug_transform) @ sub)                                   # compose_transforms(subtract_center, aug, add_center)
        points = points.to(torch.float64) @ aug[:3, :3].T + aug[:3, 3]           # apply_transform: float64 from here on
        inv = eye.clone()
        inv[:3, :3] = aug[:3, :3].T
        inv[:3, 3] = -(aug[:3, :3].T @ aug[:3, 3])
        transform = transform @ inv                                              # compose_transforms(inverse_transform(aug), transform)
        points = points + (f64(noise) - 0.5) * augmentation_noise
    centred = imgs[mean_key]
    imgs[mean_key] = centred - centred.mean(dtype=torch.float64).to(centred.dtype) if centred.is_floating_point() else centred - centred.double().mean()
    depth32 = imgs["depth"].to(torch.float32).contiguous()
    args = (depth32, points, intrinsics, transform, matching_radius_2d, matching_radius_3d)
    if return_corr_indices:
        pix, idx = (get_2d3d_correspondences_mutual if matching_method == "mutual_nearest" else get_2d3d_correspondences_radius)(*args)
        out["img_corr_pixels"], out["img_corr_indices"], out["pcd_corr_indices"] = pix, pix[:, 0] * W + pix[:, 1], idx
    if return_overlap_indices:
        io, po = get_2d3d_overlap_indices(*args)
        out["img_overlap_pixels"] = torch.stack([io // W, io % W], dim=1)
        out["img_overlap_indices"], out["pcd_overlap_indices"] = io, po
    out["intrinsics"] = intrinsics.to(torch.float32)
    out["transform"] = transform.to(torch.float32)
    for k in ("image", "depth", "image_gray", "ori_image"):
        out[k] = imgs[k].to(torch.float32)
    out["points"] = points.to(torch.float32)
    out["feats"] = torch.ones(points.shape[0], 1, dtype=torch.float32, device=device)
    return out
