"""The geometry head and the feature-layout glue of MATR2D3D.forward on the device (csrc/front2d3d.hip, ABI 0.7.0, second set).

`back_project`, `render` and `create_meshgrid` keep vision3d.ops' names, argument orders, defaults and return shapes / dtypes
(ops/back_project.py, ops/render.py, ops/meshgrid.py); `back_project_depth` is MATR2D3D.back_project_depth (EXP/model.py:852-901) without `self`.
One image per call runs in libdiffreg_hip; what the kernels do not cover (a batch larger than 1, render's rounding=True, a dtype other than
float32, a normalised / centred meshgrid) runs the same definition in torch INSIDE this module -- never the reference's code.

    img_points, img_masks = back_project(depth, intrinsics, depth_limit=6.0, transposed=True, return_mask=True)     # EXP/model.py:306
    pcd_pixels_f = render(pcd_points_f, intrinsics, extrinsics=transform, rounding=False)                           # :335

The two layout calls of forward are inline `F.` code; they become one call each:

    img_feats_c = resize_tokens(img_feats_x, img_shape_c)       # :374-375  F.interpolate(bilinear, align_corners=True) + view + transpose
    img_feats_f = rows_normalized(img_feats_f)                  # :535-538  view + transpose + contiguous + F.normalize(p=2, dim=1)

Both are autograd functions whose forward and backward are library calls.  `rows_normalized(feats, rows=idx)` is the form for a consumer that
reads K rows only (the fine loss: at most 1 024 of 307 200): it returns `(full, picked)` -- `full` [H*W, C] carries no gradient, `picked` =
full[idx] [K, C] does, and its backward hands the K gradient rows straight to the sparse kernel (repeats in idx accumulate), so no dense
[H*W, C] gradient is ever built.  (The `rows=` argument rather than a handle object: one function, one extra return value.)
"""
import torch

from . import lib


def _is_f32_cuda(*ts):
    return all(t is None or (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32) for t in ts)


# ---- torch statements of the same definitions: the argument combinations the kernels do not cover ------------------------------------------
def _back_project_torch(depth_mat, intrinsics, z_of, depth_limit, transposed, return_mask):
    focal_x, focal_y = intrinsics[..., 0:1, 0:1], intrinsics[..., 1:2, 1:2]
    center_x, center_y = intrinsics[..., 0:1, 2:3], intrinsics[..., 1:2, 2:3]
    _, height, width = depth_mat.shape
    coords = torch.arange(height * width, device=depth_mat.device).view(height, width).unsqueeze(0).expand_as(depth_mat)
    u, v = coords % width, torch.div(coords, width, rounding_mode="floor")
    z = z_of(depth_mat)
    if depth_limit is not None:
        z = z.masked_fill(torch.gt(z, depth_limit), 0.0)
    x, y = (u - center_x) * z / focal_x, (v - center_y) * z / focal_y
    points = torch.stack([x, y, z], dim=-1 if transposed else 1)
    return (points, torch.gt(z, 0.0)) if return_mask else points


def _back_project(depth_mat, intrinsics, mode, a, b, z_of, depth_limit, transposed, return_mask):
    if depth_mat.dim() != 3:
        raise ValueError("depth_mat is (B, H, W) (got %s)" % (tuple(depth_mat.shape),))
    B, H, W = depth_mat.shape
    if B != 1 or intrinsics.numel() != 9 or not _is_f32_cuda(depth_mat, intrinsics):
        return _back_project_torch(depth_mat, intrinsics, z_of, depth_limit, transposed, return_mask)
    pts, mask, _ = lib.back_project_points(depth_mat[0], intrinsics.reshape(3, 3), mode=mode, a=a, b=b, depth_limit=depth_limit)
    points = pts.view(1, H, W, 3)
    if not transposed:
        points = points.permute(0, 3, 1, 2).contiguous()
    return (points, mask.view(1, H, W).bool()) if return_mask else points


def back_project(depth_mat, intrinsics, scaling_factor=1000.0, depth_limit=None, transposed=False, return_mask=False):
    """vision3d.ops.back_project: depth (B, H, W), intrinsics (B, 3, 3) -> points (B, 3, H, W) or (B, H, W, 3) (+ bool masks (B, H, W))"""
    if torch.is_tensor(scaling_factor):          # the kernel's mode 0 divides by a host number
        return _back_project_torch(depth_mat, intrinsics, lambda d: d / scaling_factor, depth_limit, transposed, return_mask)
    return _back_project(depth_mat, intrinsics, 0, scaling_factor, 0.0, lambda d: d / scaling_factor, depth_limit, transposed, return_mask)


def back_project_depth(depth_mat, intrinsics, scaling_factor_a=1000.0, scaling_factor_b=1000.0, depth_limit=None, transposed=False,
                       return_mask=False):
    """MATR2D3D.back_project_depth: z = depth * scaling_factor_a + scaling_factor_b; the two factors are numbers or (device) tensors of one
    element, read by the kernel from device memory"""
    one = lambda s: not torch.is_tensor(s) or s.numel() == 1
    z_of = lambda d: d * scaling_factor_a + scaling_factor_b
    if not (one(scaling_factor_a) and one(scaling_factor_b)):
        return _back_project_torch(depth_mat, intrinsics, z_of, depth_limit, transposed, return_mask)
    return _back_project(depth_mat, intrinsics, 1, scaling_factor_a, scaling_factor_b, z_of, depth_limit, transposed, return_mask)


def _apply_transform(points, transform):
    if transform.dim() == 2:
        shape = points.shape
        return (torch.matmul(points.reshape(-1, 3), transform[:3, :3].transpose(-1, -2)) + transform[None, :3, 3]).reshape(*shape)
    if points.dim() == 3:
        return torch.matmul(points, transform[:, :3, :3].transpose(-1, -2)) + transform[:, None, :3, 3]
    return (torch.matmul(points.unsqueeze(1), transform[:, :3, :3].transpose(-1, -2)) + transform[:, None, :3, 3]).squeeze(1)


def _render_torch(points, intrinsics, extrinsics, rounding, return_depth, eps):
    if extrinsics is not None:
        points = _apply_transform(points, extrinsics)
    x, y, z = points[..., 0], points[..., 1], points[..., 2]
    focal_x, focal_y = intrinsics[..., 0, 0].unsqueeze(-1), intrinsics[..., 1, 1].unsqueeze(-1)
    center_x, center_y = intrinsics[..., 0, 2].unsqueeze(-1), intrinsics[..., 1, 2].unsqueeze(-1)
    w = focal_x * x / z.clamp(min=eps) + center_x
    h = focal_y * y / z.clamp(min=eps) + center_y
    if rounding:
        w, h = w.long(), h.long()
    pixels = torch.stack([h, w], dim=-1)
    return (pixels, z) if return_depth else pixels


def render(points, intrinsics, extrinsics=None, rounding=True, return_depth=False, eps=1e-8):
    """vision3d.ops.render: points (N, 3) or (B, N, 3) -> pixels (h, w) of the same leading shape (+ depth)"""
    assert points.dim() == intrinsics.dim()
    if extrinsics is not None:
        assert points.dim() == extrinsics.dim()
    single = points.dim() == 2 or (points.dim() == 3 and points.shape[0] == 1 and intrinsics.shape[0] == 1
                                   and (extrinsics is None or extrinsics.shape[0] == 1))
    if rounding or not single or points.shape[-1] != 3 or not _is_f32_cuda(points, intrinsics, extrinsics):
        return _render_torch(points, intrinsics, extrinsics, rounding, return_depth, eps)
    lead = points.shape[:-1]
    out = lib.render_points(points.reshape(-1, 3), intrinsics.reshape(3, 3), None if extrinsics is None else extrinsics.reshape(4, 4), eps=eps,
                            return_depth=return_depth)
    if return_depth:
        return out[0].view(*lead, 2), out[1].view(*lead)
    return out.view(*lead, 2)


def create_meshgrid(height, width, normalized=False, flatten=False, centering=False, device="cuda"):
    """vision3d.ops.create_meshgrid: cartesian_prod of the row and column values -> (H, W, 2), or (H*W, 2) when flatten.  int64 from
    torch.arange when neither normalised nor centred; torch.linspace(0, 1, steps) values when normalised without centring; float otherwise.
    (The float32 form forward() takes with `.float()` is also an output of dr_back_project_f32: lib.back_project_points(..., pixels=True).)"""
    if normalized and not centering:
        h_values = torch.linspace(0.0, 1.0, steps=height).to(device)
        w_values = torch.linspace(0.0, 1.0, steps=width).to(device)
    else:
        h_values, w_values = torch.arange(height).to(device), torch.arange(width).to(device)
        if centering:
            h_values, w_values = h_values.float() + 0.5, w_values.float() + 0.5
        if normalized:
            h_values, w_values = h_values.float() / float(height), w_values.float() / float(width)
    pixels = torch.cartesian_prod(h_values, w_values)
    return pixels if flatten else pixels.view(height, width, 2)


# ---- the two layout calls ------------------------------------------------------------------------------------------------------------------
def _chw(feats):
    """(1, C, H, W) or (C, H, W) -> (C, H, W)"""
    if feats.dim() == 4:
        if feats.shape[0] != 1:
            raise ValueError("one image per call: the batch dimension is 1 (got %s)" % (tuple(feats.shape),))
        return feats[0]
    if feats.dim() != 3:
        raise ValueError("feats is (1, C, H, W) or (C, H, W) (got %s)" % (tuple(feats.shape),))
    return feats


class _ResizeTokens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, size):
        ctx.src_shape, ctx.size = tuple(feats.shape), size
        return lib.resize_tokens(feats, size)

    @staticmethod
    def backward(ctx, grad):
        return lib.resize_tokens_backward(grad, ctx.src_shape, ctx.size), None


def resize_tokens(feats_nchw, size):
    """F.interpolate(feats, size, mode="bilinear", align_corners=True).squeeze(0).view(C, -1).transpose(0, 1), contiguous: [Hd*Wd, C]"""
    x = _chw(feats_nchw)
    return _ResizeTokens.apply(x.float(), (int(size[0]), int(size[1])))


class _RowsNormalized(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return lib.rows_normalize_chw(x)

    @staticmethod
    def backward(ctx, grad):
        (x,) = ctx.saved_tensors
        return lib.rows_normalize_chw_backward(x, grad)


class _RowsNormalizedPicked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rows):
        full = lib.rows_normalize_chw(x)
        ctx.save_for_backward(x, rows)
        ctx.mark_non_differentiable(full)
        return full, full.index_select(0, rows)

    @staticmethod
    def backward(ctx, _grad_full, grad_picked):
        x, rows = ctx.saved_tensors
        return lib.rows_normalize_chw_backward(x, grad_picked, rows=rows), None


def rows_normalized(feats_nchw, rows=None):
    """F.normalize(feats.squeeze(0).view(C, -1).transpose(0, 1).contiguous(), p=2, dim=1): [H*W, C].  With rows (int64 [K], repeats allowed):
    -> (full [H*W, C] without gradient, full[rows] [K, C] whose backward is the sparse kernel) -- see the module docstring.  C <= 256."""
    x = _chw(feats_nchw)
    x = x.float().reshape(x.shape[0], -1)
    if rows is None:
        return _RowsNormalized.apply(x)
    return _RowsNormalizedPicked.apply(x, torch.as_tensor(rows).to(device=x.device, dtype=torch.int64).reshape(-1))
