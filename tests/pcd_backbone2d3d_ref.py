"""Test-side restatement of the 2D-3D model's point backbone in plain torch (dtype / device generic: float64 for the tests, float32 on the GPU for
tools/pcd_backbone2d3d_time.py), written against the cited lines in our own words, and of the data loader's graph pyramid in numpy float64:

    PointBackbone        EXP/point_backbone.py:8-95 (encoder1_1 .. encoder3_3, decoder2, decoder1, out_proj; the output list reversed)
    KPConv               vision3d/layers/kpconv.py:96-151 (shadow point at +1e6, linear influence, positive-sum neighbour count, bias after it)
    KPConvBlock          kpconv.py:168-207                 KPResidualBlock  kpconv.py:210-280 (bottleneck out/4, strided max-pool shortcut)
    UnaryBlock           vision3d/layers/unary_block.py:7-30 (Linear with bias, GroupNormPackMode, LeakyReLU(0.2) or none)
    GroupNorm groups     vision3d/layers/basic_layers/builder.py:72-86 (at most 32 groups, at least 8 channels per group)
    max-pool             vision3d/ops/pooling.py:6-19      kNN interpolation  vision3d/ops/knn_interpolate.py:43-77 (k = None)
    pyramid              vision3d/array_ops/graph_pyramid.py:9-70 (4 stages, voxel 0.025 doubling, radius 0.0625 doubling)

EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.  The module below has the reference's attribute and parameter names
(110 parameter tensors + 8 kernel-point buffers), so the device path and the reference load the same state dict.

Pyramid (our statement of the loader's; the collate-time code itself stays the reference's CPU code): level 0 = the given float32 points; level i > 0
= the barycentres of the occupied voxels floor(p / (0.025 2^i)) of level i - 1, in ascending voxel-key order, rounded to float32; radius lists in
float64 on those float32 coordinates, the supports with d^2 < r^2 in ascending (d^2, index) order, cut at LIMITS[i] and padded with the support
count (the shadow index), as wide as the longest row up to the limit:
    neighbors[i]   level i in level i,     radius 0.0625 2^i,  limit LIMITS[i]
    subsampling[i] level i+1 in level i,   radius 0.0625 2^i,  limit LIMITS[i]
    upsampling[i]  level i in level i+1,   radius 0.125 2^i,   limit LIMITS[i+1]
Scene "c" (the sparse 600-point scene of tests/partition2d3d_ref.py) is built with two edits the tests need: one point moved 3 m away from the
cloud (a query whose neighbour lists hold one entry: itself), and row 0 of upsampling[0] replaced by shadow entries (an all-shadow interpolation row:
a barycentre pyramid never leaves a point without a coarser point within 2 r, but the reference's code takes any index list).
"""
import math

import numpy as np
import torch
import torch.nn as nn

from tests.partition2d3d_ref import _hash01, make_scene

VOXEL, RADIUS, SIGMA, KERNEL_SIZE = 0.025, 0.0625, 0.05, 15
LIMITS = (40, 36, 36, 36)
NUM_STAGES = 4
INPUT_DIM, OUTPUT_DIM, INIT_DIM = 1, 128, 64
SLOPE = 0.2


# ------------------------------------------------------------------------------------------------------------------------------------------
# graph pyramid (numpy float64)
# ------------------------------------------------------------------------------------------------------------------------------------------
def grid_subsample(points, voxel):
    """barycentres of the occupied voxels, ascending voxel key -> float32"""
    p = points.astype(np.float64)
    keys = np.floor(p / voxel).astype(np.int64)
    _, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    n = int(inv.max()) + 1
    cnt = np.bincount(inv, minlength=n).astype(np.float64)
    bary = np.stack([np.bincount(inv, weights=p[:, k], minlength=n) for k in range(3)], 1) / cnt[:, None]
    return bary.astype(np.float32)


def radius_search(q, s, radius, limit, chunk=1024):
    """[Nq, width] int64: supports with d^2 < r^2, ascending (d^2, index), padded with len(s)"""
    q64, s64 = q.astype(np.float64), s.astype(np.float64)
    Nq, Ns = len(q64), len(s64)
    out = np.full((Nq, limit), Ns, np.int64)
    r2 = radius * radius
    width = 0
    for i0 in range(0, Nq, chunk):
        qq = q64[i0:i0 + chunk]
        d2 = None
        for k in range(3):
            t = qq[:, k, None] - s64[None, :, k]
            d2 = t * t if d2 is None else d2 + t * t
        rows, cols = np.nonzero(d2 < r2)
        dv = d2[rows, cols]
        o = np.lexsort((cols, dv, rows))
        rows, cols = rows[o], cols[o]
        start = np.searchsorted(rows, np.arange(len(qq)))
        rank = np.arange(len(rows)) - start[rows]
        keep = rank < limit
        out[i0 + rows[keep], rank[keep]] = cols[keep]
        if len(rows):
            width = max(width, int(rank.max()) + 1)
    return out[:, :max(1, min(width, limit))]


def build_pyramid(points, edits=False):
    """-> dict(points [4 float32 arrays], neighbors [4], subsampling [3], upsampling [3]) (numpy)"""
    pts = [np.ascontiguousarray(points, dtype=np.float32)]
    for i in range(1, NUM_STAGES):
        pts.append(grid_subsample(pts[-1], VOXEL * 2 ** i))
    nb, sub, up = [], [], []
    r = RADIUS
    for i in range(NUM_STAGES):
        nb.append(radius_search(pts[i], pts[i], r, LIMITS[i]))
        if i < NUM_STAGES - 1:
            sub.append(radius_search(pts[i + 1], pts[i], r, LIMITS[i]))
            up.append(radius_search(pts[i], pts[i + 1], 2 * r, LIMITS[i + 1]))
        r *= 2
    if edits:
        up[0][0, :] = len(pts[1])
    return dict(points=pts, neighbors=nb, subsampling=sub, upsampling=up)


def scene_points(name):
    """level 0 of scene "a" (20 000 points) or "c" (600 points, point 1 moved 3 m along x)"""
    p = make_scene(name)["pcd_points"].numpy().copy()
    if name == "c":
        p[1] = p[1] + np.array([3.0, 0.0, 0.0], dtype=np.float32)
    return p


def make_pyramid(name):
    return build_pyramid(scene_points(name), edits=(name == "c"))


def pyramid_checksum(pyr):
    vals = []
    for k in ("points", "neighbors", "subsampling", "upsampling"):
        for a in pyr[k]:
            vals += [float(a.shape[0]), float(a.shape[1]), float(np.asarray(a, dtype=np.float64).sum())]
    return np.array(vals)


def to_torch(pyr, device="cpu"):
    return {k: [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in v] for k, v in pyr.items()}


# ------------------------------------------------------------------------------------------------------------------------------------------
# the module (the reference's names)
# ------------------------------------------------------------------------------------------------------------------------------------------
def num_groups(C):
    g = 32
    while g > 1 and not (C % g == 0 and C // g >= 8):
        g //= 2
    assert g > 1, C
    return g


def kernel_disposition(radius, index, K=KERNEL_SIZE):
    """the fixture's stand-in for vision3d's load_kernels: the centre plus K-1 points at 0.66 radius, directions from the integer hash of
    (point, index) normalised with sqrt only (exactly rounded: every platform yields the same float32 buffer)"""
    i = np.arange(K - 1)
    v = np.stack([_hash01(3 * i + k, 1000 + index) * 2.0 - 1.0 for k in range(3)], 1)
    v = v / np.sqrt((v * v).sum(1, keepdims=True))
    return np.concatenate([np.zeros((1, 3)), v * (0.66 * radius)], 0).astype(np.float32)


class GroupNormPackMode(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.norm = nn.GroupNorm(num_groups(C), C)

    def forward(self, x):
        return self.norm(x.t().unsqueeze(0)).squeeze(0).t()


def _act(on):
    return nn.LeakyReLU(SLOPE) if on else nn.Identity()


class UnaryBlockPackMode(nn.Module):
    def __init__(self, cin, cout, act=True):
        super().__init__()
        self.mlp = nn.Linear(cin, cout)
        self.norm = GroupNormPackMode(cout)
        self.act = _act(act)

    def forward(self, x):
        return self.act(self.norm(self.mlp(x)))


class KPConv(nn.Module):
    def __init__(self, cin, cout, radius, sigma, index):
        super().__init__()
        self.in_channels, self.out_channels, self.radius, self.sigma, self.groups = cin, cout, radius, sigma, 1
        self.weights = nn.Parameter(torch.zeros(KERNEL_SIZE, cin, cout))
        self.bias = nn.Parameter(torch.zeros(cout))
        self.register_buffer("kernel_points", torch.from_numpy(kernel_disposition(radius, index)))

    def forward(self, q, s, x, inds, counts=None):
        s_pad = torch.cat([s, torch.full_like(s[:1], 1e6)], 0)
        rel = s_pad[inds] - q[:, None, :]                                           # (M, H, 3)
        d2 = ((rel[:, :, None, :] - self.kernel_points) ** 2).sum(3)              # (M, H, K)
        w = torch.clamp(1 - torch.sqrt(d2) / self.sigma, min=0.0).transpose(1, 2)  # (M, K, H)
        nf = torch.cat([x, torch.zeros_like(x[:1])], 0)[inds]                      # (M, H, C)
        y = torch.einsum("mkc,kcd->md", torch.matmul(w, nf), self.weights)
        num = (nf.sum(-1) > 0).sum(-1)
        if counts is not None:
            counts.append(num.clone())
        return y / torch.clamp(num, min=1)[:, None] + self.bias


class KPConvBlock(nn.Module):
    def __init__(self, cin, cout, radius, sigma, index):
        super().__init__()
        self.conv = KPConv(cin, cout, radius, sigma, index)
        self.norm = GroupNormPackMode(cout)
        self.act = _act(True)

    def forward(self, q, s, x, inds, counts=None):
        return self.act(self.norm(self.conv(q, s, x, inds, counts)))


class KPResidualBlock(nn.Module):
    def __init__(self, cin, cout, radius, sigma, index, strided=False):
        super().__init__()
        mid = cout // 4
        self.strided = strided
        self.unary1 = UnaryBlockPackMode(cin, mid)
        self.conv = KPConvBlock(mid, mid, radius, sigma, index)
        self.unary2 = UnaryBlockPackMode(mid, cout, act=False)
        self.unary_shortcut = UnaryBlockPackMode(cin, cout, act=False) if cin != cout else nn.Identity()
        self.act = _act(True)

    def forward(self, q, s, x, inds, counts=None):
        y = self.unary2(self.conv(q, s, self.unary1(x), inds, counts))
        sc = torch.cat([x, torch.zeros_like(x[:1])], 0)[inds].max(1)[0] if self.strided else x
        return self.act(y + self.unary_shortcut(sc))


def knn_interpolate(q, s, x, inds):
    s_pad = torch.cat([s, torch.zeros_like(s[:1])], 0)
    x_pad = torch.cat([x, torch.zeros_like(x[:1])], 0)
    d2 = ((q[:, None, :] - s_pad[inds]) ** 2).sum(-1)
    w = (inds != s.shape[0]).to(x.dtype) / (d2 + 1e-8)
    w = w / (w.sum(1, keepdim=True) + 1e-8)
    return (x_pad[inds] * w[..., None]).sum(1)


class PointBackbone(nn.Module):
    def __init__(self, input_dim=INPUT_DIM, output_dim=OUTPUT_DIM, init_dim=INIT_DIM, radius=RADIUS, sigma=SIGMA):
        super().__init__()
        d, r, s = init_dim, radius, sigma
        self.encoder1_1 = KPConvBlock(input_dim, d, r, s, 0)
        self.encoder1_2 = KPResidualBlock(d, 2 * d, r, s, 1)
        self.encoder2_1 = KPResidualBlock(2 * d, 2 * d, r, s, 2, strided=True)
        self.encoder2_2 = KPResidualBlock(2 * d, 4 * d, 2 * r, 2 * s, 3)
        self.encoder2_3 = KPResidualBlock(4 * d, 4 * d, 2 * r, 2 * s, 4)
        self.encoder3_1 = KPResidualBlock(4 * d, 4 * d, 2 * r, 2 * s, 5, strided=True)
        self.encoder3_2 = KPResidualBlock(4 * d, 8 * d, 4 * r, 4 * s, 6)
        self.encoder3_3 = KPResidualBlock(8 * d, 8 * d, 4 * r, 4 * s, 7)
        self.decoder2 = UnaryBlockPackMode(12 * d, 4 * d)
        self.decoder1 = UnaryBlockPackMode(6 * d, 2 * d)
        self.out_proj = nn.Linear(2 * d, output_dim)

    def forward(self, feats, data_dict, counts=None):
        p, nb, sub, up = data_dict["points"], data_dict["neighbors"], data_dict["subsampling"], data_dict["upsampling"]
        s1 = self.encoder1_1(p[0], p[0], feats, nb[0], counts)
        s1 = self.encoder1_2(p[0], p[0], s1, nb[0], counts)
        s2 = self.encoder2_1(p[1], p[0], s1, sub[0], counts)
        s2 = self.encoder2_2(p[1], p[1], s2, nb[1], counts)
        s2 = self.encoder2_3(p[1], p[1], s2, nb[1], counts)
        s3 = self.encoder3_1(p[2], p[1], s2, sub[1], counts)
        s3 = self.encoder3_2(p[2], p[2], s3, nb[2], counts)
        s3 = self.encoder3_3(p[2], p[2], s3, nb[2], counts)
        l2 = self.decoder2(torch.cat([knn_interpolate(p[1], p[2], s3, up[1]), s2], 1))
        l1 = self.decoder1(torch.cat([knn_interpolate(p[0], p[1], l2, up[0]), s1], 1))
        return [self.out_proj(l1), l2, s3]


# ------------------------------------------------------------------------------------------------------------------------------------------
# weights and loss of the fixture
# ------------------------------------------------------------------------------------------------------------------------------------------
def make_weights(module, seed=5):
    """state dict for any module with the reference's parameter names: parameter p (named_parameters order) drawn from the integer hash with seed
    1000 seed + p, uniform in [-b, b]: KPConv weights b = 1/sqrt(K Cin), Linear weights b = 1/sqrt(in), biases 0.1, GroupNorm gamma 1 +- 0.2,
    beta +- 0.2.  Kernel-point buffers are left as the module holds them."""
    sd = {}
    for p, (name, t) in enumerate(module.named_parameters()):
        u = _hash01(np.arange(t.numel()), 1000 * seed + p).reshape(tuple(t.shape)) * 2.0 - 1.0
        if name.endswith("conv.weights"):
            v = u / math.sqrt(t.shape[0] * t.shape[1])
        elif name.endswith("norm.norm.weight"):
            v = 1.0 + 0.2 * u
        elif name.endswith("norm.norm.bias"):
            v = 0.2 * u
        elif name.endswith("bias"):
            v = 0.1 * u
        else:
            v = u / math.sqrt(t.shape[1])
        sd[name] = torch.from_numpy(v).float()
    return sd


def loss_weights(outs, seed=77):
    """w_i for loss = sum_i <out_i, w_i>: uniform [-1, 1] from the integer hash (numpy float64)"""
    return [_hash01(np.arange(o.numel()), seed + i).reshape(tuple(o.shape)) * 2.0 - 1.0 for i, o in enumerate(outs)]


def loss_of(outs, ws):
    return sum((o * torch.as_tensor(w, dtype=o.dtype, device=o.device)).sum() for o, w in zip(outs, ws))


OUT_ROWS = {"a": 8, "c": 1}      # rows [::n] of the outputs stored per scene
GRAD_STRIDE = 16                 # parameter gradients: [::16, ::16] of a matrix, [::16, ::16, :] of a KPConv weight, all of a vector


def sub_grad(g):
    g = g.detach()
    if g.dim() == 1:
        return g
    return g[::GRAD_STRIDE, ::GRAD_STRIDE]


# outputs are stored quantised: the committed-file limit (1 MiB) does not hold 20 000 / 8 rows x 128 float32 values.  The step is max|out| 2^-18
# (half-step error 1.9e-6 of the tensor's maximum: 2 % of the 1e-4 bar); the float64 column sums of the full outputs carry the 1e-9 check.
QSTEP_BITS = 18


def quantise(x):
    x = np.asarray(x, dtype=np.float64)
    m = float(np.abs(x).max())
    step = m * 2.0 ** -QSTEP_BITS if m > 0 else 1.0
    q = np.ascontiguousarray(np.rint(x / step).astype(np.int32))
    return np.ascontiguousarray(np.moveaxis(q.view(np.uint8).reshape(q.shape + (4,)), -1, 0)), np.array([step])      # byte planes: they compress


def dequantise(planes, step):
    q = np.ascontiguousarray(np.moveaxis(planes, 0, -1)).view(np.int32)[..., 0]
    return q.astype(np.float64) * float(step[0])
