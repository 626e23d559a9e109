"""Test-side restatement of the 2D-3D model's image backbone in plain torch (dtype / device generic: float64 for the tests, float32 on the GPU as
the timing baseline of tools/image_backbone2d3d_time.py), written against the cited lines in our own words:

    ImageBackbone   EXP/image_backbone.py:69-289   (encoder1 .. encoder4, the lateral 1 x 1 convs, the three-stage decoder, out_proj; the DINO
                                                    grid resampled onto the stage-4 map; the output list finest first)
    BasicBlock      EXP/image_backbone.py:9-66     (conv1 with activation, conv2 without, the strided identity a ConvBlock of its own)
    ConvBlock       vision3d/layers/conv_block.py:10-125 (Conv2d with bias -> GroupNorm or nothing -> LeakyReLU(0.2) or nothing)
    GroupNorm rule  vision3d/layers/basic_layers/builder.py:72-86 (at most 32 groups, at least 8 channels per group)

EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.  The modules below carry the reference's attribute and parameter names, so
the reference, this restatement and the device path load one state dict.  No weights are stored: make_weights draws them from a seeded generator.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

SLOPE = 0.2

# the fixture's cases (tests/golden/image_backbone2d3d.npz): 16 base channels, the smallest width the GroupNorm rule admits (16 / 32 / 64 -> G = 2 / 4 / 8)
CASES = {
    "a": dict(image=(24, 32), dino=(2, 3), base=16, out=16, seed=11),      # a true resample of the DINO grid onto the 3 x 4 stage-4 map
    "b": dict(image=(21, 27), dino=(2, 3), base=16, out=16, seed=12),      # odd sizes everywhere: 11 x 14, 6 x 7, 3 x 4; 11 x 14 -> 21 x 27 upsampling
    "c": dict(image=(24, 32), dino=(3, 4), base=16, out=24, seed=13),      # the identity resample
}
REAL = dict(image=(48, 64), dino=(4, 5), base=128, out=128, seed=21)       # the production widths: K up to 4 608, Cout up to 512
PRODUCTION = dict(image=(480, 640), dino=(34, 45), base=128, out=128, seed=31)

# the conv primitive's cases: (k, stride, padding, dilation, Cin, Cout, H, W)
CONV_CASES = {
    "edge_5x7": (3, 1, 1, 1, 16, 16, 5, 7),            # every pixel touches the padding, below one tile
    "stride2": (3, 2, 1, 1, 16, 32, 21, 27),
    "stem_c1": (7, 2, 3, 1, 1, 16, 21, 27),            # direct path
    "stem_c3": (7, 2, 3, 1, 3, 16, 21, 27),            # direct path
    "pointwise": (1, 1, 0, 1, 64, 64, 3, 4),
    "dilated": (3, 1, 2, 2, 16, 16, 9, 9),
    "ragged": (3, 1, 1, 1, 20, 160, 13, 11),           # pixels and Cout ragged over more than one tile, Cin no multiple of the k-chunk
    "one_pixel": (3, 1, 1, 1, 16, 16, 1, 1),
    "large_tile": (3, 1, 1, 1, 128, 16, 240, 280),     # 525 tiles of 128 x 128 and K = 1 152 > 1 024: the large-tile kernel, ragged in both
}
RESIZE_CASES = {"up_3x4": ((3, 4), (6, 7)), "up_11x14": ((11, 14), (21, 27)), "identity": ((6, 7), (6, 7)), "one_texel": ((1, 1), (5, 3))}


def num_groups(channels):
    """the largest power of two <= 32 that divides `channels` and leaves at least 8 channels per group"""
    g = 32
    while g > 1 and (channels % g or channels // g < 8):
        g //= 2
    if g == 1:
        raise ValueError("no GroupNorm grouping for %d channels" % channels)
    return g


class ConvBlock(nn.Module):
    def __init__(self, cin, cout, k, stride=1, padding=0, dilation=1, norm=False, act=False):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=padding, dilation=dilation, bias=True)
        self.norm = nn.GroupNorm(num_groups(cout), cout) if norm else nn.Identity()
        self.act = nn.LeakyReLU(SLOPE) if act else nn.Identity()

    def forward(self, x):
        return self.act(self.norm(self.conv(x)))


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride=1, dilation=1):
        super().__init__()
        self.conv1 = ConvBlock(cin, cout, 3, stride, 1, dilation, norm=True, act=True)
        self.conv2 = ConvBlock(cout, cout, 3, 1, 1, dilation, norm=True)
        self.identity = nn.Identity() if stride == 1 else ConvBlock(cin, cout, 3, stride, 1, dilation, norm=True)
        self.act = nn.LeakyReLU(SLOPE)

    def forward(self, x):
        return self.act(self.identity(x) + self.conv2(self.conv1(x)))


def _up(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=True)


class ImageBackbone(nn.Module):
    def __init__(self, in_channels, out_channels, base, dilation=1):
        super().__init__()
        b = base
        self.encoder1 = ConvBlock(in_channels, b, 7, 2, 3, norm=True, act=True)
        self.encoder2 = nn.Sequential(BasicBlock(b, b, 1, dilation), BasicBlock(b, b, 1, dilation))
        self.encoder3 = nn.Sequential(BasicBlock(b, 2 * b, 2, dilation), BasicBlock(2 * b, 2 * b, 1, dilation))
        self.encoder4 = nn.Sequential(BasicBlock(2 * b, 4 * b, 2, dilation), BasicBlock(4 * b, 4 * b, 1, dilation))
        self.decoder4_1 = ConvBlock(4 * b, 4 * b, 1)
        self.decoder3_1 = ConvBlock(2 * b, 4 * b, 1)
        self.decoder3_2 = nn.Sequential(ConvBlock(4 * b, 4 * b, 3, 1, 1, norm=True, act=True), ConvBlock(4 * b, 2 * b, 3, 1, 1))
        self.decoder2_1 = ConvBlock(b, 2 * b, 1)
        self.decoder2_2 = nn.Sequential(ConvBlock(2 * b, 2 * b, 3, 1, 1, norm=True, act=True), ConvBlock(2 * b, b, 3, 1, 1))
        self.decoder1_1 = ConvBlock(b, b, 1)
        self.decoder1_2 = nn.Sequential(ConvBlock(b, b, 3, 1, 1, norm=True, act=True), ConvBlock(b, b, 3, 1, 1))
        self.out_proj = ConvBlock(b, out_channels, 1)

    def forward(self, x, dino_feat=None):
        s1 = self.encoder1(x)
        s2 = self.encoder2(s1)
        s3 = self.encoder3(s2)
        s4 = self.encoder4(s3)
        l4 = self.decoder4_1(s4 + _up(dino_feat.permute(0, 3, 1, 2).contiguous(), s4.shape[2:]))
        l3 = self.decoder3_2(self.decoder3_1(s3) + _up(l4, s3.shape[2:]))
        l2 = self.decoder2_2(self.decoder2_1(s2) + _up(l3, s2.shape[2:]))
        l1 = self.decoder1_2(_up(self.decoder1_1(s1) + l2, x.shape[2:]))
        return [self.out_proj(l1), l2, l3, l4]


def build(case, dtype=torch.float32, device="cpu"):
    """the restatement's module for a case of the table, weights from make_weights"""
    m = ImageBackbone(1, case["out"], case["base"])
    m.load_state_dict(make_weights(m, case["seed"]))
    return m.to(device=device, dtype=dtype).eval()


def make_weights(module, seed, device="cpu"):
    """state dict for `module` (the reference's ImageBackbone or the restatement: same names, same order), drawn from a generator seeded with
    `seed` on `device`: conv weights uniform with variance 1 / fan_in, GroupNorm gamma in 1 +- 0.2, every bias in +- 0.1"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    u = lambda shape: torch.rand(shape, generator=g, device=device, dtype=torch.float32) * 2.0 - 1.0
    sd = {}
    for name, p in module.named_parameters():
        if name.endswith("conv.weight"):
            fan_in = p.shape[1] * p.shape[2] * p.shape[3]
            sd[name] = u(tuple(p.shape)) * (3.0 / fan_in) ** 0.5
        elif name.endswith("norm.weight"):
            sd[name] = 1.0 + 0.2 * u(tuple(p.shape))
        elif name.endswith(".bias"):
            sd[name] = 0.1 * u(tuple(p.shape))
        else:
            raise KeyError(name)
    return sd


def make_inputs(case, device="cpu"):
    """(x [1, 1, H, W] gray image in [0, 1), dino_feat [1, h, w, 4 base] unit normal), float32, from the case's seed"""
    g = torch.Generator(device=device)
    g.manual_seed(case["seed"] + 1000)
    H, W = case["image"]
    h, w = case["dino"]
    x = torch.rand((1, 1, H, W), generator=g, device=device, dtype=torch.float32)
    dino = torch.randn((1, h, w, 4 * case["base"]), generator=g, device=device, dtype=torch.float32)
    return x, dino


def rel_dev(a, ref):
    """the error measure of every check here: max|a - ref| / max|ref|"""
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max() / ref.abs().max())
