"""Plain-torch restatement of Depth-Anything's decoder, DPTHead (depth_anything/dpt.py:22-136; ResidualConvUnit and FeatureFusionBlock,
depth_anything/blocks.py), written from its description: the float64 yardstick for shapes the fixture lacks and the module the GPU tests bind (the
reference itself is not needed to run them).  The modules carry the reference's attribute and parameter names, so the reference, this
restatement and the device path load one state dict.  Also here: the fixture's cases, the weight drawing by parameter name, the input drawing,
the recorder of the named intermediates and the fixture's reader / writer (tests/golden/dpt2d3d_*.npz; minted by
tools/golden/make_golden_dpt2d3d.py from the reference's own DPTHead).
"""
import glob
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

# the fixture's head: small widths, every channel count a multiple of 4
SMALL = dict(in_channels=128, features=32, out_channels=[16, 32, 64, 64])
# the patch grids (those of the ViT fixture's images): the odd ones give ceil(h / 2) layers whose resample back up is not x 2; 10 x 13 gives
# 40 x 52 = 2 080 pixels at layer_1, not a multiple of 64
GRIDS = {"3x5": (3, 5), "5x5": (5, 5), "10x13": (10, 13)}
WEIGHT_SEED = 41
# the model's geometry (EXP/model.py:176-190: 476 x 630 -> a 34 x 45 grid of width 1 024)
PRODUCTION = dict(in_channels=1024, features=256, out_channels=[256, 512, 1024, 1024], grid=(34, 45))
NAMES = ("layer_1", "layer_2", "layer_3", "layer_4", "path_4", "path_3", "path_2", "path_1", "output_conv1", "out")
FILE_LIMIT = 1 << 20


class ResidualConvUnit(nn.Module):
    """pre-activation residual unit: conv2(act(conv1(act(x)))) + x, the activation not in place"""

    def __init__(self, features, activation):
        super().__init__()
        self.conv1 = nn.Conv2d(features, features, 3, padding=1)
        self.conv2 = nn.Conv2d(features, features, 3, padding=1)
        self.activation = activation

    def forward(self, x):
        y = self.conv1(self.activation(x))
        y = self.conv2(self.activation(y))
        return y + x


class FeatureFusionBlock(nn.Module):
    def __init__(self, features):
        super().__init__()
        self.out_conv = nn.Conv2d(features, features, 1)
        self.resConfUnit1 = ResidualConvUnit(features, nn.ReLU(False))
        self.resConfUnit2 = ResidualConvUnit(features, nn.ReLU(False))

    def forward(self, *xs, size=None):
        y = xs[0]
        if len(xs) == 2:
            y = y + self.resConfUnit1(xs[1])
        y = self.resConfUnit2(y)
        how = dict(scale_factor=2) if size is None else dict(size=size)
        y = F.interpolate(y, mode="bilinear", align_corners=True, **how)
        return self.out_conv(y)


class DPTHead(nn.Module):
    def __init__(self, in_channels, features=256, out_channels=(256, 512, 1024, 1024)):
        super().__init__()
        oc = list(out_channels)
        self.nclass, self.use_clstoken = 1, False
        self.projects = nn.ModuleList([nn.Conv2d(in_channels, c, 1) for c in oc])
        self.resize_layers = nn.ModuleList([nn.ConvTranspose2d(oc[0], oc[0], 4, stride=4), nn.ConvTranspose2d(oc[1], oc[1], 2, stride=2),
                                            nn.Identity(), nn.Conv2d(oc[3], oc[3], 3, stride=2, padding=1)])
        s = self.scratch = nn.Module()
        for i in range(4):
            setattr(s, "layer%d_rn" % (i + 1), nn.Conv2d(oc[i], features, 3, padding=1, bias=False))
        s.stem_transpose = None
        for i in (1, 2, 3, 4):
            setattr(s, "refinenet%d" % i, FeatureFusionBlock(features))
        s.output_conv1 = nn.Conv2d(features, features // 2, 3, padding=1)
        s.output_conv2 = nn.Sequential(nn.Conv2d(features // 2, 32, 3, padding=1), nn.ReLU(True), nn.Conv2d(32, 1, 1), nn.ReLU(True), nn.Identity())

    def forward(self, out_features, patch_h, patch_w):
        layers = []
        for i, feat in enumerate(out_features):
            x = feat[0]
            x = x.permute(0, 2, 1).reshape(x.shape[0], x.shape[-1], patch_h, patch_w)
            layers.append(self.resize_layers[i](self.projects[i](x)))
        s = self.scratch
        rn = [getattr(s, "layer%d_rn" % (i + 1))(layers[i]) for i in range(4)]
        p = s.refinenet4(rn[3], size=rn[2].shape[2:])
        p = s.refinenet3(p, rn[2], size=rn[1].shape[2:])
        p = s.refinenet2(p, rn[1], size=rn[0].shape[2:])
        p = s.refinenet1(p, rn[0])
        y = s.output_conv1(p)
        y = F.interpolate(y, (14 * int(patch_h), 14 * int(patch_w)), mode="bilinear", align_corners=True)
        return s.output_conv2(y)


def small_head(dtype=torch.float32, device="cpu", weights=None):
    """the fixture's head; weights: a state dict (the fixture's), or None for draw_weights(WEIGHT_SEED)"""
    m = DPTHead(SMALL["in_channels"], SMALL["features"], SMALL["out_channels"])
    m.load_state_dict(draw_weights(m, WEIGHT_SEED) if weights is None else weights)
    return m.to(device=device, dtype=dtype).eval()


def draw_weights(module, seed, device="cpu"):
    """state dict for `module` (the reference's DPTHead or the restatement: same names, same order) from a generator seeded with `seed`: by
    parameter name, a weight uniform with variance 1 / (terms per output element) -- the scale at which a trained checkpoint keeps activations of
    order one through the depth of the decoder -- and a bias uniform in +- [0.05, 0.15]: away from zero, either sign"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    u = lambda shape: torch.rand(shape, generator=g, device=device, dtype=torch.float32) * 2.0 - 1.0
    sd = {}
    for name, p in module.state_dict().items():
        if name.endswith(".weight"):
            terms = p.shape[0] if (name.startswith("resize_layers.0") or name.startswith("resize_layers.1")) else p[0].numel()
            sd[name] = u(tuple(p.shape)) * (3.0 / terms) ** 0.5
        elif name.endswith(".bias"):
            v = u(tuple(p.shape))
            sd[name] = torch.sign(v) * (0.05 + 0.1 * v.abs())
        else:
            raise ValueError("unexpected entry %s" % name)
    return sd


def make_inputs(grid, seed, in_channels=SMALL["in_channels"], device="cpu"):
    """what get_intermediate_layers(x, 4, return_class_token=True) returns on a patch grid: four (tokens [1, L, C], class token [1, C]), unit
    normal float32"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    L = grid[0] * grid[1]
    r = lambda *shape: torch.randn(shape, generator=g, device=device, dtype=torch.float32)
    return tuple((r(1, L, in_channels), r(1, in_channels)) for _ in range(4))


def grid_seed(name):
    return 500 + sorted(GRIDS).index(name)


def run_named(head, feats, patch_h, patch_w):
    """head(feats, patch_h, patch_w) with forward hooks on the modules whose outputs the tests compare -> {name: [1, C, H, W] tensor} for NAMES"""
    got, hooks = {}, []

    def keep(name):
        return lambda mod, args, out: got.__setitem__(name, out.detach().clone())
    for i in range(4):
        hooks.append(head.resize_layers[i].register_forward_hook(keep("layer_%d" % (i + 1))))
        hooks.append(getattr(head.scratch, "refinenet%d" % (i + 1)).register_forward_hook(keep("path_%d" % (i + 1))))
    hooks.append(head.scratch.output_conv1.register_forward_hook(keep("output_conv1")))
    try:
        with torch.no_grad():
            got["out"] = head(feats, patch_h, patch_w).detach().clone()
    finally:
        for h in hooks:
            h.remove()
    return got


def rel_dev(a, ref):
    """the error measure of every check here: max|a - ref| / max|ref|"""
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max() / ref.abs().max())


def nchw(rows, size):
    """[H W, C] rows -> [1, C, H, W]"""
    return rows.reshape(size[0], size[1], -1).permute(2, 0, 1).contiguous()[None]


# ---- the fixture's files: every file stays under FILE_LIMIT, so a large array is cut along its first axis into parts "name@i" ----------------------
def save_parts(prefix, arrays, budget=900 * 1024):
    """write `arrays` into prefix_00.npz, prefix_01.npz, ...; returns the paths"""
    parts = []
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        n = max(1, -(-a.nbytes // budget))
        if n == 1:
            parts.append((name, a))
        else:
            flat = a.reshape(-1)
            step = -(-flat.size // n)
            parts.append((name + "@shape", np.array(a.shape, dtype=np.int64)))
            parts += [("%s@%d" % (name, i), flat[i * step:(i + 1) * step]) for i in range(n)]
    files, cur, size = [], {}, 0
    for name, a in parts:
        if cur and size + a.nbytes > budget:
            files.append(cur)
            cur, size = {}, 0
        cur[name] = a
        size += a.nbytes
    if cur:
        files.append(cur)
    paths = []
    for i, f in enumerate(files):
        paths.append("%s_%02d.npz" % (prefix, i))
        np.savez_compressed(paths[-1], **f)
        assert os.path.getsize(paths[-1]) < FILE_LIMIT, paths[-1]
    return paths


def load_parts(prefix):
    """the inverse of save_parts -> ({name: array}, [paths])"""
    paths = sorted(glob.glob(prefix + "_[0-9][0-9].npz"))
    if not paths:
        raise FileNotFoundError(prefix + "_NN.npz")
    raw = {}
    for p in paths:
        with np.load(p) as z:
            raw.update({k: z[k] for k in z.files})
    out = {}
    for k, v in raw.items():
        if "@" not in k:
            out[k] = v
        elif k.endswith("@shape"):
            name = k[:-len("@shape")]
            n = sum(1 for q in raw if q.startswith(name + "@") and not q.endswith("@shape"))
            out[name] = np.concatenate([raw["%s@%d" % (name, i)] for i in range(n)]).reshape(tuple(v))
    return out, paths


def golden_prefix(root, what):
    return os.path.join(root, "tests", "golden", "dpt2d3d_" + what)


def load_fixture(root):
    """-> dict(weights = state dict of float32 tensors, floor, grids = {name: dict(feats, ref64 = {NAME: array}, dev32 = {NAME: float})}, paths)"""
    w, paths = load_parts(golden_prefix(root, "weights"))
    fx = dict(weights={k: torch.from_numpy(v) for k, v in w.items() if k != "floor"}, floor=float(w["floor"][0]), grids={}, paths=list(paths))
    for name in GRIDS:
        d, p = load_parts(golden_prefix(root, name))
        fx["paths"] += p
        feats = tuple((torch.from_numpy(d["in_tok%d" % i]), torch.from_numpy(d["in_cls%d" % i])) for i in range(4))
        fx["grids"][name] = dict(feats=feats, ref64={n: d[n + "_64"] for n in NAMES}, dev32={n: float(d["dev32_" + n][0]) for n in NAMES})
    return fx
