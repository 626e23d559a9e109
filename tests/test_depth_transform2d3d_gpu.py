"""GPU: Depth-Anything's input transform on the device (csrc/image_transform.hip, csrc/cubic_index.h; diffreg_hip/depth_transform2d3d.py), the depth
branch as one engine (diffreg_hip/depth_branch2d3d.py) and the overlay's depth_transform flag.

Bars.  The kernel, per case: max |device - float64 statement| <= 4 x max |torch float32 - float64 statement|, where the float64 statement is
tests/depth_transform_ref.py (held to torch's float64 bicubic by tests/test_depth_transform2d3d_oracle.py) and torch float32 is
F.interpolate(mode="bicubic", align_corners=False) in float32 on the same device followed by the same float64 normalisation narrowed to float32,
computed on the spot.  No floor.  The largest measured ratio device / torch is printed.  The engine: torch.equal between its own forms; within
1e-4 max(1, max |depth|) (the bar tests/test_depth_encoder2d3d_gpu.py holds the bound encoder + head to) of the module's own float32 run on the
float64-stated transform.  The sizes are the smallest at which the kernel can go wrong; every output lies between guard bands."""
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import depth_encoder2d3d_ref as ER
from tests import depth_transform_ref as R
from tests import dpt2d3d_ref as DR
from tests.conftest import ROOT
from tests.helpers import guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DR_OK, DR_EINVAL = 0, -1
NORM = (R.MEAN, R.STD)
# source, destination                                  what it exercises
CASES = [((1, 1), (14, 14)),                          # all taps clamped
         ((2, 3), (14, 14)),
         ((3, 5), (14, 14)),
         ((5, 7), (5, 7)),                            # identity: t = 0, output equals input bit for bit before normalisation
         ((30, 40), (28, 42)),                        # down on one axis and up on the other, at the production ratio
         ((48, 64), (14, 70)),                        # a destination width off a multiple of 64
         ((9, 11), (28, 28)),                         # 3 x up
         ((4, 640), (4, 630))]                        # the production row


@pytest.fixture(scope="module")
def T():
    from diffreg_hip import depth_transform2d3d as mod
    return mod


@pytest.fixture(scope="module")
def B():
    from diffreg_hip import depth_branch2d3d as mod
    return mod


@pytest.fixture(scope="module")
def fx():
    return ER.load_fixture()


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def image(src, hi, pad, seed):
    """a [Hs, Ws, 3] view with 3 Ws + pad floats between rows, values in [0, hi]"""
    Hs, Ws = src
    buf = torch.rand(Hs, 3 * Ws + pad, generator=gen(seed), device=DEV) * hi
    return buf[:, :3 * Ws].view(Hs, Ws, 3) if pad == 0 else torch.as_strided(buf, (Hs, Ws, 3), (3 * Ws + pad, 3, 1))


def narrowed_norm(chw32):
    """the float64 normalisation of a float32 [3, h, w], narrowed to float32 as the kernel and PrepareForNet narrow it"""
    m, s = (torch.tensor(v, dtype=torch.float64).view(3, 1, 1) for v in NORM)
    return ((chw32.double().cpu() - m) / s).float()


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hi", [1.0, 255.0])
@pytest.mark.parametrize("src,dst", CASES)
def test_kernel_against_the_float64_statement(T, src, dst, hi):
    worst = 0.0
    for pad in (0, 5):
        img = image(src, hi, pad, seed=src[0] * 1000 + src[1] + pad)
        assert img.stride(0) == 3 * src[1] + pad or src[0] == 1
        t32 = F.interpolate(img.permute(2, 0, 1)[None].contiguous(), size=dst, mode="bicubic", align_corners=False)[0]
        for normalize in (False, True):
            out, check = guarded((3,) + dst, torch.float32, DEV, fill=float("nan"))
            rc = T.image_cubic_chw_raw(src[0], src[1], 3 * src[1] + pad, img, dst[0], dst[1], normalize, NORM if normalize else None, out)
            assert rc == DR_OK
            check()
            again, check2 = guarded((3,) + dst, torch.float32, DEV, fill=float("nan"))
            assert T.image_cubic_chw_raw(src[0], src[1], 3 * src[1] + pad, img, dst[0], dst[1], normalize, NORM if normalize else None, again) == DR_OK
            check2()
            assert torch.equal(out, again), "two runs differ"
            f64 = torch.from_numpy(R.transform(img.cpu().numpy(), dst, *(NORM if normalize else (None, None))))
            ref32 = narrowed_norm(t32) if normalize else t32.cpu()
            e, d = (out.cpu().double() - f64).abs().max().item(), (ref32.double() - f64).abs().max().item()
            ratio = e / d if d > 0 else (0.0 if e == 0 else float("inf"))
            worst = max(worst, ratio)
            print("%s -> %s, [0, %g], pad %d, normalize %d: device %.3e from float64, torch float32 %.3e (bar %.3e, ratio %.3f)"
                  % (src, dst, hi, pad, normalize, e, d, 4 * d, ratio))
            assert e <= 4 * d, (src, dst, hi, pad, normalize, e, d)
            if src == dst and not normalize:
                assert torch.equal(out, img.permute(2, 0, 1)), "the identity is not bit for bit"
    print("largest measured ratio device / torch float32: %.3f" % worst)


def test_kernel_refusals_leave_the_output_untouched(T):
    src, dst = (5, 7), (14, 14)
    img = image(src, 1.0, 0, seed=3)
    out, check = guarded((3,) + dst, torch.float32, DEV, fill=-7.0)
    ok = dict(Hs=5, Ws=7, ld_src=21, src=img, Hd=14, Wd=14, normalize=True, norm=NORM, out=out)
    bad = [dict(Hs=0), dict(Ws=0), dict(Hd=0), dict(Wd=0), dict(Hs=-1), dict(Wd=-3), dict(ld_src=20), dict(ld_src=0), dict(src=None),
           dict(norm=None), dict(norm=(R.MEAN, (0.229, 0.0, 0.225))), dict(norm=(R.MEAN, (0.0, 0.224, 0.225))), dict(norm=(R.MEAN, (0.229, 0.224, 0.0)))]
    for change in bad:
        a = dict(ok, **change)
        rc = T.image_cubic_chw_raw(a["Hs"], a["Ws"], a["ld_src"], a["src"], a["Hd"], a["Wd"], a["normalize"], a["norm"], a["out"], stream_tensor=out)
        assert rc == DR_EINVAL, change
        check()
        assert bool((out == -7.0).all()), change
    assert T.image_cubic_chw_raw(5, 7, 21, img, 14, 14, True, NORM, None, stream_tensor=out) == DR_EINVAL      # no output to write
    assert T.image_cubic_chw_raw(5, 7, 21, img, 14, 14, False, None, out) == DR_OK                             # without normalize a NULL norm is fine
    check()
    assert bool(torch.isfinite(out).all()) and not bool((out == -7.0).all())


def test_device_transform_is_the_size_rule_and_one_launch_into_chw(T):
    t = T.DeviceTransform(width=42, height=28, multiple_of=14)
    img = image((30, 40), 1.0, 5, seed=11)                        # a wider leading dimension goes in as ld_src
    x = t(img)
    assert tuple(x.shape) == (1, 3, 28, 42) and x.dtype == torch.float32 and x.is_contiguous() and t.size(40, 30) == (42, 28)
    f64 = torch.from_numpy(R.transform(img.cpu().numpy(), (28, 42)))
    assert (x[0].cpu().double() - f64).abs().max().item() < 1e-5
    assert torch.equal(x, t(img.contiguous()))
    plain = T.DeviceTransform(width=42, height=28, multiple_of=14, mean=None, std=None)(img)
    assert torch.equal(narrowed_norm(plain[0]), x[0].cpu())
    assert T.DeviceTransform().size(640, 480) == (630, 476)
    for wrong in (img.cpu(), img.double(), img.permute(2, 0, 1), img[None], img.half(), img.cpu().numpy(), img[:, :, :2]):
        with pytest.raises(TypeError):
            t(wrong)


def test_kernel_against_opencv_when_it_is_there(T):
    cv2 = pytest.importorskip("cv2")
    for src, dst in CASES:
        img = image(src, 255.0, 0, seed=17)
        host = img.cpu().numpy()
        want = torch.from_numpy(np.ascontiguousarray(cv2.resize(host, (dst[1], dst[0]), interpolation=cv2.INTER_CUBIC).reshape(dst + (3,))
                                                     .transpose(2, 0, 1)))
        out = torch.empty((3,) + dst, device=DEV)
        assert T.image_cubic_chw_raw(src[0], src[1], 3 * src[1], img, dst[0], dst[1], False, None, out) == DR_OK
        f64 = torch.from_numpy(R.transform(host, dst, None, None))
        t32 = F.interpolate(img.permute(2, 0, 1)[None].contiguous(), size=dst, mode="bicubic", align_corners=False)[0].cpu()
        own, bar = (want.double() - f64).abs().max().item(), 4 * (t32.double() - f64).abs().max().item()
        e = (out.cpu() - want).abs().max().item()
        print("%s -> %s: device %.3e from cv2, cv2 %.3e from the float64 statement (bar %.3e)" % (src, dst, e, own, own + bar))
        assert e <= own + bar


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------------
def depth_model(fx):
    vit = ER.fixture_vit(fx, torch.float32, DEV)
    head = DR.small_head(device=DEV, weights=DR.load_fixture(ROOT)["weights"])
    return ER.DepthModelStandIn(vit, head).to(DEV).eval(), vit, head


def small_transform(T):
    return T.DeviceTransform(width=42, height=28, multiple_of=14)          # a 2 x 3 patch grid


def bound(vit, head):
    return "get_intermediate_layers" in vit.__dict__, "forward" in head.__dict__


def test_engine_eager_equals_the_unskipped_path_and_the_modules_own_run(T, B, fx):
    dm, vit, head = depth_model(fx)
    img = image((30, 40), 1.0, 0, seed=21)
    t = small_transform(T)
    x64 = torch.from_numpy(R.transform(img.cpu().numpy(), (28, 42))).float().to(DEV)[None]
    with torch.no_grad():
        own = dm(x64)                                                      # the module's own float32 code on the float64-stated transform
    branch = B.DepthBranch2D3D(dm, transform=t)
    assert bound(vit, head) == (True, True)
    got = branch(img)
    assert tuple(got.shape) == (1, 28, 42) and got.dtype == torch.float32
    with torch.no_grad():
        want = dm(t(img))                                                  # the trailing F.interpolate + F.relu executed
    assert torch.equal(got, want)
    e, bar = (got - own).abs().max().item(), 1e-4 * max(1.0, own.abs().max().item())
    print("engine eager: %.3e from the module's own float32 run on the float64-stated transform (bar %.3e)" % (e, bar))
    assert e <= bar
    with torch.enable_grad():                                              # the engine runs under its own no_grad
        assert torch.equal(branch(img), got) and not branch(img).requires_grad
    for wrong in (img.cpu(), img.double(), img.permute(2, 0, 1)):
        for graph in (False, True):
            with pytest.raises(TypeError):
                branch(wrong, graph=graph)
    branch.remove()
    assert bound(vit, head) == (False, False)


def test_engine_graph_replay_equals_eager_and_keeps_four_shapes(T, B, fx):
    dm, vit, head = depth_model(fx)
    branch = B.DepthBranch2D3D(dm, transform=small_transform(T))
    img, img2 = image((30, 40), 1.0, 0, seed=31), image((30, 40), 1.0, 5, seed=32)
    eager, eager2 = branch(img).clone(), branch(img2).clone()
    first = branch(img, graph=True)                                        # capture + first replay
    assert torch.equal(first, eager) and branch.graphs == [(30, 40, 3)]
    again = branch(img, graph=True)
    assert again.data_ptr() == first.data_ptr() and torch.equal(again, eager)
    other = branch(img2, graph=True)                                       # the same shape, other values, a wider leading dimension: a replay
    assert other.data_ptr() == first.data_ptr() and torch.equal(other, eager2) and len(branch.graphs) == 1
    img3 = image((48, 64), 1.0, 0, seed=33)                                # a second source shape captures a second graph
    assert torch.equal(branch(img3, graph=True), branch(img3)) and branch.graphs == [(30, 40, 3), (48, 64, 3)]
    assert torch.equal(branch(img, graph=True), eager)                     # the first one still replays, and is now the most recent
    for k, shape in enumerate([(31, 40), (32, 40), (33, 40)]):             # at most four are kept: the one used longest ago goes first
        im = image(shape, 1.0, 0, seed=40 + k)
        assert torch.equal(branch(im, graph=True), branch(im))
    assert len(branch.graphs) == 4 and (48, 64, 3) not in branch.graphs and (30, 40, 3) in branch.graphs
    branch.remove()
    assert branch.graphs == [] and bound(vit, head) == (False, False)


def test_engine_refresh_after_an_in_place_weight_update(T, B, fx):
    dm, vit, head = depth_model(fx)
    branch = B.DepthBranch2D3D(dm, transform=small_transform(T))
    img = image((30, 40), 1.0, 0, seed=51)
    before = branch(img, graph=True).clone()
    with torch.no_grad():
        vit.patch_embed.proj.weight.mul_(-1.0)                             # the encoder keeps a padded copy of this one
        head.scratch.output_conv1.weight.mul_(0.5)                         # and the head a packed image of this one
    branch.refresh()
    assert branch.graphs == []
    after = branch(img, graph=True).clone()
    assert not torch.equal(after, before) and torch.equal(after, branch(img))
    branch.remove()


def test_engine_remove_undoes_only_its_own_binds_and_a_refusal_leaves_nothing(T, B, fx):
    from diffreg_hip import depth_encoder2d3d, dpt2d3d
    dm, vit, head = depth_model(fx)
    undo = depth_encoder2d3d.bind(dm)                                      # the encoder was bound before the engine was built
    mine = vit.__dict__["get_intermediate_layers"]
    branch = B.DepthBranch2D3D(dm, transform=small_transform(T))
    assert vit.__dict__["get_intermediate_layers"] is mine and bound(vit, head) == (True, True)
    branch.remove()
    assert vit.__dict__.get("get_intermediate_layers") is mine and bound(vit, head) == (True, False)
    undo()
    undo_head = dpt2d3d.bind(head)                                         # the same for the head
    branch = B.DepthBranch2D3D(dm, transform=small_transform(T))
    branch.remove()
    assert bound(vit, head) == (False, True)
    undo_head()
    assert bound(vit, head) == (False, False)
    head.use_clstoken = True                                               # the head refuses after the encoder was bound: nothing stays
    with pytest.raises(NotImplementedError):
        B.DepthBranch2D3D(dm, transform=small_transform(T))
    assert bound(vit, head) == (False, False)
    head.use_clstoken = False
    vit.num_register_tokens = 4                                            # the encoder refuses
    with pytest.raises(NotImplementedError):
        B.DepthBranch2D3D(dm, transform=small_transform(T))
    assert bound(vit, head) == (False, False)


# ---- the overlay flag ------------------------------------------------------------------------------------------------------------------------------
MODEL_SOURCE = '''
import types
import torch


@torch.no_grad()
def predict_depth(model, image):
    return model(image)


class Model(types.SimpleNamespace):
    """the depth stretch of a forward that copies its image to the host, transforms it there and copies it back"""

    def forward(self, data_dict):
        host = data_dict["image"].unsqueeze(1).detach().squeeze(0).squeeze(0).cpu().numpy()
        host = self.transform({"image": host})["image"]
        return predict_depth(self.depth_model, torch.from_numpy(host).unsqueeze(0).cuda())
'''


@pytest.fixture
def model_module():
    name = "dr_test_depth_transform_model"
    mod = types.ModuleType(name)
    sys.modules[name] = mod
    exec(compile(MODEL_SOURCE, name, "exec"), mod.__dict__)
    mod.Model.__module__ = name
    yield mod
    del sys.modules[name]


def test_accelerate_depth_transform_binds_three_sites_and_removes(T, B, fx, model_module):
    from diffreg_hip import overlay2d3d
    dm, vit, head = depth_model(fx)
    seen = []

    def host_transform(sample):
        seen.append(tuple(sample["image"].shape))
        return {"image": R.transform(sample["image"], (28, 42)).astype(np.float32)}
    stub = lambda: types.SimpleNamespace(forward=None)
    model = lambda: model_module.Model(depth_model=dm, transform=host_transform, denoising_transformer=stub(), denoising_coarse_matching=stub(),
                                       get_warped_from_noising_matching3D3D=None)
    img = image((30, 40), 1.0, 0, seed=61)
    data = {"image": img[None]}
    original = model_module.predict_depth
    m = model()
    own = m.forward(data)                                                  # the host path as it stands
    assert seen == [(30, 40, 3)]
    ov = overlay2d3d.accelerate(m)                                         # opt-in: off by default
    assert "forward" not in m.__dict__ and m.transform is host_transform and model_module.predict_depth is original and bound(vit, head) == (False, False)
    ov.remove()
    m = model()
    ov = overlay2d3d.accelerate(m, depth_transform=dict(width=42, height=28))
    assert "forward" in m.__dict__ and m.transform is not host_transform and model_module.predict_depth is not original
    assert bound(vit, head) == (True, True)
    got = m.forward(data)
    assert seen == [(30, 40, 3)], "the host transform was given an image"
    engine = B.DepthBranch2D3D(dm, transform=small_transform(T))           # (reuses the overlay's binds)
    assert torch.equal(got, engine(img)) and tuple(got.shape) == (1, 28, 42)
    assert torch.equal(ov.depth(img[None, None]), got)                     # what the one-line edit of the model file calls
    e, bar = (got - own).abs().max().item(), 1e-4 * max(1.0, own.abs().max().item())
    print("overlay depth: %.3e from the host path (bar %.3e)" % (e, bar))
    assert e <= bar
    x = small_transform(T)(img)                                            # a real image through the bound global: the original predict_depth
    assert torch.equal(model_module.predict_depth(dm, x), original(dm, x))
    engine.remove()
    assert bound(vit, head) == (True, True)
    ov.remove()
    assert "forward" not in m.__dict__ and m.transform is host_transform and model_module.predict_depth is original
    assert bound(vit, head) == (False, False) and "_dr_overlay" not in m.__dict__
    assert torch.equal(m.forward(data), own) and len(seen) == 2            # the host path again
    m = model()                                                            # replay
    ov = overlay2d3d.accelerate(m, depth_transform=dict(graph=True, width=42, height=28))
    assert torch.equal(m.forward(data), got) and torch.equal(m.forward(data), got) and len(seen) == 2
    ov.remove()
    head.use_clstoken = True                                               # a refusing head leaves nothing bound
    m = model()
    with pytest.raises(NotImplementedError):
        overlay2d3d.accelerate(m, depth_transform=True)
    assert "forward" not in m.__dict__ and m.transform is host_transform and model_module.predict_depth is original
    assert bound(vit, head) == (False, False) and m.denoising_transformer.forward is None
