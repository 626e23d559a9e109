"""CPU checks of the DPT head (Depth-Anything's decoder): the restatement of tests/dpt2d3d_ref.py pinned to the reference's own tensors
(tests/golden/dpt2d3d_*.npz, minted by tools/golden/make_golden_dpt2d3d.py from depth_anything/dpt.py's DPTHead), what the fixture claims to
exercise, the ABI boundary of the seventh set, and the configurations DeviceDPTHead refuses at construction.

Bars.  Error measure: per tensor, max|a - ref64| / max|ref64| (dpt2d3d_ref.rel_dev).  The restatement in float64 reproduces every float64 tensor
of the fixture to 1e-9; in float32 it stays within 2 x the deviation the reference's own float32 run recorded for that tensor."""
import os
import re

import pytest
import torch
import torch.nn as nn

from tests import dpt2d3d_ref as R
from tests.conftest import ROOT

NEW = ("dr_conv2d_rows_act_f32", "dr_conv_transpose2d_rows_f32", "dr_conv2d_rows_project_f32")


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture(ROOT)


@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_restatement_against_the_reference(fx, grid):
    ph, pw = R.GRIDS[grid]
    g = fx["grids"][grid]
    drawn = R.make_inputs((ph, pw), R.grid_seed(grid))
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(drawn, g["feats"])), "the stored inputs are the drawn ones"
    t64 = R.run_named(R.small_head(torch.float64, weights=fx["weights"]), tuple((a.double(), b.double()) for a, b in g["feats"]), ph, pw)
    t32 = R.run_named(R.small_head(torch.float32, weights=fx["weights"]), g["feats"], ph, pw)
    for n in R.NAMES:
        ref, d = g["ref64"][n], g["dev32"][n]
        assert tuple(t64[n].shape) == ref.shape and ref.dtype.name == "float64"
        e64, e32 = R.rel_dev(t64[n], ref), R.rel_dev(t32[n], ref)
        print("grid %s %s: restatement float64 %.2e, float32 %.2e; the reference's float32 %.2e" % (grid, n, e64, e32, d))
        assert e64 <= 1e-9, (grid, n, e64)
        assert e32 <= 2 * d, (grid, n, e32, d)


def test_stored_weights_are_the_drawn_ones(fx):
    drawn = R.draw_weights(R.DPTHead(R.SMALL["in_channels"], R.SMALL["features"], R.SMALL["out_channels"]), R.WEIGHT_SEED)
    assert list(drawn) == list(fx["weights"])
    for k, v in drawn.items():
        assert v.dtype == torch.float32 and torch.equal(v, fx["weights"][k]), k
        if k.endswith(".bias"):
            assert float(v.abs().min()) >= 0.05, "biases lie away from zero"


def test_fixture_exercises_what_it_claims(fx):
    assert set(fx["grids"]) == {"3x5", "5x5", "10x13"} and R.GRIDS == {"3x5": (3, 5), "5x5": (5, 5), "10x13": (10, 13)}
    up = lambda n: -(-n // 2)
    not_x2 = 0
    for grid, (ph, pw) in R.GRIDS.items():
        ref = fx["grids"][grid]["ref64"]
        sizes = {n: tuple(ref[n].shape[2:]) for n in R.NAMES}
        assert sizes["layer_1"] == (4 * ph, 4 * pw) and sizes["layer_2"] == (2 * ph, 2 * pw) and sizes["layer_3"] == (ph, pw)
        assert sizes["layer_4"] == (up(ph), up(pw))                                # the stride-2 conv: ceil(h / 2)
        assert sizes["path_4"] == sizes["layer_3"] and sizes["path_3"] == sizes["layer_2"] and sizes["path_2"] == sizes["layer_1"]
        assert sizes["path_1"] == sizes["output_conv1"] == (8 * ph, 8 * pw) and sizes["out"] == (14 * ph, 14 * pw)
        not_x2 += sizes["path_4"] != (2 * sizes["layer_4"][0], 2 * sizes["layer_4"][1])
        assert [ref["layer_%d" % (i + 1)].shape[1] for i in range(4)] == R.SMALL["out_channels"]
    assert not_x2 >= 1, "at least one resample that is not x 2"
    assert (40 * 52) % 64 != 0 and fx["grids"]["10x13"]["ref64"]["layer_1"].shape[2:] == (40, 52)
    devs = [d for g in fx["grids"].values() for d in g["dev32"].values()]
    assert len(devs) == 30 and fx["floor"] == min(devs) > 0
    for p in fx["paths"]:
        assert os.path.getsize(p) < 1 << 20, p


@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_every_relu_sees_negative_values(fx, grid):
    """a missing ReLU cannot pass: the input of every ReLU call of the head holds negative values (and positive ones)"""
    ph, pw = R.GRIDS[grid]
    head = R.small_head(torch.float64, weights=fx["weights"])
    seen = []
    hooks = [m.register_forward_pre_hook(lambda mod, args: seen.append((float(args[0].min()), float(args[0].max()))))
             for m in head.modules() if isinstance(m, nn.ReLU)]
    with torch.no_grad():
        head(tuple((a.double(), b.double()) for a, b in fx["grids"][grid]["feats"]), ph, pw)
    for h in hooks:
        h.remove()
    assert len(seen) == 2 * 7 + 2                                                   # seven units run (refinenet4 skips its first), two calls each; the tail's two
    assert all(lo < 0 < hi for lo, hi in seen), seen


def test_new_entries_are_bound_and_declared():
    from diffreg_hip import lib
    header = open(os.path.join(ROOT, "include", "diffreg_hip.h")).read()
    assert lib.raw().dr_version() == lib.ABI_VERSION == 700 and re.search(r"#define DR_ABI_VERSION 700\b", header)
    for name in NEW:
        assert name in lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib.raw(), name)
    assert re.search(r"#define DR_CONV_RELU_IN %d\b" % lib.CONV_RELU_IN, header) and re.search(r"#define DR_CONV_RELU_OUT %d\b" % lib.CONV_RELU_OUT, header)
    for f in ("conv2d_rows_act", "conv_transpose2d_rows", "pack_conv_transpose_weight", "conv2d_rows_project"):
        assert callable(getattr(lib, f))


def test_argument_checks_run_before_any_launch():
    """the host-side checks of the three entries (no GPU needed: the pointers are never dereferenced)"""
    from diffreg_hip import lib
    r = lib.raw()
    buf = torch.zeros(1 << 16)
    p, q, w = buf.data_ptr(), buf.data_ptr() + 4 * 20000, buf.data_ptr() + 4 * 40000          # x, out, weight: disjoint
    act = lambda Hi=5, Wi=5, Cin=4, Cout=4, k=3, s=1, pad=1, d=1, x=p, ldx=None, flags=0, a=None, a2=None, out=q, wt=w: r.dr_conv2d_rows_act_f32(
        Hi, Wi, Cin, Cout, k, s, pad, d, x, Cin if ldx is None else ldx, wt, None, flags, a, Cout, a2, Cout, out, Cout, None)
    assert act(out=p) == -1 and act(a=q) == -1 and act(a2=q) == -1 and act(out=p + 4 * 50) == -1 and act(out=w) == -1      # out aliases an input
    assert act(x=None) == -1 and act(out=None) == -1 and act(wt=None) == -1 and act(x=p + 2) == -1 and act(flags=4) == -1 and act(ldx=3) == -1
    assert act(Cin=3, flags=1) == -3 and act(Cin=3, flags=2) == -3 and act(Cin=3, a2=p + 4 * 60000) == -3                  # flags on the direct arm
    assert act(Hi=5000, Wi=5000) == -3 and act(k=32, pad=16) == -3 and act(Cin=1 << 17) == -3
    assert act(Hi=2, Wi=2, pad=0) == -1
    tr = lambda H=3, W=5, Cin=4, Cout=4, s=2, x=p, out=q, wt=w, ldx=None, ldo=None: r.dr_conv_transpose2d_rows_f32(
        H, W, Cin, Cout, s, x, Cin if ldx is None else ldx, wt, None, out, Cout if ldo is None else ldo, None)
    assert tr(s=0) == -1 and tr(s=9) == -3 and tr(Cin=6) == -3 and tr(x=None) == -1 and tr(out=None) == -1 and tr(wt=None) == -1
    assert tr(out=p) == -1 and tr(ldx=3) == -1 and tr(ldo=3) == -1 and tr(H=4096, W=2048, s=2) == -3 and tr(s=8, Cout=1028) == -3
    pr = lambda Hi=5, Wi=5, Cin=4, Cmid=4, k=3, pad=1, x=p, w1=w, w2=w + 4 * 5000, out=q, ldo=1: r.dr_conv2d_rows_project_f32(
        Hi, Wi, Cin, Cmid, k, 1, pad, 1, x, Cin, w1, None, w2, None, 1, out, ldo, None)
    assert pr(Cmid=68) == -3 and pr(Cin=6) == -3 and pr(x=None) == -1 and pr(w2=None) == -1 and pr(out=None) == -1 and pr(out=p) == -1
    assert pr(ldo=0) == -1 and pr(Hi=5000, Wi=5000) == -3 and pr(Hi=2, Wi=2, pad=0) == -1


def test_pack_conv_transpose_weight_layout():
    from diffreg_hip import lib
    w = torch.arange(4 * 3 * 2 * 2, dtype=torch.float32).reshape(4, 3, 2, 2)                   # [Cin, Cout, s, s]
    pk = lib.pack_conv_transpose_weight(w)
    assert pk.shape == (2 * 2 * 3, 4) and pk.is_contiguous()
    for i in range(2):
        for j in range(2):
            for co in range(3):
                assert torch.equal(pk[(i * 2 + j) * 3 + co], w[:, co, i, j])
    with pytest.raises(NotImplementedError):
        lib.pack_conv_transpose_weight(torch.zeros(4, 3, 2, 3))


# ---- what DeviceDPTHead refuses, at construction ----------------------------------------------------------------------------------------------------
def _refused():
    small = lambda: R.DPTHead(R.SMALL["in_channels"], R.SMALL["features"], R.SMALL["out_channels"])
    cases = {}
    m = small(); m.use_clstoken = True; cases["use_clstoken"] = m
    m = small(); m.nclass = 3; cases["nclass > 1"] = m
    m = small(); del m.scratch.output_conv1; cases["no output_conv1"] = m
    m = small(); m.scratch.refinenet2.resConfUnit1.bn = True; cases["use_bn"] = m
    m = small(); m.scratch.refinenet3.expand = True; cases["expand"] = m
    m = small(); m.scratch.refinenet3.deconv = True; cases["deconv"] = m
    m = small(); m.scratch.refinenet1.resConfUnit2.groups = 2; cases["unit groups"] = m
    m = small(); m.scratch.layer2_rn = nn.Conv2d(32, 32, 3, padding=1, groups=2, bias=False); cases["conv groups"] = m
    m = small(); m.scratch.refinenet1.resConfUnit2.activation = nn.GELU(); cases["gelu"] = m
    m = small(); m.scratch.refinenet1.resConfUnit2.activation = nn.LeakyReLU(0.1); cases["leaky relu"] = m
    m = small(); m.scratch.refinenet1.resConfUnit2.activation = nn.ReLU(True); cases["in-place relu in a unit"] = m
    m = small(); m.scratch.output_conv2[1] = nn.Sigmoid(); cases["tail activation"] = m
    m = small(); m.resize_layers[0] = nn.ConvTranspose2d(16, 16, 4, stride=2, padding=1); cases["transposed conv, kernel != stride"] = m
    m = small(); m.resize_layers[1] = nn.Upsample(scale_factor=2); cases["reassemble layer of another kind"] = m
    m = small(); m.resize_layers[0] = nn.ConvTranspose2d(16, 16, 9, stride=9); cases["stride 9"] = m
    m = small(); m.projects[0] = nn.Conv2d(126, 16, 1); cases["Cin % 4 != 0"] = m
    m = small(); m.scratch.output_conv2[0] = nn.Conv2d(16, 68, 3, padding=1); m.scratch.output_conv2[2] = nn.Conv2d(68, 1, 1); cases["Cmid = 68"] = m
    cases["float64"] = small().double()
    cases["float16"] = small().half()
    return cases


@pytest.mark.parametrize("name", list(_refused()))
def test_binding_refuses_at_construction(name):
    from diffreg_hip import dpt2d3d
    mod = _refused()[name].eval()
    with pytest.raises(NotImplementedError):
        dpt2d3d.DeviceDPTHead(mod)
    with pytest.raises(NotImplementedError):
        dpt2d3d.bind(mod)
    assert "forward" not in mod.__dict__, name


def test_binding_accepts_the_restatement_and_undoes():
    from diffreg_hip import dpt2d3d
    head = R.small_head()
    undo = dpt2d3d.bind(head)
    assert "forward" in head.__dict__ and isinstance(undo.device, dpt2d3d.DeviceDPTHead)
    feats = R.make_inputs((3, 5), 1)
    with torch.no_grad():                                                           # CPU inputs: the module's own forward, unchanged
        got = head(feats, 3, 5)
    undo()
    assert "forward" not in head.__dict__
    with torch.no_grad():
        assert torch.equal(got, head(feats, 3, 5))
