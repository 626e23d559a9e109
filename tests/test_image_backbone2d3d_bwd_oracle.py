"""CPU checks of the 2D-3D image backbone's backward: the ABI boundary of the fifth set, the gradient fixture minted from the reference
(tests/golden/image_backbone2d3d_bwd*.npz, tools/golden/make_golden_image_backbone2d3d_bwd.py), the restatement of
tests/image_backbone2d3d_ref.py as float64 autograd against it, and the slab / workspace rule of the weight gradient.

Bars.  Error measure: per gradient tensor, max|a - ref64| / max|ref64| (image_backbone2d3d_ref.rel_dev).  The restatement's float64 autograd
reproduces every stored float64 gradient to 1e-12 (same operations; what remains is the summation order of the CPU kernels)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import image_backbone2d3d_bwd_ref as B
from tests import image_backbone2d3d_ref as R
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("dr_conv2d_rows_backward_data_f32", "dr_conv2d_rows_backward_weight_f32", "dr_conv2d_rows_backward_weight_workspace_bytes",
       "dr_resize_rows_backward_f32")


@pytest.fixture(scope="module")
def fixture():
    return B.load(GOLDEN)


def test_new_entries_are_bound_and_declared():
    from diffreg_hip import lib
    header = open(os.path.join(ROOT, "include", "diffreg_hip.h")).read()
    assert lib.raw().dr_version() == lib.ABI_VERSION and re.search(r"#define DR_ABI_VERSION %d\b" % lib.ABI_VERSION, header)
    for name in NEW:
        assert name in lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib.raw(), name)
    for name in ("pack_conv_weight_t", "conv2d_rows_backward_data", "conv2d_rows_backward_weight", "resize_rows_backward"):
        assert callable(getattr(lib, name)), name


def test_fixture_records_its_floors_and_no_gradient_is_zero(fixture):
    for name in B.BWD_CASES:
        names, dev = [str(n) for n in fixture[name + "_names"]], fixture[name + "_dev32"]
        assert names == B.grad_names(R.ImageBackbone(1, R.CASES[name]["out"], R.CASES[name]["base"]))
        assert dev.shape == (len(names),) and (dev > 0).all()
        assert float(fixture[name + "_floor"][0]) == float(np.median(dev)) > 0
        for n in names:
            g = fixture["%s/%s" % (name, n)]
            assert g.dtype == np.float64 and np.isfinite(g).all() and float(np.abs(g).max()) > 0, (name, n)
        print("case %s: %d tensors, dev32 %.2e .. %.2e, floor %.3e" % (name, len(names), dev.min(), dev.max(), float(fixture[name + "_floor"][0])))
    for fn in os.listdir(GOLDEN):
        if fn.startswith("image_backbone2d3d_bwd"):
            assert os.path.getsize(os.path.join(GOLDEN, fn)) < 1024 * 1024, fn


@pytest.mark.parametrize("name", B.BWD_CASES)
def test_restatement_autograd_against_the_reference(name, fixture):
    case = R.CASES[name]
    x, dino = R.make_inputs(case)
    _, g64 = B.run_backward(R.build(case, torch.float64), x, dino, case)
    worst = 0.0
    for n in B.grad_names(R.ImageBackbone(1, case["out"], case["base"])):
        ref = fixture["%s/%s" % (name, n)]
        assert tuple(g64[n].shape) == ref.shape, n
        e = R.rel_dev(g64[n], ref)
        worst = max(worst, e)
        assert e <= 1e-12, (name, n, e)
    print("case %s: restatement float64 autograd within %.2e of the reference's float64 gradients" % (name, worst))


def _backbone_convs(H, W, base, out):
    """(k, s, p, d, Cin, Cout, H, W) of every conv of ImageBackbone(1, out, base) on an H x W image"""
    from diffreg_hip.lib import conv_out_size as o
    b = base
    H1, W1 = o(H, 7, 2, 3), o(W, 7, 2, 3)
    H2, W2 = o(H1, 3, 2, 1), o(W1, 3, 2, 1)
    H3, W3 = o(H2, 3, 2, 1), o(W2, 3, 2, 1)
    return [(7, 2, 3, 1, 1, b, H, W), (3, 1, 1, 1, b, b, H1, W1), (3, 2, 1, 1, b, 2 * b, H1, W1), (3, 1, 1, 1, 2 * b, 2 * b, H2, W2),
            (3, 2, 1, 1, 2 * b, 4 * b, H2, W2), (3, 1, 1, 1, 4 * b, 4 * b, H3, W3), (1, 1, 0, 1, 4 * b, 4 * b, H3, W3), (1, 1, 0, 1, 2 * b, 4 * b, H2, W2),
            (3, 1, 1, 1, 4 * b, 2 * b, H2, W2), (1, 1, 0, 1, b, 2 * b, H1, W1), (3, 1, 1, 1, 2 * b, b, H1, W1), (1, 1, 0, 1, b, b, H1, W1),
            (3, 1, 1, 1, b, b, H, W), (1, 1, 0, 1, b, out, H, W)]


EXTRA_CONV_CASES = {
    "uncovered": (3, 2, 0, 1, 16, 16, 8, 10),
    "stride3_dil2": (3, 3, 2, 2, 8, 12, 14, 17),
    "slabs": (3, 1, 1, 1, 20, 72, 65, 67),
    "cout_10": (3, 1, 1, 1, 16, 10, 9, 11),
    "cin_6": (3, 2, 1, 1, 6, 12, 9, 11),
}


def test_slab_and_workspace_rule_agrees_with_the_library():
    """lib.conv_wgrad_slabs / conv_wgrad_workspace_bytes (the Python statement of conv_index.h's rule) against the library's own size query, a pure
    host call, on the test and production shapes; the rule depends on the shape alone"""
    from diffreg_hip import lib
    q = lib.raw().dr_conv2d_rows_backward_weight_workspace_bytes
    shapes = list(R.CONV_CASES.values()) + list(EXTRA_CONV_CASES.values())
    for case in (R.CASES["b"], R.CASES["c"], R.REAL, R.PRODUCTION):
        shapes += _backbone_convs(case["image"][0], case["image"][1], case["base"], case["out"])
    worst = 0
    for (k, s, p, d, cin, cout, H, W) in shapes:
        M = lib.conv_out_size(H, k, s, p, d) * lib.conv_out_size(W, k, s, p, d)
        S, L = lib.conv_wgrad_slabs(M)
        assert 1 <= S <= 64 and L % 32 == 0 and S * L >= M > (S - 1) * L
        want = lib.conv_wgrad_workspace_bytes(M, cout, k * k * cin)
        assert q(H, W, cin, cout, k, s, p, d) == want, (k, s, p, d, cin, cout, H, W)
        worst = max(worst, want)
    print("largest workspace over the test and production shapes: %.1f MB" % (worst / 1e6))
    assert worst < 64e6                                                 # the production workspace stays under 64 MB
    assert lib.conv_wgrad_slabs(65 * 67) == (3, 1472)                    # the `slabs` case: three slabs, the last one ragged (1 411 pixels)
    assert q(2, 2, 4, 4, 3, 1, 0, 1) == 0 and q(5, 5, 4, 4, 32, 1, 16, 1) == 0          # outside the domain


def test_out_of_domain_arguments_return_their_code_on_the_host():
    """the argument checks run before any launch (no GPU needed; the pointers are never dereferenced)"""
    from diffreg_hip import lib
    r = lib.raw()
    p_ = torch.zeros(8).data_ptr() // 16 * 16 + 16
    dg = lambda H, W, cin, cout, k, s, p, d, ldg=None, ldgx=None, g=p_: r.dr_conv2d_rows_backward_data_f32(
        H, W, cin, cout, k, s, p, d, g, cout if ldg is None else ldg, p_, None, 0, p_, cin if ldgx is None else ldgx, None)
    assert dg(2, 2, 4, 4, 3, 1, 0, 1) == -1 and dg(5, 5, 4, 4, 3, 0, 1, 1) == -1 and dg(5, 5, 4, 4, 3, 1, 1, 1, ldg=3) == -1
    assert dg(5, 5, 4, 4, 3, 1, 1, 1, ldgx=3) == -1 and dg(5, 5, 4, 4, 3, 1, 1, 1, g=None) == -1 and dg(5, 5, 4, 4, 3, 1, 1, 1, g=p_ + 2) == -1
    assert dg(5, 5, 4, 4, 32, 1, 16, 1) == -3 and dg(5000, 5000, 4, 4, 3, 1, 1, 1) == -3 and dg(5, 5, 4, 1 << 17, 3, 1, 1, 1) == -3
    wg = lambda H, W, cin, cout, k, s, p, d, ldx=None, x=p_, ws=p_, wsb=1 << 30: r.dr_conv2d_rows_backward_weight_f32(
        H, W, cin, cout, k, s, p, d, x, cin if ldx is None else ldx, p_, cout, p_, p_, ws, wsb, None)
    assert wg(2, 2, 4, 4, 3, 1, 0, 1) == -1 and wg(5, 5, 4, 4, 3, 1, 1, 1, ldx=3) == -1 and wg(5, 5, 4, 4, 3, 1, 1, 1, x=None) == -1
    assert wg(5, 5, 4, 4, 3, 1, 1, 1, ws=None) == -1 and wg(5, 5, 4, 4, 3, 1, 1, 1, wsb=16) == -1 and wg(5, 5, 4, 4, 32, 1, 16, 1) == -3
    rb = r.dr_resize_rows_backward_f32
    assert rb(4, 0, 3, 2, 2, p_, 4, p_, 4, None) == -1 and rb(4, 2, 3, 2, 2, p_, 3, p_, 4, None) == -1 and rb(4, 2, 3, 2, 2, None, 4, p_, 4, None) == -1
    assert rb(4, 5000, 5000, 2, 2, p_, 4, p_, 4, None) == -3
