"""CPU checks of the 2D-3D image backbone: the restatement of tests/image_backbone2d3d_ref.py pinned to the reference's own outputs
(tests/golden/image_backbone2d3d.npz, minted by tools/golden/make_golden_image_backbone2d3d.py from EXP/image_backbone.py's ImageBackbone), the
output-size function of csrc/conv_index.h against torch's conv2d shapes, and the ABI boundary of the two new entries.

Bars.  Error measure: per output tensor, max|a - ref64| / max|ref64| (image_backbone2d3d_ref.rel_dev).  The restatement in float64 reproduces the
reference's float64 outputs to 1e-12 (same operations, same order: what remains is the thread count of the CPU convolution); in float32 it stays
within 4 x the deviation the reference's own float32 run recorded for that output."""
import os
import re

import numpy as np
import pytest
import torch

from tests import image_backbone2d3d_ref as R
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "image_backbone2d3d.npz"))
NEW = ("dr_conv2d_rows_f32", "dr_resize_rows_f32")


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_against_the_reference(name):
    case = R.CASES[name]
    x, dino = R.make_inputs(case)
    assert np.array_equal(x.numpy(), G[name + "_in_x"]) and np.array_equal(dino.numpy(), G[name + "_in_dino"])
    with torch.no_grad():
        o64 = R.build(case, torch.float64)(x.double(), dino.double())
        o32 = R.build(case, torch.float32)(x, dino)
    assert len(o64) == 4
    for i in range(4):
        ref = G["%s_out%d_64" % (name, i)]
        assert tuple(o64[i].shape) == ref.shape and o64[i].is_contiguous()
        e64, e32, d = R.rel_dev(o64[i], ref), R.rel_dev(o32[i], ref), float(G[name + "_dev32"][i])
        print("case %s out%d: restatement float64 %.2e, float32 %.2e; the reference's float32 %.2e" % (name, i, e64, e32, d))
        assert e64 <= 1e-12, (name, i, e64)
        assert e32 <= 4 * d, (name, i, e32, d)


def test_fixture_records_its_floor():
    devs = np.concatenate([G[n + "_dev32"] for n in R.CASES])
    assert devs.shape == (12,) and float(G["floor"][0]) == float(devs.min()) > 0


def test_group_rule():
    """builder.py:72-86: at most 32 groups, at least 8 channels per group"""
    assert [R.num_groups(c) for c in (16, 32, 64, 128, 256, 512, 24)] == [2, 4, 8, 16, 32, 32, 2]


def test_conv_out_size_against_torch_shapes():
    """conv_index.h's conv_out_size (through its Python mirror lib.conv_out_size and through the library's own argument check) against the shapes
    torch.nn.functional.conv2d produces on the primitive case table"""
    from diffreg_hip import lib
    for name, (k, s, p, d, cin, cout, H, W) in R.CONV_CASES.items():
        if name == "large_tile":
            H, W = 24, 28                                            # the same geometry; the shape rule does not depend on the extent
        y = torch.nn.functional.conv2d(torch.zeros(1, cin, H, W), torch.zeros(cout, cin, k, k), stride=s, padding=p, dilation=d)
        assert (lib.conv_out_size(H, k, s, p, d), lib.conv_out_size(W, k, s, p, d)) == tuple(y.shape[2:]), name
    # the library's own use of it, in the argument checks that run before any launch (no GPU needed; the pointers are never dereferenced)
    r = lib.raw()
    p_ = torch.zeros(4).data_ptr()
    call = lambda H, W, cin, cout, k, s, p, d, ldx=None, ldo=None, x=p_: r.dr_conv2d_rows_f32(
        H, W, cin, cout, k, s, p, d, x, cin if ldx is None else ldx, p_, None, None, 0, p_, cout if ldo is None else ldo, None)
    assert call(2, 2, 4, 4, 3, 1, 0, 1) == -1                        # DR_EINVAL: a 3 x 3 kernel does not fit 2 x 2 without padding
    assert call(5, 5, 4, 4, 3, 1, 0, 3) == -1                        # ... nor its dilated extent 7 a 5 x 5 image
    assert call(0, 5, 4, 4, 3, 1, 1, 1) == -1 and call(5, 5, 4, 4, 3, 0, 1, 1) == -1 and call(5, 5, 4, 4, 3, 1, -1, 1) == -1
    assert call(5, 5, 4, 4, 3, 1, 1, 1, ldx=3) == -1 and call(5, 5, 4, 4, 3, 1, 1, 1, ldo=3) == -1
    assert call(5, 5, 4, 4, 3, 1, 1, 1, x=None) == -1 and call(5, 5, 4, 4, 3, 1, 1, 1, x=p_ + 2) == -1
    assert call(5, 5, 4, 4, 32, 1, 16, 1) == -3                      # DR_ENOSUP: beyond the stated domain
    assert call(5000, 5000, 4, 4, 3, 1, 1, 1) == -3 and call(5, 5, 1 << 17, 4, 3, 1, 1, 1) == -3
    assert r.dr_resize_rows_f32(4, 0, 3, 2, 2, p_, 4, None, 0, p_, 4, None) == -1
    assert r.dr_resize_rows_f32(4, 2, 3, 2, 2, p_, 3, None, 0, p_, 4, None) == -1
    assert r.dr_resize_rows_f32(4, 2, 3, 2, 2, None, 4, None, 0, p_, 4, None) == -1
    assert r.dr_resize_rows_f32(4, 5000, 5000, 2, 2, p_, 4, None, 0, p_, 4, None) == -3


def test_new_entries_are_bound_and_declared():
    from diffreg_hip import lib
    header = open(os.path.join(ROOT, "include", "diffreg_hip.h")).read()
    assert lib.raw().dr_version() == lib.ABI_VERSION and re.search(r"#define DR_ABI_VERSION %d\b" % lib.ABI_VERSION, header)
    for name in NEW:
        assert name in lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib.raw(), name)
