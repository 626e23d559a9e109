"""CPU: the two yardsticks of Depth-Anything's device transform (diffreg_hip/depth_transform2d3d.py).

 * transform_size against tests/golden/depth_transform_sizes.json, what the reference's own Resize.get_size returned for a table of inputs
   (tools/mint_depth_transform_sizes.py): production 640 x 480 -> (630, 476), the half-way widths 637 and 651 (45.5 and 46.5 multiples of 14: both
   round to even, 644), portrait, small, the min_val / max_val branches, keep_aspect_ratio=False, all three resize methods.
 * the float64 statement of the resample (tests/depth_transform_ref.py) against F.interpolate(mode="bicubic", align_corners=False) in float64 on the
   CPU at 1e-12 relative: torch uses the same kernel (A = -0.75), the same mapping and the same clamp, which pins the helper the GPU tests measure
   the kernel with.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import depth_transform_ref as R
from tests.conftest import ROOT

SIZES = os.path.join(ROOT, "tests", "golden", "depth_transform_sizes.json")
# (source, destination) of tests/test_depth_transform2d3d_gpu.py and the production axes on a strip
CASES = [((1, 1), (14, 14)), ((2, 3), (14, 14)), ((3, 5), (14, 14)), ((5, 7), (5, 7)), ((30, 40), (28, 42)), ((48, 64), (14, 70)), ((9, 11), (28, 28)),
         ((4, 640), (4, 630)), ((480, 4), (476, 4)), ((4, 640), (4, 644)), ((17, 13), (5, 3))]


def rows():
    with open(SIZES) as f:
        return json.load(f)


def test_size_table_holds_the_cases_it_must():
    t = {(r["width"], r["height"], r["resize_method"], r["keep_aspect_ratio"]): (r["new_width"], r["new_height"]) for r in rows()
         if (r["target_width"], r["target_height"], r["multiple_of"]) == (630, 476, 14)}
    assert t[(640, 480, "lower_bound", True)] == (630, 476)
    assert t[(637, 476, "lower_bound", True)] == (644, 476) and t[(651, 476, "lower_bound", True)] == (644, 476)
    assert any(r["height"] > r["width"] for r in rows()) and (100, 50, "lower_bound", True) in t
    assert {r["resize_method"] for r in rows()} == {"lower_bound", "upper_bound", "minimal"}
    assert any(not r["keep_aspect_ratio"] for r in rows())


def test_transform_size_equals_the_reference():
    from diffreg_hip.depth_transform2d3d import transform_size
    for r in rows():
        got = transform_size(r["width"], r["height"], r["target_width"], r["target_height"], r["multiple_of"], r["keep_aspect_ratio"],
                             r["resize_method"])
        assert got == (r["new_width"], r["new_height"]) and all(type(v) is int for v in got), (r, got)
    assert transform_size(640, 480) == (630, 476)                        # the defaults are the reference's Compose
    with pytest.raises(ValueError):
        transform_size(640, 480, resize_method="nearest")


@pytest.mark.parametrize("src,dst", CASES)
def test_float64_statement_equals_torch_bicubic_float64(src, dst):
    rng = np.random.default_rng(1000 * src[0] + src[1])
    img = rng.uniform(0.0, 255.0, size=(src[0], src[1], 3))
    got = R.resample(img, dst)
    x = torch.from_numpy(img).permute(2, 0, 1)[None]
    want = F.interpolate(x, size=dst, mode="bicubic", align_corners=False)[0].permute(1, 2, 0).numpy()
    assert want.dtype == np.float64 and got.shape == want.shape
    err = np.abs(got - want).max() / np.abs(want).max()
    print("%s -> %s: float64 statement %.3e relative from torch's float64 bicubic" % (src, dst, err))
    assert err <= 1e-12
    chw = R.transform(img, dst)
    assert chw.shape == (3,) + tuple(dst) and np.array_equal(chw, np.ascontiguousarray(R.normalize(got).transpose(2, 0, 1)))
    if src == dst:
        assert np.array_equal(got, img)                                 # t = 0: the weights are (0, 1, 0, 0)
