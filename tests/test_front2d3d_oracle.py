"""CPU checks of the 2D-3D geometry head: the restatement of tests/front2d3d_ref.py pinned to the reference's own outputs
(tests/golden/front2d3d.npz, minted by tools/golden/make_golden_front2d3d.py from vision3d.ops.back_project, vision3d.ops.render and
MATR2D3D.back_project_depth), the fixture rules (the 1e-3 margin of every z from 0 and from the depth limit), create_meshgrid's definition, and
the ABI boundary of the new entries.  create_meshgrid calls `.cuda()` in the reference and has no golden: it is pinned to its definition,
cartesian_prod of arange / linspace."""
import os
import re

import numpy as np
import pytest

from tests import front2d3d_ref as F
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "front2d3d.npz"))
NEW = ("dr_back_project_f32", "dr_render_f32", "dr_resize_tokens_f32", "dr_resize_tokens_backward_f32", "dr_rows_normalize_chw_f32",
       "dr_rows_normalize_chw_backward_f32", "dr_rows_normalize_chw_backward_rows_f32")


def test_fixture_rules_hold():
    """every z at least 1e-3 away from 0 and from the limit (exact zeros aside), every clamp of render decided, every kind of depth present"""
    assert F.fixture_rules() == []


@pytest.mark.parametrize("name", list(F.BACK_PROJECT_CASES))
def test_back_project_restatement_against_the_reference(name):
    kw = F.BACK_PROJECT_CASES[name]
    c = F.make_back_project(**kw)
    for k in ("depth", "intrinsics", "a", "b"):
        assert np.array_equal(np.asarray(c[k]), G["%s_in_%s" % (name, k)]), k
    for tag, dt, tol in (("64", np.float64, 1e-14), ("32", np.float32, 1e-6)):
        pts, mask = F.back_project(c["depth"][0], c["intrinsics"][0], kw["mode"], c["a"], c["b"], F.DEPTH_LIMIT, dt)
        assert np.array_equal(mask, G["%s_mask%s" % (name, tag)])
        assert F.rel_dev(pts, G["%s_points%s" % (name, tag)]) <= tol, (name, tag)
    assert np.array_equal(G[name + "_mask32"], G[name + "_mask64"])


@pytest.mark.parametrize("name", list(F.RENDER_CASES))
def test_render_restatement_against_the_reference(name):
    c = F.make_render(**F.RENDER_CASES[name])
    assert np.array_equal(c["points"], G[name + "_in_points"]) and np.array_equal(c["intrinsics"], G[name + "_in_intrinsics"])
    assert (c["extrinsics"] is None) == (name + "_in_extrinsics" not in G.files)
    for tag, dt, tol in (("64", np.float64, 1e-13), ("32", np.float32, 1e-4)):      # float32: the matrix product's order of summation
        pix, z = F.render(c["points"], c["intrinsics"], c["extrinsics"], dt)
        assert F.rel_dev(pix, G["%s_pixels%s" % (name, tag)]) <= tol, (name, tag)
        assert F.rel_dev(z, G["%s_depth%s" % (name, tag)]) <= tol, (name, tag)


def test_meshgrid_definition():
    for (h, w) in F.MESHGRID_SIZES:
        g = F.create_meshgrid(h, w)
        assert g.dtype == np.int64 and g.shape == (h, w, 2)
        assert g[h - 1, w - 1].tolist() == [h - 1, w - 1] and g[0, w - 1].tolist() == [0, w - 1]
        f = F.create_meshgrid(h, w, flatten=True, centering=True)
        assert f.dtype == np.float32 and f.shape == (h * w, 2) and f[1].tolist() == [0.5, 1.5]


def test_new_entries_are_bound_and_declared():
    from diffreg_hip import lib
    header = open(os.path.join(ROOT, "include", "diffreg_hip.h")).read()
    # additions leave the number alone (an older check pins it); the binding and the header agree, whatever it is
    assert lib.raw().dr_version() == lib.ABI_VERSION >= 700 and re.search(r"#define DR_ABI_VERSION %d\b" % lib.ABI_VERSION, header)
    for name in NEW:
        assert name in lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    # argument checks run without a GPU
    r = lib.raw()
    assert r.dr_rows_normalize_chw_f32(257, 4, None, None, None) == -3          # DR_ENOSUP
    assert r.dr_rows_normalize_chw_f32(-1, 4, None, None, None) == -1           # DR_EINVAL
    assert r.dr_rows_normalize_chw_f32(4, 4, None, None, None) == -1            # NULL pointers
    assert r.dr_resize_tokens_f32(2, -1, 3, 2, 2, None, None, None) == -1
    assert r.dr_back_project_f32(2, 2, None, None, 0, 1.0, 0.0, None, None, 0, 0.0, None, None, None, None) == -1
    assert r.dr_render_f32(-1, None, None, None, 1e-8, None, None, None) == -1


def test_public_names_and_defaults_are_the_reference_s():
    import inspect
    from diffreg_hip import front2d3d as fr
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    assert sig(fr.back_project) == [("depth_mat", inspect._empty), ("intrinsics", inspect._empty), ("scaling_factor", 1000.0),
                                    ("depth_limit", None), ("transposed", False), ("return_mask", False)]
    assert sig(fr.render) == [("points", inspect._empty), ("intrinsics", inspect._empty), ("extrinsics", None), ("rounding", True),
                              ("return_depth", False), ("eps", 1e-8)]
    assert sig(fr.create_meshgrid)[:5] == [("height", inspect._empty), ("width", inspect._empty), ("normalized", False), ("flatten", False),
                                           ("centering", False)]
    assert sig(fr.back_project_depth)[2:4] == [("scaling_factor_a", 1000.0), ("scaling_factor_b", 1000.0)]
