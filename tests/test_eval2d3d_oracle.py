"""CPU checks of the 2D-3D evaluation metrics: the restatement of tests/eval2d3d_ref.py pinned to the reference's own outputs
(tests/golden/eval2d3d.npz, minted by tools/golden/make_golden_eval2d3d.py), the fixture rules, summarize() against the reference's SummaryBoard
arithmetic, and the ABI boundary of the new entries."""
import os
import re

import numpy as np
import pytest

from tests import eval2d3d_ref as F
from tests.conftest import ROOT

G = np.load(os.path.join(ROOT, "tests", "golden", "eval2d3d.npz"))
NEW = ("dr_sparse_corr_eval_workspace_bytes", "dr_sparse_corr_eval_i64", "dr_corr_eval_workspace_bytes", "dr_corr_eval_f32",
       "dr_registration_eval_workspace_bytes", "dr_registration_eval_f64")


def same(a, b, tol):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol * max(1.0, abs(b))


@pytest.mark.parametrize("name", list(F.SCENES))
def test_scenes_are_the_fixtures_inputs_and_keep_the_rules(name):
    s = F.make_scene(**F.SCENES[name])
    for k in F.INPUT_KEYS:
        assert np.array_equal(np.asarray(s[k]), G["%s_in_%s" % (name, k)]), k
    assert int(G["%s_in_num_corr" % name]) == (-1 if s["num_corr"] is None else s["num_corr"])
    assert F.fixture_rules(s) == []


@pytest.mark.parametrize("name", list(F.SCENES))
def test_restatement_against_the_reference(name):
    """float64 restatement against the reference's float64 run to 1e-12 (summation order only), float32 against its float32 run to 1e-5; every
    integer count equal in both; EvalFunction's IR, a float32 mean in either run of the reference, bit-equal after the same rounding"""
    s = {k: G["%s_in_%s" % (name, k)] for k in F.INPUT_KEYS}
    nc = int(G["%s_in_num_corr" % name])
    s["num_corr"] = None if nc < 0 else nc
    for tag, dt, tol in (("64", np.float64, 1e-12), ("32", np.float32, 1e-5)):
        o = F.restate(s, dt)
        for k in F.REAL_KEYS:
            ref = float(G["%s_%s%s" % (name, k, tag)])
            if k == "ev_IR":
                assert np.float32(o[k]) == np.float32(ref), (k, tag, o[k], ref)
            elif k == "ev_PIR" and tag == "32":
                assert same(o[k], ref, 1e-6), (k, tag, o[k], ref)       # the reference's float32 mean of a 0 / 1 matrix
            elif k in ("rre", "ev_rre") and tag == "32":
                assert abs(o[k] - ref) <= 0.05, (k, tag, o[k], ref)     # acos of a float32 trace: 1e-7 at x = cos(1.5 deg) is 2e-4 rad
            else:
                assert same(o[k], ref, tol), (k, tag, o[k], ref)
        for k in F.INT_KEYS:
            assert o[k] == int(G["%s_%s" % (name, k)]), (k, tag)


def test_the_clip_cases_decide_by_the_clip():
    for name, want in (("clip0", 0.0), ("clip180", 180.0)):
        for tag in ("32", "64"):
            assert float(G["%s_rre%s" % (name, tag)]) == want and float(G["%s_ev_rre%s" % (name, tag)]) == want
        s = F.make_scene(**F.SCENES[name])
        x = 0.5 * ((s["estimated_transform"][:3, :3] * s["transform"][:3, :3]).sum() - 1.0)
        assert abs(x) > 1.0


def test_mutants_differ_from_the_restatement():
    s = F.make_scene(**F.SCENES["clip180"])
    a = (s["img_num_nodes"], s["pcd_num_nodes"], s["img_node_corr_indices"], s["pcd_node_corr_indices"], s["gt_img_node_corr_indices"],
         s["gt_pcd_node_corr_indices"])
    assert F.evaluate_sparse_correspondences(*a)["precision"] != F.evaluate_sparse_correspondences(*a, mutant="dup_twice")["precision"]
    ov = np.array([0.3, 0.5], dtype=np.float32)
    assert F.coarse_precision(2, 2, [0], [0], [0, 1], [0, 1], ov, 0.3)[0] == 0.0
    assert F.coarse_precision(2, 2, [0], [0], [0, 1], [0, 1], ov, 0.3, mutant="ge_overlap")[0] == 1.0


def test_summarize_against_the_reference_summary_board():
    """eval.py:205-330 on a three-scene table: scene means, the mean of the scene means, medians of RRE / RTE over the recalled pairs"""
    from diffreg_hip import metrics2d3d as M
    r = M.summarize(F.make_table(), F.CFG["inlier_ratio_threshold"])
    keys = [k[len("summary_"):] for k in G.files if k.startswith("summary_")]
    assert len(keys) == 14
    for k in keys:
        assert same(r[k], float(G["summary_" + k]), 1e-14), (k, r[k], float(G["summary_" + k]))
    assert set(r["scenes"]) == {"kitchen", "office", "stairs"}
    # a scene without a recalled pair: NaN, as np.mean / np.median of nothing
    t = {"a": [dict(PIR=0.2, IR=0.3, OR=0.5, RR=0.0, RRE=1.0, RTE=0.1)]}
    assert np.isnan(M.summarize(t)["median_RRE"]) and M.summarize(t)["RR"] == 0.0


def test_new_entries_are_bound_and_declared():
    from diffreg_hip import lib
    header = open(os.path.join(ROOT, "include", "diffreg_hip.h")).read()
    assert re.search(r"#define DR_ABI_VERSION 700\b", header) and "0.7.0" in header
    assert lib.ABI_VERSION == 700 and lib.raw().dr_version() == 700
    for name in NEW:
        assert name in lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    # the size queries run without a GPU: the stated limits
    assert lib.raw().dr_sparse_corr_eval_workspace_bytes(1530, 4096) == (2 * 1530 * 128 + 2 * 128 + 2 * 48 + 4) * 4
    assert lib.raw().dr_sparse_corr_eval_workspace_bytes(8193, 8193) == 0
    assert lib.raw().dr_corr_eval_workspace_bytes(16384) > 0 and lib.raw().dr_corr_eval_workspace_bytes(16385) == 0
