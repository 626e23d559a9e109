"""CPU checks of the RANSAC-free rigid estimators: the library binds the twentieth set with the header's argument counts and refuses what it
documents before any launch; tests/lgr_ref.py, the float64 statement the GPU tests lean on, reproduces every output the reference's own
code produced (tests/golden/lgr.npz); every screen of the fixture is re-checked from the stored inputs; the CPU fallbacks of
diffreg_hip.registration equal the statement; the host walk of csrc/lgr_index.h ends clean under ASan + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import lgr_ref as R
from tests.conftest import GOLDEN, ROOT

ALL = R.SCENES + [R.E2E]
NAMES = [s[0] for s in ALL]
NEW = ("dr_lgr_wave_limit", "dr_sc_block", "dr_sc_tile", "dr_weighted_procrustes_f32", "dr_lgr_workspace_bytes", "dr_lgr_f32",
       "dr_spatial_consistency_f32", "dr_sc_row_sums_f32", "dr_sc_leading_eigenvector_workspace_bytes", "dr_sc_leading_eigenvector_f32")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "lgr.npz"))


def scene(gold, name):
    spec = next(s for s in ALL if s[0] == name)
    sc = {k: gold["%s/in_%s" % (name, k)] for k in ("src_knn_points", "tgt_knn_points", "src_masks", "tgt_masks", "score_mat", "global_scores",
                                                    "R", "t")}
    sc.update(name=name, opts=dict(R.OPTS, **spec[3]))
    return sc


def bar(gold, name, key, want):
    """the project's bar: one float32 ulp at the tensor's scale, or 4 x the reference's own float32 deviation from float64"""
    scale = float(np.abs(want).max()) if np.size(want) else 1.0
    return max(float(np.spacing(np.float32(max(scale, 1e-30)))), 4.0 * float(gold["%s/dev_%s" % (name, key)]))


def test_library_binds_the_twentieth_set_with_the_headers_argument_counts():
    from diffreg_hip import lib
    text = open(os.path.join(ROOT, "include", "diffreg_hip.h")).read()
    raw = lib.raw()
    for name in NEW:
        m = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % name, text, re.M)
        assert m, name
        args = m.group(1).strip()
        n = 0 if args == "void" else args.count(",") + 1
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == n, (name, n)
        assert getattr(raw, name).argtypes is not None
    assert raw.dr_lgr_wave_limit() >= 64 and raw.dr_sc_tile() % raw.dr_sc_block() == 0
    assert raw.dr_lgr_workspace_bytes(0, 100) == 0 and raw.dr_lgr_workspace_bytes(2, 100) >= 100 * (8 * 4 + 64)
    assert raw.dr_sc_leading_eigenvector_workspace_bytes(2, 100) >= 100 * 4 + 8


def test_library_refuses_before_any_launch():
    from diffreg_hip import lib
    raw = lib.raw()
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call below is refused on the host
    EINVAL, ENOSUP, EWORKSPACE = -1, -3, -4
    i32 = lambda *v: np.array(v, np.int32)
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    good = i32(0, 4, 10)

    def proc(G=2, n=10, s=fake, off=fake, h=good, T=fake, st=fake):
        return raw.dr_weighted_procrustes_f32(G, n, s, fake, None, off, hp(h), 0.0, 1e-5, -1, T, st, None)
    assert proc(G=0) == 0
    for kw in (dict(h=i32(0, 6, 4)), dict(h=i32(0, 4, 11)), dict(s=None), dict(off=None), dict(T=None), dict(st=None), dict(G=-1), dict(n=-1),
               dict(T=ctypes.c_void_p(4100))):
        assert proc(**kw) == EINVAL, kw

    def lgr(P=2, n=10, s=fake, hc=good, hv=good, ml=3, steps=5, T=fake, ws=fake, wsb=1 << 20):
        return raw.dr_lgr_f32(P, n, s, fake, fake, fake, fake, 10, fake, fake, fake, fake, hp(hc), hp(hv), 0.1, ml, steps, 0.0, 1e-5, T, None, None,
                              None, None, None, fake, ws, wsb, None)
    assert lgr(P=0) == 0
    for kw in (dict(hc=i32(0, 6, 4)), dict(hv=i32(0, 4, 11)), dict(s=None), dict(ml=0), dict(steps=0), dict(steps=65), dict(T=None), dict(P=-1),
               dict(ws=ctypes.c_void_p(4100))):
        assert lgr(**kw) == EINVAL, kw
    assert lgr(ws=None) == EWORKSPACE and lgr(wsb=64) == EWORKSPACE
    assert lgr(P=70000, hc=None, hv=None, wsb=1 << 30) == ENOSUP

    def sums(P=2, q=fake, hq=good, sigma=0.1, out=fake):
        return raw.dr_sc_row_sums_f32(P, 10, q, fake, fake, 10, fake, fake, fake, hp(hq), hp(good), sigma, None, out, fake, None)
    assert sums(P=0) == 0
    for kw in (dict(hq=i32(0, 6, 4)), dict(q=None), dict(sigma=0.0), dict(out=None)):
        assert sums(**kw) == EINVAL, kw
    assert raw.dr_spatial_consistency_f32(2, 10, fake, fake, fake, 10, fake, fake, fake, None, None, 0.1, None, fake, fake, None) == EINVAL

    def eig(P=2, s=fake, mat=None, mo=None, it=10, ws=fake, wsb=1 << 20, h=good):
        return raw.dr_sc_leading_eigenvector_f32(P, 10, s, s, fake, hp(h), 0.1, mat, mo, it, fake, fake, fake, ws, wsb, None)
    assert eig(P=0) == 0
    for kw in (dict(s=None), dict(mat=fake, mo=fake), dict(s=None, mat=fake), dict(it=-1), dict(h=i32(0, 6, 4))):
        assert eig(**kw) == EINVAL, kw
    assert eig(ws=None) == EWORKSPACE and eig(wsb=16) == EWORKSPACE


def test_fixture_says_where_it_comes_from(gold):
    p = str(gold["provenance"])
    assert "torch.Tensor.cuda = identity" in p and "set_default_dtype" in p and "share left out 0" in p
    assert len(R.SCENES) == 11 and os.path.getsize(os.path.join(GOLDEN, "lgr.npz")) < 512 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_scene_passes_every_screen(gold, name):
    sc = scene(gold, name)
    m = R.screens(sc)
    assert m["ok"], m
    assert np.array_equal(np.array([float(m[k]) for k in R.MARGIN_KEYS]), gold[name + "/screens"])
    assert m["eig_iterations"] == int(gold[name + "/eig_iterations"])
    if name == "power_runs_out":
        assert not m["eig_stopped"] and m["eig_iterations"] == R.EIG_ITERS
    regenerated = R.make_scene(next(s for s in ALL if s[0] == name), int(gold[name + "/seed"]))
    assert all(np.array_equal(regenerated[k], sc[k]) for k in ("src_knn_points", "score_mat", "src_masks"))


def test_scenes_cover_what_the_fixture_promises(gold):
    lens = lambda name: [b - a for a, b in R.chunks_of(R.forward(scene(gold, name))[0], 1)]
    assert {2, 3, 4} <= set(lens("min_local_edges")) and lens("wave_edges") == [63, 64, 65]
    assert R.forward(scene(gold, "no_valid_chunk"))[6]["best_chunk"] == -1
    assert len(R.forward(scene(gold, "one_valid_chunk"))[6]["chunks"]) == 1
    assert min(gold[n + "/screens"][R.MARGIN_KEYS.index("min_det")] for n in NAMES) < 0          # the sign fix is exercised
    assert len(R.forward(scene(gold, "max_global"))[5]) == 30


@pytest.mark.parametrize("name", NAMES)
def test_statement_reproduces_the_reference(gold, name):
    sc = scene(gold, name)
    b, i, j, vs, vt, vw, r = R.forward(sc)
    close = lambda got, key: np.testing.assert_allclose(np.asarray(got, np.float64), gold["%s/%s" % (name, key)], rtol=0,
                                                        atol=bar(gold, name, key, gold["%s/%s" % (name, key)]), err_msg=key)
    assert np.array_equal(vs.astype(np.float64), gold[name + "/src_corr"]) and np.array_equal(vt.astype(np.float64), gold[name + "/tgt_corr"])
    close(vw, "corr_scores")
    close(r["transform"], "transform")
    close(R.weighted_procrustes(vs, vt, vw), "procrustes")
    close(R.weighted_procrustes(vs, vt), "procrustes_unweighted")
    mat = R.spatial_consistency(vs, vt)
    if len(vw) <= R.DENSE_MAX:
        close(mat, "sc")
        h = max(len(vw) // 2, 1)
        close(R.spatial_consistency(vs[:h], vt[:h], vs, vt), "cross_sc")
    close(mat.sum(1), "sc_counts")
    k = min(R.SCF_K, len(vw))
    assert np.array_equal(np.argsort(-mat.sum(1), kind="stable")[:k], gold[name + "/scf_topk"])
    vec, it, _ = R.leading_eigenvector(mat)
    assert it == int(gold[name + "/eig_iterations"])
    close(vec, "eig")


def test_tie_goes_to_the_lowest_chunk():
    src, tgt, w, ids = R.tie_scene()
    r = R.lgr(src, tgt, w, ids, 0.1, 3, 2)
    assert list(r["chunk_counts"]) == [4, 4] and r["best_chunk"] == 0
    from diffreg_hip import registration as G
    o = G.local_to_global_registration_pairs(torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(w), torch.from_numpy(ids),
                                             torch.tensor([0, 8], dtype=torch.int32), 0.1, 3, 2)
    assert int(o["best_chunk"][0]) == 0
    np.testing.assert_allclose(o["transform"][0].numpy(), r["transform"], atol=1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_cpu_fallbacks_equal_the_statement(gold, name):
    from diffreg_hip import registration as G
    sc = scene(gold, name)
    o = sc["opts"]
    t = torch.from_numpy
    b, i, j, vs, vt, vw, r = R.forward(sc)
    mod = G.LocalGlobalRegistration(o["k"], o["radius"], o["mutual"], o["threshold"], o["use_dustbin"], o["use_global_score"], o["use_logits"],
                                    o["min_local"], o["max_global"], o["steps"])
    gs, gt, gw, T = mod(t(sc["src_knn_points"]), t(sc["tgt_knn_points"]), t(sc["src_masks"]), t(sc["tgt_masks"]), t(sc["score_mat"]),
                        t(sc["global_scores"]))
    assert np.array_equal(gs.numpy(), vs) and np.array_equal(gt.numpy(), vt)
    np.testing.assert_allclose(gw.numpy(), vw, rtol=0, atol=2.4e-7)          # torch's and numpy's float32 exp differ by an ulp below 1
    np.testing.assert_allclose(T.numpy(), r["transform"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(G.weighted_procrustes(t(vs), t(vt), t(vw)).numpy(), R.weighted_procrustes(vs, vt, vw), rtol=0, atol=2e-6)
    np.testing.assert_allclose(G.WeightedProcrustes()(t(vs)[None], t(vt)[None]).numpy()[0], R.weighted_procrustes(vs, vt), rtol=0, atol=2e-6)
    mat = R.spatial_consistency(vs, vt, dtype=np.float32)
    # torch's CPU float32 arithmetic may contract where numpy's does not: two float32 evaluations of one value (lgr_ref.sc_bar)
    per = R.sc_bar(R.SIGMA, vs, vt)
    np.testing.assert_allclose(G.spatial_consistency(t(vs), t(vt), R.SIGMA).numpy(), mat, rtol=0, atol=per)
    np.testing.assert_allclose(G.cross_spatial_consistency(t(vs[:3]), t(vt[:3]), t(vs), t(vt), R.SIGMA).numpy(), mat[:3], rtol=0, atol=per)
    np.testing.assert_allclose(G.spatial_consistency_counts(t(vs), t(vt), R.SIGMA).numpy(), mat.astype(np.float64).sum(1), rtol=0,
                               atol=len(vw) * per)
    k = min(R.SCF_K, len(vw))
    assert np.array_equal(G.SpatialConsistencyFiltering(k, R.SIGMA)(t(vs), t(vt)).numpy(), gold[name + "/scf_topk"])
    vec, its = G.leading_eigenvector(t(vs), tgt_points=t(vt), sigma=R.SIGMA, num_iterations=R.EIG_ITERS, return_iterations=True)
    assert int(its) == int(gold[name + "/eig_iterations"])
    np.testing.assert_allclose(vec.numpy(), R.leading_eigenvector(R.spatial_consistency(vs, vt))[0], rtol=0, atol=2e-6)
    vec2 = G.leading_eigenvector(t(mat), num_iterations=R.EIG_ITERS)
    np.testing.assert_allclose(vec2.numpy(), vec.numpy(), rtol=0, atol=2e-6)


def test_python_refusals():
    from diffreg_hip import registration as G
    with pytest.raises(AssertionError):
        G.leading_eigenvector(torch.eye(3), method="lanczos")
    v = G.leading_eigenvector(torch.diag(torch.tensor([1.0, 3.0, 2.0])), method="torch")
    assert abs(abs(float(v[1])) - 1.0) < 1e-6


def test_index_walk_ends_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for tools/lgr_index_check.cpp"
    exe = str(tmp_path / "lgr_index_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "diff-reg_amd", "csrc"), os.path.join(ROOT, "tools", "lgr_index_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "lgr_index_check: ok" in r.stdout, r.stdout + r.stderr
