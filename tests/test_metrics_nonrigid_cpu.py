"""CPU checks of the non-rigid evaluation: the library binds the nineteenth set and refuses what it documents before any launch (no GPU is
needed for that); tests/metrics_nonrigid_ref.py, the statement the GPU edge tests lean on, reproduces every array the reference's own
functions produced (tests/golden/metrics_nonrigid.npz); the fixture's scenes pass both screens with no query excluded; the host walk of
csrc/knn_index.h ends clean under ASan + UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import metrics_nonrigid_ref as R
from tests.conftest import GOLDEN, ROOT

NAMES = [s[0] for s in R.SCENES]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "metrics_nonrigid.npz"))


def scene(gold, name):
    return {k: gold["%s/in_%s" % (name, k)] for k in ("q", "s", "feats", "transform", "flow", "pred", "tgt_c", "s_moved", "test")}


def test_library_binds_the_nineteenth_set():
    from diffreg_hip import lib
    raw = lib.raw()
    for name in ("dr_knn_points_f32", "dr_nn_stats_f32", "dr_nn_stats_workspace_bytes", "dr_flow_metrics_f32", "dr_flow_metrics_workspace_bytes"):
        assert name in lib.SIGNATURES and getattr(raw, name).argtypes is not None, name
    assert raw.dr_knn_points_max_k() == 16
    assert raw.dr_knn_points_tile() > 0 and raw.dr_knn_points_block() > 0
    assert raw.dr_knn_points_tile() % raw.dr_knn_points_block() == 0
    assert raw.dr_nn_stats_workspace_bytes(2, 1000) >= (1000 // raw.dr_knn_points_block() + 2) * 32
    assert raw.dr_nn_stats_workspace_bytes(0, 1000) == 0 and raw.dr_flow_metrics_workspace_bytes(1, 4097) >= (4097 // 256 + 1) * 48


def test_library_refuses_before_any_launch():
    from diffreg_hip import lib
    raw = lib.raw()
    fake = ctypes.c_void_p(4096)                             # never dereferenced: every call below is refused on the host
    EINVAL, ENOSUP, EWORKSPACE = -1, -3, -4
    i32 = lambda *v: np.array(v, np.int32)
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    good = i32(0, 4, 10)

    def knn(P=2, nq=10, q=fake, qo=fake, ns=10, s=fake, so=fake, hq=good, hs=good, k=3, st=fake):
        return raw.dr_knn_points_f32(P, nq, q, qo, ns, s, so, hp(hq), hp(hs), k, fake, fake, st, None)
    assert knn(P=0) == 0
    for kw in (dict(k=0), dict(k=17), dict(k=-1), dict(hq=i32(0, 6, 4)), dict(hs=i32(0, 11, 10)), dict(hq=i32(-1, 4, 10)), dict(hs=i32(0, 4, 11)),
               dict(q=None), dict(s=None), dict(qo=None), dict(so=None), dict(st=None), dict(P=-1), dict(nq=-1), dict(ns=-1)):
        assert knn(**kw) == EINVAL, kw
    assert knn(P=70000, hq=None, hs=None) == ENOSUP

    def stats(P=2, nq=10, q=fake, ns=10, s=fake, hq=good, hs=good, out=fake, ws=fake, wsb=1 << 20):
        return raw.dr_nn_stats_f32(P, nq, q, fake, ns, s, fake, hp(hq), hp(hs), 0.1, out, fake, ws, wsb, None)
    for kw in (dict(hq=i32(0, 6, 4)), dict(q=None), dict(s=None), dict(out=None), dict(ws=ctypes.c_void_p(4100))):
        assert stats(**kw) == EINVAL, kw
    assert stats(ws=None) == EWORKSPACE and stats(wsb=16) == EWORKSPACE

    def flow(P=2, n=10, a=fake, b=fake, ho=good, rot=None, trn=None, out=fake, ws=fake, wsb=1 << 20):
        return raw.dr_flow_metrics_f32(P, n, a, b, fake, hp(ho), None, rot, trn, 0.1, 0.1, 0.2, 0.2, -1.0, -1.0, 1e-20, out, fake, ws, wsb, None)
    assert flow(P=0) == 0
    for kw in (dict(ho=i32(0, 6, 4)), dict(a=None), dict(b=None), dict(out=None), dict(rot=fake), dict(trn=fake), dict(n=-1)):
        assert flow(**kw) == EINVAL, kw
    assert flow(ws=None) == EWORKSPACE


def test_python_refusals():
    import torch
    from diffreg_hip import metrics_nonrigid as M
    pts = torch.zeros(4, 3)
    with pytest.raises(TypeError, match="on the GPU"):
        M.knn_points(pts, pts, 1)
    with pytest.raises(TypeError):
        M.knn_points(pts.double(), pts, 1)
    with pytest.raises(ValueError):
        M.knn(pts, torch.zeros(40, 3), 9, dilation=2)        # (9 - 1) * 2 + 1 = 17 neighbours
    with pytest.raises(TypeError):
        M.evaluate_nonrigid_pairs([pts], [pts], [pts], [pts])   # the thresholds have no defaults


def test_vector_starts_with_the_shard_slots():
    from diffreg_hip import metrics_nonrigid as M, shard
    assert M.VECTOR_NAMES[:5] == shard.METRIC_NAMES
    assert M.VECTOR_NAMES[5:] == ("sum_EPE", "sum_AccS", "sum_AccR", "sum_outlier", "sum_chamfer", "sum_coverage")


def test_fixture_says_where_it_comes_from(gold):
    p = str(gold["provenance"])
    assert "float64 brute-force kNN" in p and "not claimed" in p
    assert sum(d > 0 for _, _, _, d in R.SCENES) == 2 and len(R.SCENES) == 10


@pytest.mark.parametrize("name", NAMES)
def test_scene_passes_both_screens(gold, name):
    sc = scene(gold, name)
    _, Q, S, dup = next(s for s in R.SCENES if s[0] == name)
    assert sc["q"].shape == (Q, 3) and sc["s"].shape == (S, 3) and sc["q"].dtype == np.float32
    gap, margin = R.screen_gaps(sc["q"], sc["s"]), R.screen_thresholds(sc)       # over every query: none is excluded
    assert gap >= R.SCREEN_GAP and margin >= R.SCREEN_GAP, (gap, margin)
    assert gap == gold[name + "/screens"][0] and margin == gold[name + "/screens"][1]
    if dup:
        d = np.sort(np.sqrt(R.d2_matrix(sc["s"][:dup], sc["s"], np.float64)), axis=1)
        assert np.all(d[:, 1] == 0.0)                        # the duplicates are exact


@pytest.mark.parametrize("name", NAMES)
def test_statement_reproduces_the_reference(gold, name):
    sc = scene(gold, name)
    q, s, T = sc["q"], sc["s"], sc["transform"]
    close = lambda got, key: np.testing.assert_allclose(np.asarray(got, np.float64), gold["%s/%s" % (name, key)], rtol=0, atol=1e-12, err_msg=key)
    for tag, kw in R.KNN_CASES:
        dist, idx = R.knn(q, s, **kw)
        want = gold["%s/knn_%s_idx" % (name, tag)]
        assert idx.shape == want.shape and np.array_equal(idx, want), tag
        close(dist, "knn_%s_dist" % tag)
    close(R.knn_interpolate(q, s, sc["feats"], 3), "interp")
    close(R.knn_interpolate(q, s, sc["feats"], 3, distance_limit=R.INTERP_LIMIT), "interp_limit")
    # the six ratios are `.float().mean()` in the reference (metrics.py:283 ...): float32 quotients of the same counts in either run
    f32 = lambda got, key: close(np.float32(got), key)
    f32(R.nonrigid_inlier_ratio(q, sc["tgt_c"], sc["flow"], T, R.RADIUS), "nir")
    f32(R.nonrigid_inlier_ratio(q, sc["tgt_c"], sc["flow"], None, R.RADIUS), "nir_no_transform")
    f32(R.nonrigid_fmr(s, sc["s_moved"], q, sc["flow"], sc["test"], T, R.RADIUS, R.NFMR_LIMIT)[0], "nfmr")
    f32(R.scene_flow_accuracy(sc["pred"], sc["flow"], *R.STRICT), "acc_strict")
    f32(R.scene_flow_accuracy(sc["pred"], sc["flow"], *R.RELAXED), "acc_relaxed")
    f32(R.scene_flow_outlier_ratio(sc["pred"], sc["flow"], *R.OUTLIER), "outlier")
    f32(R.scene_flow_outlier_ratio(sc["pred"], sc["flow"], *R.OUTLIER_NONE), "outlier_none")
    f32(R.corr_coverage(q, s, R.COVERAGE_LIMIT), "coverage")
    close(R.chamfer_distance(q, s), "chamfer")
    close(R.chamfer_distance(q, s, squared=True), "chamfer_squared")
    o = R.flow_metrics(sc["pred"], sc["flow"])
    close(o[1] / o[0], "epe")
    # counts are the same integers in the device's float32 rule: the screens keep every compared quantity 1e-5 from its threshold
    for kw in (dict(strict=R.STRICT, relaxed=R.RELAXED, outlier=R.OUTLIER), dict(outlier=R.OUTLIER_NONE)):
        a, b = R.flow_metrics(sc["pred"], sc["flow"], **kw), R.flow_metrics(sc["pred"], sc["flow"], dtype=np.float32, **kw)
        assert np.array_equal(a[[0, 2, 3, 4, 5]], b[[0, 2, 3, 4, 5]])
    assert np.array_equal(R.knn_points(q, s, min(16, len(s)))[1], R.knn_points(q, s, min(16, len(s)), np.float32)[1])


def test_statement_rules():
    s = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [0, 0, 0]], np.float32)
    q = np.array([[0, 0, 0], [np.nan, 0, 0]], np.float32)
    dist, idx, st = R.knn_points(q, s, 6, np.float32)
    assert list(idx[0]) == [5, 0, 1, 2, -1, -1] and st == R.ST_NONFINITE        # ties to the lower index; NaN / Inf supports never
    assert np.all(idx[1] == -1) and np.all(np.isinf(dist[1])) and np.all(np.isinf(dist[0, 4:]))
    assert np.array_equal(R.knn_points(q[:1], s[:0], 2)[1], [[-1, -1]])
    d = np.arange(130, dtype=np.float32) / 7
    got = R.ordered_nn_stats(d, np.zeros(130, np.int64), 5.0, 64)
    assert got[0] == 130 and got[3] == (d < 5).sum() and abs(got[1] - d.astype(np.float64).sum()) < 1e-9
    o = R.flow_metrics(np.zeros((2, 3)), np.array([[0, 0, 0], [0, 0, 1e-3]]), strict=(1e-4, 0.5), outlier=(None, 0.5), dtype=np.float32)
    assert list(o) == [2, np.float32(1e-3), 1, 2, 1, 1]     # target = 0 with |e| = 0: rel = 0 / eps = 0


def test_index_walk_ends_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for tools/knn_index_check.cpp"
    exe = str(tmp_path / "knn_index_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "diff-reg_amd", "csrc"), os.path.join(ROOT, "tools", "knn_index_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "knn_index_check: ok" in r.stdout, r.stdout + r.stderr
