"""CPU checks of the point-to-point ICP: the library binds the twenty-first set with the header's argument counts, its size query equals the
carve of csrc/icp_index.h and it refuses what it documents before any launch; tests/icp_ref.py, the statement the GPU tests lean on, recovers
a known pose and names the partners a k-d tree names; every screen of tests/golden/icp.npz is re-checked from the stored inputs; the CPU paths
of diffreg_hip.registration equal the statement; the host walk of csrc/icp_index.h ends clean under ASan + UBSan.  Parity with Open3D itself
is not claimed anywhere: the fixture holds the float64 statement's outputs."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import icp_ref as R
from tests.conftest import GOLDEN, ROOT

NAMES = [s[0] for s in R.SCENES]
FIXED = [s[0] for s in R.SCENES if s[1] == "fixed"]
NEW = ("dr_icp_p2p_workspace_bytes", "dr_icp_p2p_f32", "dr_grid_subsample_open3d_f32")
EINVAL, ENOSUP, EWORKSPACE = -1, -3, -4


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "icp.npz"))


def scene(gold, name):
    spec = next(s for s in R.SCENES if s[0] == name)
    sc = {k: gold["%s/in_%s" % (name, k)] for k in ("src", "tgt", "s_off", "t_off", "init", "gt")}
    sc.update(name=name, kind=spec[1], r=spec[3], its=spec[4], opts=spec[5])
    return sc


def refusals(raw):
    """every documented refusal of dr_icp_p2p_f32, before any launch: the pointers are never dereferenced (shared with the GPU tests)"""
    fake = ctypes.c_void_p(4096)
    i32 = lambda *v: np.array(v, np.int32)
    hp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(P=2, ns=10, nt=12, src=fake, so=fake, hs=i32(0, 4, 10), ht=i32(0, 5, 12), init=None, r=0.1, it=5, rf=1e-6, rr=1e-6, T=fake,
             fit=fake, st=fake, ws=fake, wsb=1 << 24):
        return raw.dr_icp_p2p_f32(P, ns, src, so, nt, fake, fake, hp(hs), hp(ht), init, r, it, rf, rr, T, fit, fake, fake, None, st, ws, wsb, None)
    assert call(P=0) == 0
    for kw in (dict(P=-1), dict(ns=-1), dict(nt=-1), dict(it=-1), dict(it=4097), dict(r=0.0), dict(r=-1.0), dict(r=float("inf")),
               dict(r=float("nan")), dict(rf=-1.0), dict(rr=float("nan")), dict(src=None), dict(so=None), dict(T=None), dict(fit=None),
               dict(st=None), dict(hs=i32(0, 6, 4)), dict(hs=i32(0, 4, 11)), dict(ht=i32(-1, 5, 12)), dict(T=ctypes.c_void_p(4100)),
               dict(init=ctypes.c_void_p(4100)), dict(ws=ctypes.c_void_p(4100))):
        assert call(**kw) == EINVAL, kw
    need = raw.dr_icp_p2p_workspace_bytes(2, 10, 12)
    assert call(ws=None) == EWORKSPACE and call(wsb=need - 1) == EWORKSPACE and call(wsb=0) == EWORKSPACE
    assert call(P=65536, hs=None, ht=None, wsb=1 << 40) == ENOSUP
    assert call(ns=(2 ** 31 - 1) // 3 + 1, hs=None, wsb=1 << 40) == ENOSUP


def test_library_binds_the_twenty_first_set_with_the_headers_argument_counts():
    from diffreg_hip import lib
    text = open(os.path.join(ROOT, "include", "diffreg_hip.h")).read()
    for name in NEW:
        m = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % name, text, re.M)
        assert m, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
        assert getattr(lib.raw(), name).argtypes is not None
    assert "#define DR_ABI_VERSION 700" in text and "not claimed" in text.lower()


def test_size_query_equals_the_carve():
    from diffreg_hip import lib
    raw = lib.raw()
    a256 = lambda b: (b + 255) & ~255
    pow2 = lambda n: 1 << max(n - 1, 0).bit_length()

    def carve(P, ns, nt):                                    # icp_index.h: origin, keys, vals, sorted, partial, done
        if P <= 0:
            return 0
        pad = pow2(nt) if nt > 0 else 0
        return (a256(P * 16) + a256(pad * 8) + a256(pad * 4) + a256(max(nt, 0) * 16) + a256((max(ns, 0) // 64 + P) * 17 * 8) + a256(P * 4))
    for P, ns, nt in ((0, 5, 5), (1, 0, 0), (1, 1, 1), (1, 63, 64), (1, 64, 65), (3, 65, 1025), (8, 240000, 240000), (65535, 70000, 3)):
        assert raw.dr_icp_p2p_workspace_bytes(P, ns, nt) == carve(P, ns, nt), (P, ns, nt)


def test_library_refuses_before_any_launch():
    from diffreg_hip import lib
    refusals(lib.raw())
    raw, fake = lib.raw(), ctypes.c_void_p(4096)
    assert raw.dr_grid_subsample_open3d_f32(10, 1, fake, fake, 0.0, fake, fake, fake, fake, fake, 1 << 20, None) == EINVAL
    assert raw.dr_grid_subsample_open3d_f32(-1, 1, fake, fake, 0.1, fake, fake, fake, fake, fake, 1 << 20, None) == EINVAL


def test_statement_recovers_an_exact_rigid_copy_in_float64():
    rng = np.random.default_rng(5)
    src = rng.uniform(0, 1, (400, 3))
    G = R.pose([1, 2, 3], 25.0, [0.3, -0.2, 0.1])
    tgt = src @ G[:3, :3].T + G[:3, 3]
    init = R.pose([3, 1, -2], 2.0, [0.01, -0.01, 0.005]) @ G             # inside the basin: the nearest target is the row's own copy
    r = R.icp(src, tgt, init, 0.15, 30, 0.0, 0.0, np.float64)
    assert r["iterations"] == 30 and r["status"] == 0 and np.array_equal(r["corr"], np.arange(400))
    assert np.abs(r["transform"] - G).max() < 1e-9 and float(r["fitness"]) == 1.0 and float(r["rmse"]) < 1e-9
    assert R.icp(src, tgt, init, 0.15, 0, 0.0, 0.0)["iterations"] == 0
    far = R.icp(src, tgt + 50.0, init, 0.15, 5, 0.0, 0.0)
    assert far["status"] == R.ST_EMPTY and far["iterations"] == 0 and np.array_equal(far["transform"], init)
    line = np.stack([np.arange(6.0), np.zeros(6), np.zeros(6)], 1)
    assert R.icp(line + [0.01, 0.02, 0.0], line, None, 0.5, 1, 0.0, 0.0)["status"] == R.ST_DEGENERATE


def test_fixture_says_where_it_comes_from(gold):
    p = str(gold["provenance"])
    assert "float64 statement" in p and "parity with Open3D itself is not claimed" in p
    assert len(R.SCENES) == 10 and os.path.getsize(os.path.join(GOLDEN, "icp.npz")) < 512 * 1024
    for name in NAMES:
        sc = scene(gold, name)
        assert np.diff(sc["s_off"]).max() <= 600 and np.diff(sc["t_off"]).max() <= 700


@pytest.mark.parametrize("name", NAMES)
def test_scene_passes_every_screen_and_its_stored_margins_hold(gold, name):
    sc = scene(gold, name)
    m, res, _ = R.screens(sc)
    assert m["ok"], m
    assert np.array_equal(np.array([m["gap"], m["edge"], m["wall"]]), gold[name + "/screens"])
    assert min(m["gap"], m["edge"], m["wall"]) >= R.GAP
    again = R.make_scene(next(s for s in R.SCENES if s[0] == name), int(gold[name + "/seed"]))
    assert all(np.array_equal(again[k], sc[k]) for k in ("src", "tgt", "init", "s_off", "t_off"))
    if sc["kind"] == "converge":
        assert [r["iterations"] for r in res] == list(gold[name + "/iterations"]) and res[0]["iterations"] < sc["its"]
        np.testing.assert_array_equal(np.array([r["transform"] for r in res]), gold[name + "/transform"])
    elif sc["kind"] == "fixed":
        np.testing.assert_array_equal(np.array([r["transform"] for r in res]), gold[name + "/transform"][-1])
        assert gold[name + "/corr"].shape == (sc["its"] + 1, len(sc["src"]))


def test_scenes_cover_what_the_fixture_promises(gold):
    assert len(scene(gold, "two_pairs")["s_off"]) == 3
    shell = gold["outlier_shell/corr"][-1]
    assert (shell[-60:] == -1).all() and (shell[:-60] >= 0).mean() > 0.9
    part = gold["partial_overlap/corr"][-1]
    assert 0.3 < (part >= 0).mean() < 0.9
    assert gold["two_scales/scale0_src"].shape[0] < gold["two_scales/scale1_src"].shape[0] < 600
    for name in FIXED:                                       # the loop moved every scene towards its planted pose
        T, gt = gold[name + "/transform"], gold[name + "/in_gt"]
        assert np.abs(T[-1] - gt).max() < np.abs(T[0] - gt).max()


@pytest.mark.parametrize("name", FIXED)
def test_correspondences_equal_a_kd_trees(gold, name):
    from scipy.spatial import cKDTree
    sc = scene(gold, name)
    T, corr = gold[name + "/transform"], gold[name + "/corr"]
    for p in range(len(sc["s_off"]) - 1):
        a, b, c, d = sc["s_off"][p], sc["s_off"][p + 1], sc["t_off"][p], sc["t_off"][p + 1]
        tree = cKDTree(sc["tgt"][c:d].astype(np.float64))
        for k in range(T.shape[0]):
            dist, j = tree.query(R.move(T[k, p], sc["src"][a:b], np.float64), distance_upper_bound=sc["r"])
            assert np.array_equal(np.where(np.isfinite(dist), j, -1), corr[k, a:b]), (p, k)


def kd_partners(T, src, tgt, r):
    from scipy.spatial import cKDTree
    dist, j = cKDTree(np.asarray(tgt, np.float64)).query(R.move(T, src, np.float64), distance_upper_bound=r)
    return np.where(np.isfinite(dist), j, -1)


@pytest.mark.parametrize("name", [s[0] for s in R.SCENES if s[1] == "converge"])
def test_final_correspondences_of_the_convergence_scenes_equal_a_kd_trees(gold, name):
    sc = scene(gold, name)
    assert np.array_equal(kd_partners(gold[name + "/transform"][0], sc["src"], sc["tgt"], sc["r"]), gold[name + "/corr"])


def test_every_evaluation_of_the_two_scales_equals_a_kd_trees(gold):
    sc = scene(gold, "two_scales")
    _, _, traces = R.screens(sc)
    for i, scale in enumerate(traces[0]):
        assert np.array_equal(scale["src"], gold["two_scales/scale%d_src" % i]) and np.array_equal(scale["tgt"], gold["two_scales/scale%d_tgt" % i])
        assert np.array_equal(scale["T"], gold["two_scales/transform"][i])
        assert len(scale["evals"]) == sc["opts"]["its"][i] + 1
        for e in scale["evals"]:
            assert np.array_equal(kd_partners(e["T"], scale["src"], scale["tgt"], sc["r"]), e["corr"])


@pytest.mark.parametrize("name", ["two_pairs", "converge_noisy"])
def test_cpu_path_equals_the_float32_statement(gold, name):
    from diffreg_hip import registration as G
    sc = scene(gold, name)
    rel = R.REL if sc["kind"] == "converge" else 0.0
    want = R.run(sc, np.float32)
    t = torch.from_numpy
    o = G.icp_pairs(t(sc["src"]), t(sc["tgt"]), t(sc["s_off"]), t(sc["t_off"]), t(sc["init"]), sc["r"], sc["its"], rel, rel, True)
    assert o["iterations"].tolist() == [w["iterations"] for w in want] and o["status"].tolist() == [w["status"] for w in want]
    assert np.array_equal(o["correspondence"].numpy(), np.concatenate([w["corr"] for w in want]))
    # LAPACK through torch and through numpy on the same double H: a few float32 ulps of the composed transform after `its` fits
    np.testing.assert_allclose(o["transforms"].numpy(), np.array([w["transform"] for w in want]), rtol=0, atol=2e-6)
    np.testing.assert_allclose(o["fitness"].numpy(), [w["fitness"] for w in want], rtol=0, atol=1e-7)
    np.testing.assert_allclose(o["inlier_rmse"].numpy(), [w["rmse"] for w in want], rtol=0, atol=2e-7)
    one = G.IterativeClosestPoint(sc["r"], 2, 0.0, 0.0)
    assert "distance_threshold=%g" % sc["r"] in repr(one)
    a, b = sc["s_off"][1], sc["t_off"][1]
    r1 = one(t(sc["src"][:a]), t(sc["tgt"][:b]), t(sc["init"][0]))
    assert r1["transform"].shape == (4, 4) and int(r1["iterations"]) == 2


def test_cpu_voxel_down_sample_and_multi_scale_follow_the_statement(gold):
    from diffreg_hip import registration as G
    sc = scene(gold, "two_scales")
    t = torch.from_numpy
    for i, v in enumerate(sc["opts"]["voxels"]):
        got = G.voxel_down_sample(t(sc["src"]), v).numpy()
        want = gold["two_scales/scale%d_src" % i]
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=0, atol=max(2.4e-7, 4 * float(gold["two_scales/dev_scale%d" % i])))
    cfgs = [dict(voxel_size=v, max_iteration=n) for v, n in zip(sc["opts"]["voxels"], sc["opts"]["its"])]
    T = G.multi_scale_icp(t(sc["src"]), t(sc["tgt"]), t(sc["init"][0]), cfgs, sc["r"], relative_fitness=0.0, relative_rmse=0.0)
    np.testing.assert_allclose(T.numpy(), gold["two_scales/transform"][-1], rtol=0,
                               atol=max(2.4e-7, 4 * float(gold["two_scales/dev_transform"])) + 2e-6)
    buf, ln = G.voxel_down_sample(t(sc["src"]), 0.16, torch.tensor([100, len(sc["src"]) - 100], dtype=torch.int32))
    assert buf.shape[0] == len(sc["src"]) and ln.dtype == torch.int32 and int(ln.sum()) <= len(sc["src"])
    # the status words come back on request: clean here, bit 32 for a pair whose clouds never meet
    T2, st = G.multi_scale_icp(t(sc["src"]), t(sc["tgt"]), t(sc["init"][0]), cfgs, sc["r"], relative_fitness=0.0, relative_rmse=0.0, return_status=True)
    assert torch.equal(T2, T) and st.shape == () and int(st) == 0
    far, st = G.multi_scale_icp(t(sc["src"]), t(sc["tgt"] + 50.0), t(sc["init"][0]), cfgs, sc["r"], return_status=True)
    assert int(st) == 32 and torch.equal(far, t(sc["init"][0]))
    out, vst = G.voxel_down_sample(t(sc["src"]), 0.16, return_status=True)
    assert torch.equal(out, G.voxel_down_sample(t(sc["src"]), 0.16)) and vst.shape == (1,) and int(vst) == 0


def test_index_walk_ends_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for tools/icp_index_check.cpp"
    exe = str(tmp_path / "icp_index_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "diff-reg_amd", "csrc"), os.path.join(ROOT, "tools", "icp_index_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "icp_index_check: ok" in r.stdout, r.stdout + r.stderr
