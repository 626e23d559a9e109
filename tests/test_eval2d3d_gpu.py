"""The 2D-3D evaluation metrics on the device (dr_sparse_corr_eval_i64, dr_corr_eval_f32, dr_registration_eval_f64; diffreg_hip/metrics2d3d.py)
against the reference's own float64 outputs (tests/golden/eval2d3d.npz) and -- at sizes no fixture holds -- against the float64 restatement of
tests/eval2d3d_ref.py.  Needs a GPU.

Bars: every integer count and flag equal; a real-valued output |device - reference float64| <= max(1e-9 |reference float64|,
4 |reference float32 - reference float64|) -- the device computes in double, the only slack is the reference's own float32 floor.  One quantity
has no float64 reference: EvalFunction's IR is `.float().mean()` in either run, i.e. float32(inliers / kept); it is held to MORE than the bar:
the device's two counts equal the fixture's, its double equals their quotient exactly, and rounds to the reference's float32 bit for bit.
Against the restatement (double on both sides): 1e-9 relative, counts equal."""
import os

import numpy as np
import pytest
import torch

from oracle import pnp_oracle as po
from tests import eval2d3d_ref as F
from tests.conftest import ROOT
from tests.helpers import pnp_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = np.load(os.path.join(ROOT, "tests", "golden", "eval2d3d.npz"))
C = F.CFG


class Cfg(dict):
    def __getattr__(self, k):
        return self[k]


CFG = Cfg(eval=Cfg(C), ransac=Cfg(num_iterations=1000, distance_tolerance=8.0))


def bar(dev, r32, r64, what):
    dev, r32, r64 = float(dev), float(r32), float(r64)
    if np.isnan(r64):
        return np.isnan(dev), (what, dev, r64)
    e, allowed = abs(dev - r64), max(1e-9 * abs(r64), 4 * abs(r32 - r64))
    print("%s: device %.3e from float64 (bar %.3e)" % (what, e, allowed))
    return e <= allowed, (what, dev, r64, e, allowed)


def close(dev, ref, what):
    dev, ref = float(dev), float(ref)
    assert (np.isnan(dev) and np.isnan(ref)) or abs(dev - ref) <= 1e-9 * abs(ref), (what, dev, ref)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_all(s):
    """every fixture quantity of one scene on the device -> the keys of eval2d3d_ref.restate"""
    from diffreg_hip import lib, metrics2d3d as M
    o = {}
    idx = [t(s[k]) for k in ("img_node_corr_indices", "pcd_node_corr_indices", "gt_img_node_corr_indices", "gt_pcd_node_corr_indices")]
    sp = M.evaluate_sparse_correspondences(int(s["img_num_nodes"]), int(s["pcd_num_nodes"]), *idx)
    o["sp_precision"], o["sp_recall"], o["sp_hit_ratio"] = sp["precision"], sp["recall"], sp["hit_ratio"]
    out, cnt = lib.sparse_corr_eval(int(s["img_num_nodes"]), int(s["pcd_num_nodes"]), *idx, t(s["gt_node_corr_min_overlaps"]), C["acceptance_overlap"])
    o["n_pred"], o["n_listed_pos"] = int(cnt[0]), int(cnt[3])
    o["n_gt_kept"] = int(cnt[1])
    _, cnt0 = lib.sparse_corr_eval(int(s["img_num_nodes"]), int(s["pcd_num_nodes"]), *idx)
    o["n_gt"], o["n_pos"] = int(cnt0[1]), int(cnt0[2])
    sel = F.selection(s)
    fine, fc = lib.corr_eval(t(s["pcd_corr_points"]), t(s["img_corr_points"]), t(s["transform"]), C["acceptance_radius"],
                             sel_indices=None if sel is None else t(sel))
    o["ec_inlier_ratio"], o["ec_distance"], o["ec_overlap"], o["n_inlier"], o["n_overlap"] = fine[0], fine[1], fine[2], int(fc[0]), int(fc[1])
    _, mc = lib.corr_eval(t(s["pcd_corr_points"]), t(s["img_corr_points"]), t(s["transform"]), C["acceptance_radius"], depth_mask=True)
    o["n_kept"], o["n_kept_inlier"] = int(mc[2]), int(mc[3])
    ev = M.EvalFunction(CFG)
    dd = dict(transform=t(s["transform"]))
    od = {k: t(s[k]) for k in F.INPUT_KEYS[2:] if k != "transform"}
    od.update(img_num_nodes=int(s["img_num_nodes"]), pcd_num_nodes=int(s["pcd_num_nodes"]))
    r = ev(dd, od)
    o["ev_PIR"], o["ev_IR"] = r["PIR"], r["IR"]
    o["ev_rre"], o["ev_rte"], o["ev_rmse"], rec = ev.evaluate_registration(dd, od)
    o["ev_recall"] = int(rec)
    o["rmse"] = M.registration_rmse(t(s["pcd_points"]), t(s["transform"]), t(s["estimated_transform"]))
    o["rr"] = int(lib.registration_eval(t(s["pcd_points"]), t(s["transform"]), t(s["estimated_transform"]), C["rmse_threshold"])[1][0])
    o["rre"], o["rte"] = M.isotropic_registration_error(t(s["transform"]), t(s["estimated_transform"]))
    return o


# ---- against the fixture -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(F.SCENES))
def test_against_the_reference(name):
    s = F.make_scene(**F.SCENES[name])
    o = device_all(s)
    for k in F.INT_KEYS:
        assert o[k] == int(G["%s_%s" % (name, k)]), (k, o[k], int(G["%s_%s" % (name, k)]))
    for k in F.REAL_KEYS:
        r32, r64 = G["%s_%s32" % (name, k)], G["%s_%s64" % (name, k)]
        if k == "ev_IR":
            kept, inl = o["n_kept"], o["n_kept_inlier"]
            assert float(o[k]) == (inl / kept if kept else 0.0)
            assert np.float32(float(o[k])) == np.float32(r32) == np.float32(r64)
            continue
        ok, info = bar(o[k], r32, r64, name + " " + k)
        assert ok, info
    assert torch.is_tensor(o["ev_PIR"]) and o["ev_PIR"].dim() == 0 and o["ev_PIR"].is_cuda


def test_numpy_inputs_return_host_numbers():
    from diffreg_hip import metrics2d3d as M
    s = F.make_scene(**F.SCENES["base"])
    r = M.evaluate_correspondences(s["pcd_corr_points"], s["img_corr_points"], s["transform"], positive_radius=C["acceptance_radius"])
    assert isinstance(r["overlap"], float) and bar(r["inlier_ratio"], G["base_ec_inlier_ratio32"], G["base_ec_inlier_ratio64"], "IR")[0]
    assert isinstance(M.registration_rmse(s["pcd_points"], s["transform"], s["estimated_transform"]), float)
    sp = M.evaluate_sparse_correspondences(40, 70, s["img_node_corr_indices"], s["pcd_node_corr_indices"], s["gt_img_node_corr_indices"],
                                           s["gt_pcd_node_corr_indices"])
    assert bar(sp["hit_ratio"], G["base_sp_hit_ratio32"], G["base_sp_hit_ratio64"], "hit_ratio")[0]


# ---- against the restatement -----------------------------------------------------------------------------------------------------------------------
def sparse_case(img, pcd, K, G_, seed, dup_all=False, gt_twice=False, ov_lo=0.0, ov_hi=1.0):
    r = np.random.RandomState(seed)
    cells = r.permutation(img * pcd)
    gt = cells[:min(G_, img * pcd)]
    pool = np.concatenate([gt[: max(len(gt) // 2, 1)], cells[len(gt):len(gt) + K]]) if len(gt) else cells[:max(K, 1)]
    pred = pool[r.randint(0, len(pool), K)] if K else np.zeros(0, np.int64)
    if dup_all:
        pred = np.concatenate([pred, pred])
    if gt_twice:
        gt = np.concatenate([gt, gt[:1]])
    ov = r.uniform(ov_lo, ov_hi, len(gt)).astype(np.float32)
    return [np.asarray(x, dtype=np.int64) for x in (pred // pcd, pred % pcd, gt // pcd, gt % pcd)] + [ov]


SPARSE = {
    "K0": dict(img=9, pcd=11, K=0, G_=5), "G0": dict(img=9, pcd=11, K=6, G_=0), "K1": dict(img=9, pcd=11, K=1, G_=5),
    "all_duplicated": dict(img=12, pcd=40, K=20, G_=30, dup_all=True), "gt_listed_twice": dict(img=12, pcd=40, K=20, G_=30, gt_twice=True),
    "all_gt_under_threshold": dict(img=12, pcd=40, K=20, G_=30, ov_hi=0.29), "1x1": dict(img=1, pcd=1, K=3, G_=1),
    "65x33": dict(img=65, pcd=33, K=300, G_=400), "1530x257": dict(img=1530, pcd=257, K=96, G_=400),
}


@pytest.mark.parametrize("name", list(SPARSE))
def test_sparse_eval_against_the_restatement(name):
    from diffreg_hip import lib
    kw = SPARSE[name]
    pi, pp, gi, gp, ov = sparse_case(seed=len(name) + kw["img"], **kw)
    out, cnt = lib.sparse_corr_eval(kw["img"], kw["pcd"], t(pi), t(pp), t(gi), t(gp), t(ov), C["acceptance_overlap"])
    keep = ov > np.float32(C["acceptance_overlap"])
    want = F.evaluate_sparse_correspondences(kw["img"], kw["pcd"], pi, pp, gi[keep], gp[keep])
    pir, n_list, n_gt = F.coarse_precision(kw["img"], kw["pcd"], pi, pp, gi, gp, ov, C["acceptance_overlap"])
    assert cnt.tolist() == [want["n_pred"], want["n_gt"], want["n_pos"], n_list] and n_gt == want["n_gt"]
    for k, v in enumerate((pir, want["precision"], want["recall"], want["hit_ratio"])):
        close(out[k], v, (name, k))
    if name == "all_gt_under_threshold":
        assert cnt[1] == 0 and float(out[0]) == 0.0
    if name == "K0":
        assert np.isnan(float(out[0])) and float(out[1]) == 0.0


def fine_case(n, seed, nodepth=0.2):
    kw = dict(F.SCENES["base"], n=n, seed=seed, nodepth=nodepth, N=1)
    return F.make_scene(**kw)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 63, 65, 257])
def test_fine_eval_against_the_restatement(n):
    from diffreg_hip import lib
    s = fine_case(n, 100 + n)
    P, Q, T = s["pcd_corr_points"], s["img_corr_points"], s["transform"]
    sels = [None] + ([np.argsort(-s["corr_scores"], kind="stable")[:k] for k in (n, n - 1)] if n > 1 else [])
    for sel in sels:                                               # all of them; num_corr == n; num_corr == n - 1
        out, cnt = lib.corr_eval(t(P), t(Q), t(T), C["acceptance_radius"], sel_indices=None if sel is None else t(sel), depth_mask=True)
        Ps, Qs = (P, Q) if sel is None else (P[sel], Q[sel])
        want = F.evaluate_correspondences(Ps, Qs, T, C["acceptance_radius"])
        ir, kept, kinl = F.fine_precision(Qs, Ps, T, C["acceptance_radius"])
        assert cnt.tolist() == [want["n_inlier"], want["n_overlap"], kept, kinl]
        for k, v in enumerate((want["inlier_ratio"], want["distance"], want["overlap"], ir)):
            close(out[k], v, (n, k))
    if n == 0:
        assert out.tolist() == [0.0, 0.0, 0.0, 0.0]


def test_fine_eval_depth_mask_and_the_direction_of_the_overlap():
    from diffreg_hip import lib
    s = fine_case(65, 7, nodepth=1.0)                              # every image depth 0: nothing remains, nan_to_num_ -> 0
    out, cnt = lib.corr_eval(t(s["pcd_corr_points"]), t(s["img_corr_points"]), t(s["transform"]), C["acceptance_radius"], depth_mask=True)
    assert float(out[3]) == 0.0 and cnt[2:].tolist() == [0, 0]
    # one cloud point is the nearest neighbour of EVERY image point: all image points sit around cloud point 0, the other cloud points are far
    # away.  image -> cloud: every image point is within the radius of a cloud point (overlap 1); cloud -> image would find 1 of n
    n = 65
    r = np.random.RandomState(3)
    P = np.concatenate([np.zeros((1, 3)), 5.0 + r.uniform(0, 1, (n - 1, 3))]).astype(np.float32)
    Q = (r.normal(size=(n, 3)) * 0.01).astype(np.float32)
    out, cnt = lib.corr_eval(t(P), t(Q), t(np.eye(4)), C["acceptance_radius"])
    want = F.evaluate_correspondences(P, Q, np.eye(4), C["acceptance_radius"])
    wrong = F.evaluate_correspondences(P, Q, np.eye(4), C["acceptance_radius"], mutant="overlap_wrong_direction")
    assert want["overlap"] == 1.0 and abs(wrong["overlap"] - 1.0 / n) < 1e-12
    close(out[2], want["overlap"], "overlap")
    assert cnt[1] == n and cnt[0] == want["n_inlier"]


def exact_pose():
    """a pose whose rotation has entries 0 / +-1: every product in the trace is exact, so RRE is exactly 0 / 180 in any order of summation"""
    T = np.eye(4)
    T[:3, :3] = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    T[:3, 3] = [0.25, -0.5, 2.0]
    return T


@pytest.mark.parametrize("N", [1, 255, 257, 20000])
def test_registration_eval_against_the_restatement(N):
    from diffreg_hip import lib
    r = np.random.RandomState(N)
    pts = (r.uniform(-1, 1, (N, 3)) * np.array([1.0, 0.8, 0.6])).astype(np.float32)
    s = F.make_scene(**dict(F.SCENES["base"], seed=N % 97, n=1, N=1))
    Gt, E = s["transform"], s["estimated_transform"]
    out, rec = lib.registration_eval(t(pts), t(Gt), t(E), C["rmse_threshold"])
    rre, rte, ev_rmse, ev_rec = F.evaluate_registration(pts, Gt, E, C["rmse_threshold"])
    rmse = F.registration_rmse(pts, Gt, E)
    for k, v in enumerate((rmse, ev_rmse, rre, rte)):
        close(out[k], v, (N, k))
    assert rec.tolist() == [int(rmse < C["rmse_threshold"]), int(ev_rec)]
    # the estimate equal to the ground truth: both errors exactly 0, RMSE exactly 0 (the same arithmetic on both sides), the realignment error at
    # the rounding of inv(T) T p - p: a few ulp of the coordinates (|p| <= 1.5, translation 2.3: 1e-14 is 20 ulp)
    X = exact_pose()
    out, rec = lib.registration_eval(t(pts), t(X), t(X), C["rmse_threshold"])
    assert out[0] == 0.0 and out[2] == 0.0 and out[3] == 0.0 and float(out[1]) < 1e-14 and rec.tolist() == [1, 1]
    # a 180 degree rotation: (trace - 1) / 2 = -1 exactly
    Y = X.copy()
    Y[:3, :3] = X[:3, :3] @ np.diag([1.0, -1.0, -1.0])
    out, rec = lib.registration_eval(t(pts), t(X), t(Y), C["rmse_threshold"])
    close(out[2], 180.0, "RRE at 180")
    assert float(out[3]) == 0.0
    close(out[0], F.registration_rmse(pts, X, Y), "rmse at 180")
    close(out[1], F.evaluate_registration(pts, X, Y, 0.1)[2], "realignment at 180")


# ---- behaviour -------------------------------------------------------------------------------------------------------------------------------------
def three_entries(a):
    from diffreg_hip import lib
    sp = lib.sparse_corr_eval(1530, 257, a["pi"], a["pp"], a["gi"], a["gp"], a["ov"], C["acceptance_overlap"])
    fi = lib.corr_eval(a["P"], a["Q"], a["T"], C["acceptance_radius"], sel_indices=a["sel"], depth_mask=True)
    rg = lib.registration_eval(a["pts"], a["T"], a["E"], C["rmse_threshold"])
    return [x.clone() for pair in (sp, fi, rg) for x in pair]


def behaviour_inputs(seed):
    pi, pp, gi, gp, ov = sparse_case(1530, 257, 96, 400, seed)
    s = F.make_scene(**dict(F.SCENES["topk"], seed=seed, N=20000))
    return dict(pi=t(pi), pp=t(pp), gi=t(gi), gp=t(gp), ov=t(ov), P=t(s["pcd_corr_points"]), Q=t(s["img_corr_points"]), T=t(s["transform"]),
                E=t(s["estimated_transform"]), sel=t(F.selection(s)), pts=t(s["pcd_points"]))


def test_two_runs_are_bit_identical():
    a = behaviour_inputs(11)
    for x, y in zip(three_entries(a), three_entries(a)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_three_entries_capture_into_one_graph_and_replay_with_changed_inputs():
    """no entry reads anything back to the host: one capture, then a replay on inputs the capture never saw"""
    a, b = behaviour_inputs(12), behaviour_inputs(13)
    eager_a, eager_b = three_entries(a), three_entries(b)
    assert not torch.equal(eager_a[0], eager_b[0]) and not torch.equal(eager_a[2], eager_b[2]) and not torch.equal(eager_a[4], eager_b[4])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            outs = three_entries(a)
        g.replay()
        torch.cuda.synchronize()
        for x, y in zip(outs, eager_a):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        for k in a:
            a[k].copy_(b[k])
        g.replay()
    torch.cuda.synchronize()
    for x, y in zip(outs, eager_b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_an_index_out_of_range_raises_the_status_word_and_is_skipped():
    from diffreg_hip import lib
    lib.device_status(torch.device(DEV))                           # clean before
    pi, pp, gi, gp, ov = sparse_case(12, 40, 20, 30, 5)
    good, cg = lib.sparse_corr_eval(12, 40, t(pi), t(pp), t(gi), t(gp))
    bad_pi, bad_pp = np.concatenate([pi, [12, -1, 3]]), np.concatenate([pp, [0, 0, 40]])
    bad_gi, bad_gp = np.concatenate([gi, [2 ** 40]]), np.concatenate([gp, [0]])
    out, cnt = lib.sparse_corr_eval(12, 40, t(bad_pi), t(bad_pp), t(bad_gi), t(bad_gp))
    assert cnt.tolist() == cg.tolist()
    close(out[0], float(good[0]) * len(pi) / (len(pi) + 3), "the list keeps its length")
    assert out[1:].tolist() == good[1:].tolist()
    with pytest.raises(RuntimeError, match="invalid argument"):
        lib.device_status(torch.device(DEV))
    lib.device_status(torch.device(DEV))                           # consumed
    s = fine_case(65, 9)
    sel = np.array([0, 5, 65, -2, 64], dtype=np.int64)
    out, cnt = lib.corr_eval(t(s["pcd_corr_points"]), t(s["img_corr_points"]), t(s["transform"]), C["acceptance_radius"], sel_indices=t(sel))
    keep = np.array([0, 5, 64])
    want = F.evaluate_correspondences(s["pcd_corr_points"][keep], s["img_corr_points"][keep], s["transform"], C["acceptance_radius"])
    assert cnt[:2].tolist() == [want["n_inlier"], want["n_overlap"]]
    close(out[1], want["distance"] * 3 / 5, "skipped selections add nothing")
    close(out[0], want["n_inlier"] / 5, "m stays the denominator")
    close(out[3], want["n_inlier"] / 5, "and the unmasked IR's")       # depth_mask == 0: over all m
    assert cnt[2:].tolist() == [5, want["n_inlier"]]
    with pytest.raises(RuntimeError, match="invalid argument"):
        lib.device_status(torch.device(DEV))


def test_the_limits_return_enosup():
    from diffreg_hip import lib
    z = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="not supported"):
        lib.sparse_corr_eval(8193, 8193, z, z, z, z)
    p = torch.zeros(4, 3, device=DEV)
    with pytest.raises(RuntimeError, match="not supported"):
        lib.corr_eval(p, p, torch.eye(4, dtype=torch.float64, device=DEV), 0.05, sel_indices=torch.zeros(16385, dtype=torch.int64, device=DEV))


# ---- value-only mutants ----------------------------------------------------------------------------------------------------------------------------
def test_value_only_mutants_are_caught():
    """Each mutant is a mutated float64 RESTATEMENT held against the reference's stored values at the bars of test_against_the_reference (no mutated
    device build is run): the bars separate the mutants, and the device passes the same bars above."""
    s = F.make_scene(**F.SCENES["clip180"])                        # every prediction listed twice
    m = F.evaluate_sparse_correspondences(s["img_num_nodes"], s["pcd_num_nodes"], s["img_node_corr_indices"], s["pcd_node_corr_indices"],
                                          s["gt_img_node_corr_indices"], s["gt_pcd_node_corr_indices"], mutant="dup_twice")
    assert not bar(m["precision"], G["clip180_sp_precision32"], G["clip180_sp_precision64"], "mutant: duplicates counted twice")[0]
    s = F.make_scene(**F.SCENES["base"])
    m = F.evaluate_correspondences(s["pcd_corr_points"], s["img_corr_points"], s["transform"], C["acceptance_radius"], mutant="overlap_wrong_direction")
    assert not bar(m["overlap"], G["base_ec_overlap32"], G["base_ec_overlap64"], "mutant: overlap searched from the cloud")[0]
    m = F.fine_precision(s["img_corr_points"], s["pcd_corr_points"], s["transform"], C["acceptance_radius"], mutant="no_depth_mask")
    assert np.float32(m[0]) != np.float32(G["base_ev_IR64"]) and m[1] != int(G["base_n_kept"])
    m = F.registration_rmse(s["pcd_points"], s["transform"], s["estimated_transform"], mutant="mean_of_norms")
    assert not bar(m, G["base_rmse32"], G["base_rmse64"], "mutant: mean of norms")[0]
    # >= at the overlap threshold: no fixture may hold an overlap at the threshold, so the device itself is shown to take `>` where one sits
    # exactly there, and the mutant to miss the restatement's bar
    from diffreg_hip import lib
    pi, pp, gi, gp, ov = sparse_case(12, 40, 20, 30, 5)
    ov[: len(ov) // 2] = np.float32(C["acceptance_overlap"])
    out, cnt = lib.sparse_corr_eval(12, 40, t(pi), t(pp), t(gi), t(gp), t(ov), C["acceptance_overlap"])
    want = F.coarse_precision(12, 40, pi, pp, gi, gp, ov, C["acceptance_overlap"])
    mut = F.coarse_precision(12, 40, pi, pp, gi, gp, ov, C["acceptance_overlap"], mutant="ge_overlap")
    close(out[0], want[0], "PIR at the threshold")
    assert int(cnt[1]) == want[2] != mut[2] and abs(mut[0] - want[0]) > 1e-9 * abs(want[0])


# ---- evaluate_pair end to end ------------------------------------------------------------------------------------------------------------------------
def pair_data(seed, n):
    X, px, K, T, good = pnp_scene(seed, n=n)
    r = np.random.RandomState(seed)
    Y = X.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + r.normal(size=(n, 3)) * 0.01
    Y[~good] += 0.5
    pi, pp, gi, gp, _ = sparse_case(24, 33, 12, 20, seed)
    return dict(img_num_nodes=24, pcd_num_nodes=33, img_node_corr_indices=pi, pcd_node_corr_indices=pp, gt_img_node_corr_indices=gi,
                gt_pcd_node_corr_indices=gp, pcd_corr_points=X, img_corr_points=Y.astype(np.float32), img_corr_pixels=px,
                corr_scores=(r.permutation(n) / n).astype(np.float32), transform=T, intrinsics=K,
                pcd_points=(r.uniform(-1, 1, (500, 3)) * np.array([1.2, 0.9, 0.8]) + np.array([0, 0, 3.0])).astype(np.float32))


def test_evaluate_pair_end_to_end(monkeypatch):
    """a synthetic pair with a known pose: the PnP pose of lib.pnp_ransac and the RR flag against the same chain through oracle/pnp_oracle.py (the
    project's pin of dr_pnp_ransac_f64; parity against OpenCV's solvePnPRansac itself stays UNPINNED: cv2 is not available), the rest against the
    restatement; the metric vector through shard.reduce_metrics"""
    from diffreg_hip import lib, metrics2d3d as M, shard
    d = pair_data(3, 400)
    out = M.evaluate_pair(d, CFG, num_corr=256, seed=3)
    sel = np.argsort(-d["corr_scores"], kind="stable")[:256]
    want = po.pnp_ransac(d["pcd_corr_points"][sel], d["img_corr_pixels"][sel], d["intrinsics"], num_iterations=1000, distance_tolerance=8.0, seed=3)
    est = out["estimated_transform"].cpu().numpy()
    assert np.abs(est - want["transform"]).max() < 1e-6
    rmse = F.registration_rmse(d["pcd_points"], d["transform"], want["transform"])
    assert abs(rmse - C["rmse_threshold"]) > 1e-5 and float(out["RR"]) == float(rmse < C["rmse_threshold"]) == 1.0
    close(out["RMSE"], F.registration_rmse(d["pcd_points"], d["transform"], est), "RMSE of the device's own pose")
    rre, rte = F.isotropic_registration_error(d["transform"], est)
    close(out["RRE"], rre, "RRE")
    close(out["RTE"], rte, "RTE")
    fine = F.evaluate_correspondences(d["pcd_corr_points"][sel], d["img_corr_points"][sel], d["transform"], C["acceptance_radius"])
    sp = F.evaluate_sparse_correspondences(24, 33, d["img_node_corr_indices"], d["pcd_node_corr_indices"], d["gt_img_node_corr_indices"],
                                           d["gt_pcd_node_corr_indices"])
    for k, v in (("IR", fine["inlier_ratio"]), ("OR", fine["overlap"]), ("residual", fine["distance"]), ("PIR", sp["precision"])):
        close(out[k], v, k)
    assert float(out["FMR"]) == float(fine["inlier_ratio"] >= C["inlier_ratio_threshold"]) and out["num_correspondences"] == 256
    assert [float(out[k]) for k in ("PMR>0", "PMR>=0.1", "PMR>=0.3", "PMR>=0.5")] == [float(sp["precision"] > 0), float(sp["precision"] >= 0.1),
                                                                                 float(sp["precision"] >= 0.3), float(sp["precision"] >= 0.5)]
    v = out["vector"]
    assert v.dtype == torch.float64 and v.shape[0] == len(M.VECTOR_NAMES)
    red = shard.reduce_metrics(v + v)                                  # two pairs' vectors sum
    assert red["n_pairs"] == 2.0 and abs(red["mean_inlier_ratio"] - float(out["IR"])) < 1e-15 and red["registration_recall"] == 1.0
    # all fifteen sums by name (shard.reduce_metrics names the first five only)
    full = M.reduce_pair_metrics(v + v)
    assert set(M.VECTOR_NAMES) <= set(full) and full["n_pairs"] == 2.0
    for k, w in (("PIR", sp["precision"]), ("OR", fine["overlap"]), ("residual", fine["distance"]), ("mean_RRE", rre), ("mean_RTE", rte),
                 ("IR", fine["inlier_ratio"])):
        close(full[k], w, k)
    assert full["RR"] == 1.0 and full["sum_num_correspondences"] == 512.0 and full["PMR>0"] == float(sp["precision"] > 0)
    # a pose the caller already has is evaluated in place of PnP's (PnP not called: patched below)
    monkeypatch.setattr(lib, "pnp_ransac", lambda *a, **k: pytest.fail("PnP called although a pose was given"))
    og = M.evaluate_pair(d, CFG, num_corr=256, estimated_transform=want["transform"])
    close(og["RMSE"], rmse, "RMSE of a given pose")
    assert float(og["RR"]) == 1.0
    # three correspondences: RR 0 and PnP is never called
    monkeypatch.setattr(lib, "pnp_ransac", lambda *a, **k: pytest.fail("PnP called with fewer than 4 correspondences"))
    d3 = {k: (v[:3] if k in ("pcd_corr_points", "img_corr_points", "img_corr_pixels", "corr_scores") else v) for k, v in d.items()}
    o3 = M.evaluate_pair(d3, CFG)
    assert float(o3["RR"]) == 0.0 and o3["estimated_transform"] is None and o3["num_correspondences"] == 3 and float(o3["vector"][2]) == 0.0
