"""GPU checks of the point-to-point ICP (dr_icp_p2p_f32) and of Open3D's voxel origin (dr_grid_subsample_open3d_f32) against the statement of
tests/icp_ref.py and its fixture tests/golden/icp.npz.  The fixture holds the float64 statement's outputs and the float32 statement's deviation
from them -- parity with Open3D itself is not claimed.  Bar of a tensor: max(one float32 ulp at its scale, 4 x the recorded deviation).
Every call goes through twice(): two runs are bit-equal.

Largest error / bar per family measured on an MI355X: transforms 0.25, fitness 0.25, rmse 0.25, down-sampled points 0.25."""
import numpy as np
import pytest
import torch

from tests import icp_ref as R
from tests.test_icp_cpu import FIXED, NAMES, gold, refusals, scene  # noqa: F401  (gold is a fixture)

pytestmark = pytest.mark.gpu
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
RATIOS = {}


def G():
    from diffreg_hip import registration
    return registration


def bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x          # a NaN the caller planted equals itself


def twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), "two runs differ in " + k
    return a


def pairs(sc, its, rel, init="scene"):
    T = cu(sc["init"]) if isinstance(init, str) else init
    return twice(lambda: G().icp_pairs(cu(sc["src"]), cu(sc["tgt"]), cu(sc["s_off"]), cu(sc["t_off"]), T, sc["r"], its, rel, rel, True))


def bar(gold, name, key, want):
    scale = float(np.abs(want).max()) if np.size(want) else 1.0
    return max(float(np.spacing(np.float32(max(scale, 1e-30)))), 4.0 * float(gold["%s/dev_%s" % (name, key)]))


def held(gold, name, key, got, want):
    b = bar(gold, name, key, want)
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / b)
    print("%s %s: error %.3e bar %.3e ratio %.2f" % (name, key, err, b, err / b))
    assert err <= b, (name, key, err, b)


# ------------------------------------------------------------------------------------------------ (a) the fixture
@pytest.mark.parametrize("name", FIXED)
def test_fixture_every_iteration(gold, name):
    sc = scene(gold, name)
    for k in range(sc["its"] + 1):
        o = pairs(sc, k, 0.0)
        assert np.array_equal(o["correspondence"].cpu().numpy(), gold[name + "/corr"][k].astype(np.int32)), k
        assert o["iterations"].tolist() == [k] * (len(sc["s_off"]) - 1) and o["status"].tolist() == [0] * (len(sc["s_off"]) - 1)
        held(gold, name, "transform", o["transforms"].cpu().numpy(), gold[name + "/transform"][k])
        held(gold, name, "fitness", o["fitness"].cpu().numpy(), gold[name + "/fitness"][k])
        held(gold, name, "rmse", o["inlier_rmse"].cpu().numpy(), gold[name + "/rmse"][k])
    print("largest error / bar so far:", {k: round(v, 3) for k, v in RATIOS.items()})


@pytest.mark.parametrize("name", [s[0] for s in R.SCENES if s[1] == "converge"])
def test_fixture_convergence_stops_at_the_recorded_iteration(gold, name):
    sc = scene(gold, name)
    o = pairs(sc, sc["its"], R.REL)
    assert o["iterations"].tolist() == gold[name + "/iterations"].tolist() and o["status"].tolist() == [0]
    assert np.array_equal(o["correspondence"].cpu().numpy(), gold[name + "/corr"].astype(np.int32))
    held(gold, name, "transform", o["transforms"].cpu().numpy(), gold[name + "/transform"])
    held(gold, name, "fitness", o["fitness"].cpu().numpy(), gold[name + "/fitness"])
    held(gold, name, "rmse", o["inlier_rmse"].cpu().numpy(), gold[name + "/rmse"])


def test_fixture_two_scales(gold):
    sc = scene(gold, "two_scales")
    cfgs = [dict(voxel_size=v, max_iteration=n) for v, n in zip(sc["opts"]["voxels"], sc["opts"]["its"])]
    for i, v in enumerate(sc["opts"]["voxels"]):
        for side in ("src", "tgt"):
            got = G().voxel_down_sample(cu(sc[side]), v).cpu().numpy()
            want = gold["two_scales/scale%d_%s" % (i, side)]
            assert got.shape == want.shape
            held(gold, "two_scales", "scale%d" % i, got, want)
    T = twice(lambda: dict(T=G().multi_scale_icp(cu(sc["src"]), cu(sc["tgt"]), cu(sc["init"][0]), cfgs, sc["r"], relative_fitness=0.0,
                                                 relative_rmse=0.0)))["T"]
    held(gold, "two_scales", "transform", T.cpu().numpy(), gold["two_scales/transform"][-1])


# ------------------------------------------------------------------------------------------------ (b) edges, against the float32 statement
def edge_scene(ns, nt, seed, r=0.25):
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(0, 1, (nt, 3))
    D = R.pose(rng.normal(size=3), 1.5, rng.normal(size=3) * 0.01)
    src = tgt[rng.integers(0, nt, ns)] + rng.normal(size=(ns, 3)) * 0.01
    src = (src - D[:3, 3]) @ D[:3, :3]                       # D moves the sources back next to their targets
    return dict(src=src.astype(np.float32), tgt=tgt.astype(np.float32), s_off=np.array([0, ns], np.int32), t_off=np.array([0, nt], np.int32),
                init=np.eye(4, dtype=np.float32)[None], r=r, kind="fixed", its=3, opts={})


def against_statement(sc, o, its, ulps=16):
    """indices and counts equal; floats within `ulps` float32 ulps at the tensor's scale: the device and the statement round the same
    double fit of the same correspondences to float32 (<= 1 ulp apart per fit: different summation orders in double), and a fit answers an
    ulp-sized change of its moved sources with a change of that size, so after its <= 3 fits the two stay within a few ulps per fit"""
    want = R.run(dict(sc, its=its), np.float32)
    assert np.array_equal(o["correspondence"].cpu().numpy(), np.concatenate([w["corr"] for w in want]).astype(np.int32))
    assert o["iterations"].tolist() == [w["iterations"] for w in want]
    T = np.array([w["transform"] for w in want], np.float64)
    np.testing.assert_allclose(o["transforms"].cpu().numpy(), T, rtol=0, atol=ulps * float(np.spacing(np.float32(np.abs(T).max()))))
    np.testing.assert_allclose(o["fitness"].cpu().numpy(), [w["fitness"] for w in want], rtol=0, atol=6e-8)
    rm = np.array([w["rmse"] for w in want], np.float64)
    np.testing.assert_allclose(o["inlier_rmse"].cpu().numpy(), rm, rtol=0, atol=ulps * float(np.spacing(np.float32(max(rm.max(), 1e-3)))))
    return want


@pytest.mark.parametrize("nt", [1, 64, 65, 1025])
@pytest.mark.parametrize("ns", [1, 3, 4, 5, 63, 64, 65, 257])
def test_edge_sizes(ns, nt):
    sc = edge_scene(ns, nt, 1000 * ns + nt)
    o = pairs(sc, 3, 0.0)
    want = against_statement(sc, o, 3)
    assert o["status"].tolist() == [w["status"] for w in want]
    if nt == 1 or ns == 1:
        assert o["status"].tolist() == [16]                  # every partner is one target, or one correspondence: an all-zero H


def test_edge_empty_source_empty_target_and_a_normal_pair():
    a = edge_scene(70, 90, 3)
    src = np.concatenate([a["src"][:20], a["src"]])
    sc = dict(a, src=src, tgt=a["tgt"], s_off=np.array([0, 0, 20, 90], np.int32), t_off=np.array([0, 0, 0, 90], np.int32),
              init=np.repeat(np.eye(4, dtype=np.float32)[None], 3, 0))
    o = pairs(sc, 3, 0.0)
    assert o["status"].tolist() == [32, 32, 0] and o["iterations"].tolist() == [0, 0, 3]
    assert o["fitness"].tolist()[:2] == [0.0, 0.0] and torch.equal(o["transforms"][:2].cpu(), torch.eye(4).repeat(2, 1, 1))
    assert (o["correspondence"][:20] == -1).all()
    one = pairs(a, 3, 0.0)
    assert torch.equal(one["transforms"][0], o["transforms"][2]) and torch.equal(one["correspondence"], o["correspondence"][20:])


def test_edge_nothing_inside_the_threshold_keeps_the_transform():
    sc = edge_scene(65, 130, 4)
    sc["tgt"] = sc["tgt"] + np.float32(40.0)
    sc["init"] = R.pose([1, 1, 0], 3.0, [0.1, 0.2, 0.3]).astype(np.float32)[None]
    o = pairs(sc, 5, 0.0)
    assert o["status"].tolist() == [32] and o["iterations"].tolist() == [0] and torch.equal(o["transforms"].cpu(), torch.from_numpy(sc["init"]))
    assert (o["correspondence"] == -1).all() and o["fitness"].tolist() == [0.0] and o["inlier_rmse"].tolist() == [0.0]
    against_statement(sc, o, 5)


def test_edge_sources_far_outside_the_targets_grid():
    sc = edge_scene(130, 300, 5)
    sc["src"][:40] += np.float32(-3.0e4)                     # cell coordinates far below 0: clamped to cell 0
    sc["src"][40:80] += np.float32(3.0e5)                    # and beyond 65535 cells of 0.25: clamped to the last cell
    o = pairs(sc, 2, 0.0)
    c = o["correspondence"].cpu().numpy()
    assert (c[:80] == -1).all() and (c[80:] >= 0).all()
    against_statement(sc, o, 2)


def test_edge_duplicate_targets_the_lower_index_wins():
    sc = edge_scene(100, 64, 6)
    sc["tgt"] = np.concatenate([sc["tgt"], sc["tgt"][::-1], sc["tgt"]])       # every target three times
    sc["t_off"] = np.array([0, 192], np.int32)
    o = pairs(sc, 2, 0.0)
    c = o["correspondence"].cpu().numpy()
    assert (c >= 0).all() and (c < 64).all()
    against_statement(sc, o, 2)


def test_edge_collinear_correspondences_set_bit_16():
    line = np.stack([np.arange(40, dtype=np.float32) * 0.1, np.zeros(40, np.float32), np.zeros(40, np.float32)], 1)
    src = line + np.array([0.01, 0.02, -0.01], np.float32)
    sc = dict(src=src, tgt=line, s_off=np.array([0, 40], np.int32), t_off=np.array([0, 40], np.int32), init=np.eye(4, dtype=np.float32)[None],
              r=0.045, kind="fixed", its=1, opts={})
    o = pairs(sc, 1, 0.0)
    assert o["status"].tolist() == [16] and o["iterations"].tolist() == [1]
    T = o["transforms"][0].cpu().numpy().astype(np.float64)
    # the turn about the line is the Jacobi SVD's completion, not LAPACK's: the transform is held to being a rigid motion that puts the
    # sources on the line, and the outputs to the statement's evaluation of the device's own transform
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-6
    e = R.evaluate(T.astype(np.float32), src, line, sc["r"], np.float32)
    assert np.array_equal(o["correspondence"].cpu().numpy(), e["corr"].astype(np.int32)) and e["n"] == 40
    assert abs(float(o["fitness"][0]) - float(e["fitness"])) <= 6e-8 and abs(float(o["inlier_rmse"][0]) - float(e["rmse"])) <= 2e-9
    assert float(e["rmse"]) < 1e-6


@pytest.mark.parametrize("where", ["src", "tgt", "init"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_edge_nonfinite_sets_bit_8_and_leaves_the_outputs(where, bad):
    a = edge_scene(65, 70, 7)
    sc = dict(a, src=np.concatenate([a["src"], a["src"]]), tgt=np.concatenate([a["tgt"], a["tgt"]]), s_off=np.array([0, 65, 130], np.int32),
              t_off=np.array([0, 70, 140], np.int32), init=np.repeat(R.pose([0, 0, 1], 1.0, [0.01, 0, 0]).astype(np.float32)[None], 2, 0))
    good = pairs(dict(a, init=sc["init"][:1]), 2, 0.0)
    sc[where][(0, 1) if where != "init" else (0, 1, 3)] = bad
    o = pairs(sc, 2, 0.0)
    assert o["status"].tolist() == [8, 0] and o["iterations"].tolist() == [0, 2]
    # what the wrapper put there: the initial transform, zeros, -1
    if where != "init":
        assert torch.equal(o["transforms"][0].cpu(), torch.from_numpy(sc["init"][0]))
    assert o["fitness"][0] == 0 and o["inlier_rmse"][0] == 0 and (o["correspondence"][:65] == -1).all()
    assert torch.equal(o["transforms"][1], good["transforms"][0]) and torch.equal(o["correspondence"][65:], good["correspondence"])


def test_edge_offsets_that_are_no_slices_set_bit_4():
    a = edge_scene(65, 70, 8)
    sc = dict(a, src=np.concatenate([a["src"], a["src"]]), tgt=np.concatenate([a["tgt"], a["tgt"]]), t_off=np.array([0, 70, 140], np.int32),
              init=np.repeat(np.eye(4, dtype=np.float32)[None], 2, 0))
    good = pairs(a, 2, 0.0)
    for s_off, want in (([0, 65, 131], [0, 4]), ([0, 65, 60], [0, 4]), ([-1, 65, 130], [4, 4]), ([70, 65, 130], [4, 4])):
        o = pairs(dict(sc, s_off=np.array(s_off, np.int32)), 2, 0.0)
        assert o["status"].tolist() == want, s_off
        if want[0] == 0:
            assert torch.equal(o["transforms"][0], good["transforms"][0]) and o["iterations"].tolist() == [2, 0]
        assert torch.equal(o["transforms"][1].cpu(), torch.eye(4)) and (o["correspondence"][65:] == -1).all()
    o = pairs(dict(sc, s_off=np.array([0, 65, 130], np.int32), t_off=np.array([0, 70, 141], np.int32)), 2, 0.0)
    assert o["status"].tolist() == [0, 4]


def test_edge_evaluation_only_and_null_init():
    sc = edge_scene(130, 257, 9)
    o = pairs(sc, 0, 0.0)
    assert o["iterations"].tolist() == [0] and torch.equal(o["transforms"][0].cpu(), torch.eye(4))
    against_statement(sc, o, 0)
    null = pairs(sc, 3, 0.0, init=None)
    explicit = pairs(sc, 3, 0.0)
    for k in null:
        assert torch.equal(null[k], explicit[k]), k


# ------------------------------------------------------------------------------------------------ (c) a captured call
def test_graph_replay_equals_eager(gold):
    sc = scene(gold, "two_pairs")
    args = (cu(sc["src"]), cu(sc["tgt"]), cu(sc["s_off"]), cu(sc["t_off"]), cu(sc["init"]), sc["r"], 30, R.REL, R.REL, True)
    eager = G().icp_pairs(*args)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            cap = G().icp_pairs(*args)
    for k in cap:
        cap[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(cap[k], eager[k]), k
    assert int(eager["iterations"].max()) < 30


# ------------------------------------------------------------------------------------------------ (d) refusals
def test_refusals_before_any_launch():
    from diffreg_hip import lib
    refusals(lib.raw())
    src = torch.rand(10, 3, device="cuda")
    off = torch.tensor([0, 10], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        G().icp_pairs(src, src, off, off, None, -1.0)
    with pytest.raises(RuntimeError):
        G().icp_pairs(src, src, off, off, None, 0.1, host_s_offsets=np.array([0, 11], np.int32))


# ------------------------------------------------------------------------------------------------ (e) Open3D's voxel origin
def subsample_scene():
    """40 % of the points sit so that min - 0.5 v and floor(min / v) v put a wall between different neighbours"""
    rng = np.random.default_rng(11)
    a = rng.uniform(0.13, 1.9, (700, 3))
    b = rng.uniform(-0.4, 0.77, (333, 3)) + [5.0, 0.0, -2.0]
    return np.concatenate([a, b]).astype(np.float32), np.array([700, 333], np.int32)


def test_open3d_subsample_against_the_float64_statement():
    from diffreg_hip import lib
    pts, lens = subsample_scene()
    v = 0.1
    (buf, ol), (buf2, ol2) = [G().voxel_down_sample(cu(pts), v, cu(lens)) for _ in range(2)]
    n_out = int(ol.sum())                                    # the rows of the buffer behind the count are unspecified
    assert torch.equal(ol, ol2) and torch.equal(buf[:n_out], buf2[:n_out])
    ol = ol.cpu().numpy()
    cut, at, differs = [0, 700, 1033], 0, False
    for c in range(2):
        cloud = pts[cut[c]:cut[c + 1]]
        want, inv, wall = R.voxel_down_sample(cloud, v, np.float64)
        assert wall > 1e-5                                   # no coordinate within float32 rounding of a wall: the membership is the statement's
        assert ol[c] == len(want)
        got = buf[at:at + ol[c]].cpu().numpy()
        at += ol[c]
        # membership: the float32 sum of the statement's members in input order, times the float reciprocal, is the kernel's barycentre
        same, _, _ = R.voxel_down_sample(cloud, v, np.float32)
        assert np.array_equal(got, same)
        # the existing subsample tests' bar against float64: a float32 sum of k <= count members
        cnt = np.bincount(inv)
        np.testing.assert_allclose(got, want, rtol=0, atol=float(cnt.max()) * float(np.spacing(np.float32(np.abs(cloud).max() * cnt.max()))))
        o3, ov, _, _ = lib.grid_subsample(cu(cloud), cu(np.array([len(cloud)], np.int32)), v, vision3d=True)
        differs = differs or int(ov[0]) != ol[c] or not torch.equal(o3[:ol[c]], buf[at - ol[c]:at])
    assert differs                                           # the two origins give different voxels on this scene
    one = G().voxel_down_sample(cu(pts[:700]), v)
    assert torch.equal(one, buf[:ol[0]])


def test_older_origin_modes_are_unchanged():
    """the three older origins through cloud_info_kernel's new branch: the KPConv and vision3d subsamples against the statement of their
    origins in numpy (bit for bit, as tests/test_collate*.py hold them); the min-corner mode through the radius neighbours of both clouds,
    against the float32 brute-force predicate.  That comparison is by SET per row: the entry orders a row's neighbours by distance and the
    order among equal distances is not part of its contract; the limit (40) lies above every row's count on this scene, so no row is cut."""
    from diffreg_hip import lib
    pts, lens = subsample_scene()
    v = np.float32(0.1)
    for vision3d in (False, True):
        out, ol, tot, st = lib.grid_subsample(cu(pts), cu(lens), float(v), vision3d=vision3d)
        again = lib.grid_subsample(cu(pts), cu(lens), float(v), vision3d=vision3d)
        assert torch.equal(out[:int(tot)], again[0][:int(tot)]) and int(st) == 0
        at = 0
        for c, (a, b) in enumerate(((0, 700), (700, 1033))):
            p = pts[a:b]
            mn = p.min(0)
            origin = np.floor(mn / v) * v if vision3d else np.floor(mn * (np.float32(1.0) / v)) * v
            idx = np.floor((p - origin) / v).astype(np.int64)
            key = (idx[:, 2] << 42) | (idx[:, 1] << 21) | idx[:, 0]
            uniq, inv = np.unique(key, return_inverse=True)
            acc, cnt = np.zeros((len(uniq), 3), np.float32), np.zeros(len(uniq), np.int64)
            for i in range(len(p)):
                acc[inv[i]] = acc[inv[i]] + p[i]
                cnt[inv[i]] += 1
            want = acc * (1.0 / cnt.astype(np.float64)).astype(np.float32)[:, None]
            assert int(ol[c]) == len(uniq) and np.array_equal(out[at:at + len(uniq)].cpu().numpy(), want)
            at += len(uniq)
    nb, mc, st = lib.radius_neighbors(cu(pts), cu(pts), cu(lens), cu(lens), 0.15, 40)
    got = nb.cpu().numpy()
    assert int(st) == 0 and got.shape == (1033, 40)
    for a, b in ((0, 700), (700, 1033)):
        d2 = R.sq_dists(pts[a:b], pts[a:b], np.float32)
        want = [np.nonzero(row < np.float32(0.15) * np.float32(0.15))[0] + a for row in d2]
        assert max(len(w) for w in want) < 40
        for i in range(a, b):
            assert set(got[i][got[i] < 1033]) == set(want[i - a]), i


# ------------------------------------------------------------------------------------------------ (f) multi_scale_icp
def test_multi_scale_equals_chained_calls_and_recovers_the_pose(gold):
    sc = scene(gold, "rigid_copy")
    src, tgt, init = cu(sc["src"]), cu(sc["tgt"]), cu(sc["init"][0])
    # voxels this fine hold one point each, so both scales see the full clouds (in voxel order) and the copy stays exact
    cfgs = [dict(voxel_size=2e-3, max_iteration=10), dict(voxel_size=1e-3, max_iteration=20)]
    T = twice(lambda: dict(T=G().multi_scale_icp(src, tgt, init, cfgs, sc["r"])))["T"]
    chained = init
    for cfg in cfgs:
        s, t = G().voxel_down_sample(src, cfg["voxel_size"]), G().voxel_down_sample(tgt, cfg["voxel_size"])
        assert s.shape == src.shape and t.shape == tgt.shape
        chained = G().icp(s, t, chained, sc["r"], cfg["max_iteration"])["transform"]
    assert torch.equal(T, chained)
    assert float((T.cpu().double() - torch.from_numpy(sc["gt"][0])).abs().max()) < 1e-5
    # ragged: the batch of two pairs equals the pairs one by one
    two = scene(gold, "two_pairs")
    cf = [dict(voxel_size=0.12, max_iteration=4), dict(voxel_size=0.06, max_iteration=4)]
    sl, tl = cu(np.diff(two["s_off"]).astype(np.int32)), cu(np.diff(two["t_off"]).astype(np.int32))
    both = G().multi_scale_icp(cu(two["src"]), cu(two["tgt"]), cu(two["init"]), cf, two["r"], sl, tl)
    for p in range(2):
        a, b, c, d = two["s_off"][p], two["s_off"][p + 1], two["t_off"][p], two["t_off"][p + 1]
        assert torch.equal(both[p], G().multi_scale_icp(cu(two["src"][a:b]), cu(two["tgt"][c:d]), cu(two["init"][p]), cf, two["r"]))
