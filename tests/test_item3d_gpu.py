"""GPU tests of the 3D / 4D dataset item on the device: dr_item3d_prepare_f32 and dr_radius_pairs_ragged_f32 through diffreg_hip.lib /
diffreg_hip.item3d, against the fixture minted from the reference's own __getitem__ bodies (tests/golden/item3d.npz) and against the float64
statement of tests/item3d_ref.py on hand-made scenes."""
import numpy as np
import pytest
import torch

from tests import item3d_ref as R
from tests.partition2d3d_ref import GAPR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dt is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
MEASURED = {}     # array kind -> largest |device - reference| / bar seen by the prepare tests (printed by the last of them)


def case(g, kind, k):
    pre = "%s_%d_" % (kind, k)
    return {name[len(pre):]: g[name] for name in g.files if name.startswith(pre)}


def raw_item(kind, c):
    if kind == "3dmatch":
        return dict(src_pcd=c["in_src"], tgt_pcd=c["in_tgt"], rot=c["in_rot"], trans=c["in_trans"])
    raw = dict(s_pc=c["in_src"], t_pc=c["in_tgt"], rot=c["in_rot"], trans=c["in_trans"], s2t_flow=c["in_flow"], correspondences=c["in_corr"])
    if "in_metric_index" in c:
        raw["metric_index"] = c["in_metric_index"]
    return raw


def draws_of(c):
    return {name[5:]: c[name] for name in c if name.startswith("draw_")}


def settings(kind, k):
    cs = (R.CASES_3D if kind == "3dmatch" else R.CASES_4D)[k]
    return dict(max_points=cs[2], data_augmentation=cs[3], rot_factor=1.0, augment_noise=R.NOISE_3D if kind == "3dmatch" else R.NOISE_4D,
                overlap_radius=R.OVERLAP_RADIUS)


def hold(name, got, c, exact):
    """a float32 device array against the reference's output rounded to float32, under the bar of tests/item3d_ref.bar"""
    ref32 = np.asarray(c["out_" + name]).astype(np.float32)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref32.shape, (name, got.shape, ref32.shape)
    bar, _ = R.bar(exact, ref32)
    err = float(np.abs(got.astype(np.float64) - ref32).max()) if got.size else 0.0
    MEASURED[name] = max(MEASURED.get(name, 0.0), err / bar)
    print("%s: |device - reference| %.3e, bar %.3e" % (name, err, bar))
    assert err <= bar, (name, err, bar)


CASES = [("3dmatch", k) for k in range(len(R.CASES_3D))] + [("4dmatch", k) for k in range(len(R.CASES_4D))]


@pytest.mark.parametrize("kind,k", CASES)
def test_prepare_item_against_the_reference(golden, kind, k):
    from diffreg_hip import item3d
    c = case(golden("item3d"), kind, k)
    cfg = settings(kind, k)
    fn = item3d.prepare_item_3dmatch if kind == "3dmatch" else item3d.prepare_item_4dmatch
    item = fn(raw_item(kind, c), draws=draws_of(c), device=DEV, **cfg)
    raw = {k_: c["in_" + k_] for k_ in ("src", "tgt", "rot", "trans")}
    if kind == "4dmatch":
        raw["flow"] = c["in_flow"]
    exact = R.prepare_f64(kind, raw, draws_of(c), cfg["max_points"], cfg["data_augmentation"], cfg["augment_noise"])
    assert len(item) == (8 if kind == "3dmatch" else 9) and all(torch.is_tensor(x) and x.is_cuda for x in item[:7])
    hold("src", item[0], c, exact["src"])
    hold("tgt", item[1], c, exact["tgt"])
    hold("rot", item[5], c, exact["rot"])
    hold("trans", item[6], c, exact["trans"])
    assert item[6].shape == (3, 1)
    for feats, cloud in ((item[2], item[0]), (item[3], item[1])):
        assert feats.dtype == torch.float32 and feats.shape == (cloud.shape[0], 1) and bool((feats == 1).all())
    corr = item[4].cpu().numpy()
    if kind == "3dmatch":
        assert item[7] is None
        # the fixture's list entry for entry: the scenes are screened, no pair is left out
        assert corr.dtype == np.int64 and np.array_equal(corr, c["out_corr"])
    else:
        assert np.array_equal(corr, c["out_corr"])
        hold("flow", item[7], c, exact["flow"])
        if "out_metric_index" in c:
            assert np.array_equal(item[8].cpu().numpy(), c["out_metric_index"])
        else:
            assert item[8] is None
    if (kind, k) == CASES[-1]:
        print("largest |device - reference| / bar per array:", {n: "%.3f" % v for n, v in sorted(MEASURED.items())})


def test_unselected_flow_of_the_4dmatch_subsample(golden):
    """_4dmatch.py:86-88 indexes src_pcd only: without augmentation the flow comes back with the LOADED row count"""
    from diffreg_hip import item3d
    c = case(golden("item3d"), "4dmatch", 3)
    item = item3d.prepare_item_4dmatch(raw_item("4dmatch", c), draws=draws_of(c), device=DEV, **settings("4dmatch", 3))
    assert item[0].shape == (100, 3) and item[7].shape == (300, 3) and c["out_flow"].shape == (300, 3)
    assert np.array_equal(item[7].cpu().numpy(), c["in_flow"])
    assert np.array_equal(item[0].cpu().numpy(), c["in_src"][c["draw_src_perm"][:100]])


def test_batch_of_three_equals_the_pairs_one_by_one(golden):
    from diffreg_hip import item3d
    g = golden("item3d")
    ks = (2, 0, 3)          # unequal sizes, both coin branches, one side subsampled in two of them
    cs = [case(g, "3dmatch", k) for k in ks]
    cfg = dict(settings("3dmatch", 2), max_points=65)
    draws = [draws_of(c) for c in cs]
    for d, c in zip(draws, cs):     # every pair under the same settings: a permutation for each cloud above 65 points
        for side in ("src", "tgt"):
            n = len(c["in_" + side])
            if n > 65 and side + "_perm" not in d:
                d[side + "_perm"] = np.random.default_rng(n).permutation(n)
            d[side + "_jitter"] = np.random.default_rng(7 + n).random((min(n, 65), 3))
    batch = item3d.prepare_batch([raw_item("3dmatch", c) for c in cs], kind="3dmatch", draws=draws, device=DEV, **cfg)
    total = 0
    for p, c in enumerate(cs):
        one = item3d.prepare_batch([raw_item("3dmatch", c)], kind="3dmatch", draws=[draws[p]], device=DEV, **cfg)[0]
        for key in ("src_pcd", "tgt_pcd", "rot", "trn", "correspondences"):
            assert torch.equal(batch[p][key], one[key]), (p, key)
        total += one["correspondences"].shape[0]
    assert total > 0


# ----------------------------------------------------------------------------------------------------------------
# the pair list
# ----------------------------------------------------------------------------------------------------------------
def offsets(ns):
    return torch.tensor(np.concatenate([[0], np.cumsum(ns)]), dtype=torch.int32, device=DEV)


def ragged(scenes, radius, room=None):
    """one count call and one write call of dr_radius_pairs_ragged_f32 over `scenes` = [(src, tgt, tsfm [3, 4] or None)]; room: rows per pair
    (None: exactly what was found) -> (per-pair [C, 2] arrays, counts [P, 2], the raw out_src with 8 canary rows behind it)"""
    from diffreg_hip import lib
    P = len(scenes)
    src = T(np.concatenate([s[0] for s in scenes]).reshape(-1, 3).astype(np.float32))
    tgt = T(np.concatenate([s[1] for s in scenes]).reshape(-1, 3).astype(np.float32))
    so, to = offsets([len(s[0]) for s in scenes]), offsets([len(s[1]) for s in scenes])
    eye = np.eye(4)[:3]
    tsfm = T(np.stack([eye if s[2] is None else s[2] for s in scenes]).astype(np.float32))
    _, _, counts, status = lib.radius_pairs_ragged(src, so, tgt, to, tsfm, radius)
    found = counts[:, 1].cpu().numpy()
    assert not status.any() and (counts[:, 0] == 0).all()
    room = found if room is None else np.asarray(room)
    c_host = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    cap = int(c_host[-1])
    o_src, o_tgt, counts, status = lib.radius_pairs_ragged(src, so, tgt, to, tsfm, radius, T(c_host), cap + 8 if cap else 0)
    counts = counts.cpu().numpy()
    assert not status.any() and np.array_equal(counts[:, 1], found) and np.array_equal(counts[:, 0], np.minimum(found, room))
    o_src, o_tgt = o_src.cpu().numpy(), o_tgt.cpu().numpy()
    out = [np.stack([o_src[c_host[p]:c_host[p] + counts[p, 0]], o_tgt[c_host[p]:c_host[p] + counts[p, 0]]], 1) for p in range(P)]
    return out, counts, (o_src, c_host)


def screened(src, tgt, tsfm, radius):
    rot, trans = (np.eye(3), np.zeros(3)) if tsfm is None else (tsfm[:, :3], tsfm[:, 3])
    assert R.near_radius(src, tgt, rot, trans, radius) == 0, "the scene has a distance within GAPR of the radius"
    return R.radius_pairs(src, tgt, rot, trans, radius)


def cluster_scene(seed, ns, nt, spread):
    rng = np.random.default_rng(seed)
    for _ in range(50):
        src = (rng.random((ns, 3)) * spread).astype(np.float32)
        tgt = (rng.random((nt, 3)) * spread).astype(np.float32)
        if R.near_radius(src, tgt, np.eye(3), np.zeros(3), R.OVERLAP_RADIUS) == 0:
            return src, tgt
    raise AssertionError("no screened scene")


def test_pairs_of_the_fixture_scenes_entry_for_entry(golden):
    g = golden("item3d")
    scenes, want = [], []
    for k in range(len(R.CASES_3D)):
        c = case(g, "3dmatch", k)
        tsfm = np.concatenate([c["out_rot"], c["out_trans"]], 1)
        src, tgt = c["out_src"].astype(np.float32), c["out_tgt"].astype(np.float32)
        assert R.near_radius(src, tgt, c["out_rot"], c["out_trans"], R.OVERLAP_RADIUS) == 0
        scenes.append((src, tgt, tsfm))
        want.append(c["out_corr"])
    out, _, _ = ragged(scenes, R.OVERLAP_RADIUS)
    for k, (a, b) in enumerate(zip(out, want)):
        assert np.array_equal(a, b), k
    assert sum(len(b) for b in want) > 900


def test_pairs_edges():
    r = R.OVERLAP_RADIUS
    far = np.array([[5.0, 5.0, 5.0]], np.float32)
    # a pair with zero correspondences; a source entirely outside the target's grid, on either side of it
    src0, tgt0 = cluster_scene(1, 40, 50, 0.2)
    out, counts, _ = ragged([(src0 + 3.0, tgt0, None), (src0 - 3.0, tgt0, None), (far, tgt0, None)], r)
    assert all(len(o) == 0 for o in out) and not counts.any()
    # points exactly on cell borders: the grid's cell edge is r (1 + 2^-7) from the target's min corner
    cell = np.float32(r) * np.float32(1.0 + 1.0 / 128.0)
    tgt1 = (np.array([[i, j, k] for i in range(4) for j in range(4) for k in range(3)], np.float32) * cell).astype(np.float32)
    src1 = np.concatenate([tgt1[::3] + np.float32(0.25) * cell * np.array([1, -1, 1], np.float32), tgt1[5:9]]).astype(np.float32)
    # rows with more than 64 partners (the neighbour search's limit does not apply), in a cloud with rows that have none
    rng = np.random.default_rng(3)
    tgt2 = np.concatenate([(rng.random((150, 3)) * 0.02).astype(np.float32), (rng.random((30, 3)) * 0.5 + 0.2).astype(np.float32)])
    src2 = np.concatenate([(rng.random((5, 3)) * 0.01).astype(np.float32), (rng.random((70, 3)) * 0.5 + 0.2).astype(np.float32)])
    scenes = [(src1, tgt1, None), (src2, tgt2, None)]
    want = [screened(s, t, None, r) for s, t, _ in scenes]
    assert np.bincount(want[1][:, 0]).max() > 64 and len(want[0]) > len(src1)
    out, _, _ = ragged(scenes, r)
    for a, b in zip(out, want):
        assert np.array_equal(a, b)


def test_pairs_capacity_below_found():
    r = R.OVERLAP_RADIUS
    scenes = [cluster_scene(11, 70, 90, 0.12) + (None,), cluster_scene(12, 33, 20, 0.08) + (None,), cluster_scene(13, 5, 300, 0.1) + (None,)]
    want = [screened(s, t, None, r) for s, t, _ in scenes]
    assert all(len(w) > 10 for w in want)
    room = [len(want[0]) // 2, len(want[1]) + 5, 0]
    out, counts, (o_src, c_host) = ragged(scenes, r, room=room)
    assert np.array_equal(counts[:, 1], [len(w) for w in want])                   # found is exact
    for p in range(3):
        n = min(room[p], len(want[p]))
        assert counts[p, 0] == n and np.array_equal(out[p], want[p][:n])           # the first entries in (i, j) order


def test_pairs_nothing_written_past_the_room():
    from diffreg_hip import lib
    r = R.OVERLAP_RADIUS
    src, tgt = cluster_scene(21, 64, 64, 0.1)
    want = screened(src, tgt, None, r)
    so, to = offsets([64]), offsets([64])
    room = len(want) // 3
    canary = -0x5A5A5A5A5A5A5A5B
    # the library's wrapper allocates the outputs; the raw entry writes into ours, pre-filled
    o_src = torch.full((len(want) + 8,), canary, dtype=torch.int64, device=DEV)
    o_tgt = torch.full((len(want) + 8,), canary, dtype=torch.int64, device=DEV)
    counts = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    raw = lib.raw()
    wsb = raw.dr_radius_pairs_ragged_workspace_bytes(1, 64, 64)
    ws = torch.full((wsb + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    c_off = torch.tensor([0, room], dtype=torch.int64, device=DEV)
    s_, t_ = T(src), T(tgt)
    code = raw.dr_radius_pairs_ragged_f32(1, 64, 64, lib.ptr(s_), lib.ptr(so), lib.ptr(t_), lib.ptr(to), None, r, lib.ptr(c_off), len(want) + 8,
                                          lib.ptr(o_src), lib.ptr(o_tgt), lib.ptr(counts), lib.ptr(status), lib.ptr(ws), wsb, lib.stream_of(s_))
    torch.cuda.synchronize()
    assert code == 0 and counts.cpu().tolist() == [[room, len(want)]]
    assert np.array_equal(o_src[:room].cpu().numpy(), want[:room, 0]) and np.array_equal(o_tgt[:room].cpu().numpy(), want[:room, 1])
    assert bool((o_src[room:] == canary).all()) and bool((o_tgt[room:] == canary).all()) and bool((ws[wsb:] == 0xA5).all())
    assert raw.dr_radius_pairs_ragged_f32(1, 64, 64, lib.ptr(s_), lib.ptr(so), lib.ptr(t_), lib.ptr(to), None, r, lib.ptr(c_off), len(want) + 8,
                                          lib.ptr(o_src), lib.ptr(o_tgt), lib.ptr(counts), lib.ptr(status), lib.ptr(ws), wsb - 1,
                                          lib.stream_of(s_)) == -4


def test_three_ragged_pairs_against_the_one_pair_entry():
    from diffreg_hip.partition2d3d import radius_pairs_raw
    r = R.OVERLAP_RADIUS
    rng = np.random.default_rng(5)
    scenes = []
    for seed, ns, nt in ((31, 130, 70), (32, 1, 257), (33, 300, 3)):
        src, tgt = cluster_scene(seed, ns, nt, 0.15)
        tsfm = np.concatenate([R.euler_zyx(rng.random(3)), rng.normal(size=(3, 1)) * 0.01], 1).astype(np.float32)
        back = (src.astype(np.float64) - tsfm[:, 3]) @ tsfm[:, :3].astype(np.float64)      # so that tsfm brings the source back onto the scene
        scenes.append((back.astype(np.float32), tgt, tsfm))
    for s, t, m in scenes:
        assert R.near_radius(s, t, m[:, :3], m[:, 3], r) == 0
    out, _, _ = ragged(scenes, r)
    for (s, t, m), got in zip(scenes, out):
        i, j, counts = radius_pairs_raw(T(s), T(t), T(np.concatenate([m, [[0, 0, 0, 1]]]).astype(np.float32)), r, capacity=len(got) + 4)
        n = counts.cpu().tolist()
        assert n == [len(got), len(got)] and len(got) > 0
        assert np.array_equal(got, torch.stack([i[:n[0]], j[:n[0]]], 1).cpu().numpy())


def test_get_correspondences(golden):
    from diffreg_hip import item3d
    c = case(golden("item3d"), "3dmatch", 4)
    tsfm = np.eye(4)
    tsfm[:3, :3], tsfm[:3, 3] = c["out_rot"], c["out_trans"][:, 0]
    got = item3d.get_correspondences(T(c["out_src"]), T(c["out_tgt"]), T(tsfm), R.OVERLAP_RADIUS)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), c["out_corr"])
    with pytest.raises(NotImplementedError, match="K"):
        item3d.get_correspondences(T(c["out_src"]), T(c["out_tgt"]), T(tsfm), R.OVERLAP_RADIUS, K=5)


# ----------------------------------------------------------------------------------------------------------------
# prepare_batch -> the device collate -> Pipeline
# ----------------------------------------------------------------------------------------------------------------
def collate_config():
    from diffreg_hip import synth
    # a first cell so small that every point is its own voxel at every level: the coarse clouds are the item's clouds
    return dict(synth.KPFCN_CFG, architecture=list(synth.KPFCN_ARCH), first_subsampling_dl=1e-3, conv_radius=2.5, deform_radius=5.0,
                coarse_level=-2, coarse_match_radius=0.05)


def test_3dmatch_batch_feeds_the_collate_and_the_pipeline(golden):
    """values are pinned by tests/test_collate_gt_gpu.py: here the shapes, and that the training forward and its loss are finite"""
    from diffreg_hip import item3d, synth
    from diffreg_hip.collate import collate_fn_device
    from models.loss import MatchMotionLoss
    from models.pipeline import Pipeline
    from tests.helpers import train_weights
    from tests.test_models_api_gpu import StubBackbone, ref_like_config
    from tests.test_train_gpu import LOSS_CFG
    c = case(golden("item3d"), "3dmatch", 3)
    pairs = item3d.prepare_batch([raw_item("3dmatch", c)], kind="3dmatch", draws=[draws_of(c)], device=DEV, **settings("3dmatch", 3))
    ns, nt = pairs[0]["src_pcd"].shape[0], pairs[0]["tgt_pcd"].shape[0]
    assert (ns, nt) == (100, 65) and pairs[0]["correspondences"].is_cuda and pairs[0]["correspondences"].shape == (len(c["out_corr"]), 2)
    d = collate_fn_device(pairs, collate_config(), [4, 4, 4, 4], training=True)
    assert d["correspondences_list"][0] is pairs[0]["correspondences"] and d["batched_rot"].shape == (1, 3, 3) and d["batched_trn"].shape == (1, 3, 1)
    cs, ct = d["stack_lengths"][-2].cpu().tolist()                              # (two points may share a voxel at a coarse level)
    assert 0 < cs <= ns and 0 < ct <= nt and d["coarse_matches"][0].shape[0] == 2
    ns, nt = cs, ct
    C = synth.VARIANTS["3dmatch"]["C"]
    gen = torch.Generator().manual_seed(11)
    d.update({"_feats": (0.5 * torch.randn(ns + nt, C, generator=gen)).to(DEV), "ts": torch.tensor([300], device=DEV),
              "randn": torch.randn(1, ns, nt, generator=gen).to(DEV)})
    model = Pipeline(ref_like_config("3dmatch", 20, 200.0), backbone=StubBackbone())
    sd = model.state_dict()
    sd.update(train_weights())
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    with torch.no_grad():
        out = model(d)
        info = MatchMotionLoss(dict(LOSS_CFG, motion_weight=0.1))(out)
    assert out["matrix_gt_disturbed"].shape == (1, ns, nt) and bool(torch.isfinite(info["loss"]).all())


def test_4dmatch_batch_feeds_the_collate(golden):
    from diffreg_hip import item3d
    from diffreg_hip.collate import collate_fn_device_4dmatch
    g = golden("item3d")
    cs = [case(g, "4dmatch", 0), case(g, "4dmatch", 1)]
    cfg = settings("4dmatch", 0)
    pairs = item3d.prepare_batch([raw_item("4dmatch", c) for c in cs], kind="4dmatch", draws=[draws_of(c) for c in cs], device=DEV, **cfg)
    d = collate_fn_device_4dmatch(pairs, collate_config(), [4, 4, 4, 4])
    for p, c in enumerate(cs):
        ns = len(c["in_src"])
        assert d["sflow_list"][p].shape == (ns, 3) and d["coarse_flow"][p].shape == (ns, 3) and bool(torch.isfinite(d["coarse_flow"][p]).all())
        assert d["coarse_matches"][p].shape[0] == 2 and torch.equal(d["correspondences_list"][p].cpu(), torch.from_numpy(c["out_corr"]))
    assert d["metric_index_list"] is None and pairs[0]["metric_index"] is not None and pairs[1]["metric_index"] is None


def test_4dmatch_batch_feeds_the_collate_and_the_pipeline(golden):
    """the 4DMatch item through collate_fn_device_4dmatch into Pipeline (variant 4dmatch) under .train(): shapes, and that the training forward
    and its loss (which reads the collate's coarse_flow) are finite"""
    from diffreg_hip import item3d, synth
    from diffreg_hip.collate import collate_fn_device_4dmatch
    from models.loss import MatchMotionLoss
    from models.pipeline import Pipeline
    from tests.helpers import HEAD_GAIN
    from tests.test_models_api_gpu import StubBackbone, ref_like_config
    from tests.test_train_gpu import LOSS_CFG
    c = case(golden("item3d"), "4dmatch", 1)
    pairs = item3d.prepare_batch([raw_item("4dmatch", c)], kind="4dmatch", draws=[draws_of(c)], device=DEV, **settings("4dmatch", 1))
    assert pairs[0]["src_pcd"].shape == (300, 3) and pairs[0]["tgt_pcd"].shape == (65, 3) and pairs[0]["s2t_flow"].shape == (300, 3)
    d = collate_fn_device_4dmatch(pairs, collate_config(), [4, 4, 4, 4])
    ns, nt = d["stack_lengths"][-2].cpu().tolist()                              # (two points may share a voxel at a coarse level)
    assert 0 < ns <= 300 and 0 < nt <= 65 and d["coarse_flow"][0].shape == (ns, 3) and d["coarse_matches"][0].shape[0] == 2
    C = synth.VARIANTS["4dmatch"]["C"]
    gen = torch.Generator().manual_seed(12)
    d.update({"_feats": (0.5 * torch.randn(ns + nt, C, generator=gen)).to(DEV), "ts": torch.tensor([300], device=DEV),
              "randn": torch.randn(1, ns, nt, generator=gen).to(DEV)})
    model = Pipeline(ref_like_config("4dmatch", 20, 40.0), backbone=StubBackbone())
    assert model.variant == "4dmatch"
    W = dict(synth.make_weights(C, seed=7, head_gain=HEAD_GAIN))
    W.update(synth.make_weights_coarse(C, seed=17, head_gain=HEAD_GAIN))
    sd = model.state_dict()
    sd.update({k: torch.from_numpy(v) for k, v in W.items() if k in sd})
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    with torch.no_grad():
        out = model(d)
        info = MatchMotionLoss(dict(LOSS_CFG, dataset="4dmatch", motion_weight=0.1))(out)
    assert out["matrix_gt_disturbed"].shape == (1, ns, nt) and out["conf_matrix_pred"].shape == (1, ns, nt)
    assert out["conf_matrix_gt_hat"].shape == (1, ns, nt) and out["R_s2t_pred"].shape == (1, 3, 3)
    for key in ("conf_matrix_pred", "conf_matrix_gt_hat", "matrix_gt_disturbed", "R_s2t_pred", "t_s2t_pred"):
        assert bool(torch.isfinite(out[key]).all()), key
    assert bool(torch.isfinite(info["loss"]).all())


# ----------------------------------------------------------------------------------------------------------------
# determinism, capture, refusals
# ----------------------------------------------------------------------------------------------------------------
def entry_inputs(golden):
    c = case(golden("item3d"), "3dmatch", 3)
    d = draws_of(c)
    sel = T(np.ascontiguousarray(d["src_perm"][:100]))
    args = (T(c["in_src"]), offsets([300]), T(c["in_tgt"]), offsets([65]), T(c["in_rot"])[None], T(c["in_trans"].reshape(1, 3)))
    kw = dict(s_offsets=offsets([100]), src_sel=sel, rot_ab=T(R.euler_zyx(d["euler"]))[None], coin=T(np.array([d["coin"]])),
              src_jitter=T(d["src_jitter"]), tgt_jitter=T(d["tgt_jitter"]), noise=R.NOISE_3D)
    return args, kw


def run_both(args, kw, c_off, cap):
    from diffreg_hip import lib
    out = lib.item3d_prepare(*args, **kw)
    o_src, o_tgt, counts, _ = lib.radius_pairs_ragged(out["src"], kw["s_offsets"], out["tgt"], args[3], out["tsfm"], R.OVERLAP_RADIUS, c_off, cap)
    return [out["src"], out["tgt"], out["rot"], out["trans"], out["tsfm"], o_src, o_tgt, counts]


def test_two_runs_bit_equal_and_capture_replay(golden):
    from diffreg_hip import lib
    lib.ensure_init()
    args, kw = entry_inputs(golden)
    c_off = torch.tensor([0, 64], dtype=torch.int64, device=DEV)
    a = [t.clone() for t in run_both(args, kw, c_off, 64)]
    b = run_both(args, kw, c_off, 64)
    n = int(a[7][0, 0])
    assert 0 < n <= 64
    for x, y in zip(a, b):
        assert torch.equal(x[:n] if x.dtype == torch.int64 else x, y[:n] if y.dtype == torch.int64 else y)
    # one capture of both entries on one stream, replayed once
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            cap = run_both(args, kw, c_off, 64)
    torch.cuda.current_stream().wait_stream(stream)
    for t in cap:
        t.fill_(0) if t.dtype != torch.float32 else t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(a, cap):
        assert torch.equal(x[:n] if x.dtype == torch.int64 else x, y[:n] if y.dtype == torch.int64 else y)


@pytest.mark.parametrize("gen_device", ["cuda:0", "cpu"])
def test_draws_from_a_torch_generator(golden, gen_device):
    """the default path: nothing replayed, every draw made by torch from `generator` (on the device, or on the host and moved)"""
    from diffreg_hip import item3d
    g = golden("item3d")
    c3, c4 = case(g, "3dmatch", 3), case(g, "4dmatch", 1)
    cfg = dict(settings("3dmatch", 3), max_points=100)

    def run(seed, **kw):
        gen = torch.Generator(device=gen_device)
        gen.manual_seed(seed)
        return item3d.prepare_batch([raw_item("3dmatch", c3), raw_item("3dmatch", case(g, "3dmatch", 2))], kind="3dmatch", generator=gen,
                                    device=DEV, **dict(cfg, **kw))
    a, b, other = run(5), run(5), run(6)
    for p, (ns, nt) in enumerate(((100, 65), (65, 100))):
        d = a[p]
        assert d["src_pcd"].shape == (ns, 3) and d["tgt_pcd"].shape == (nt, 3) and d["rot"].shape == (3, 3) and d["trn"].shape == (3, 1)
        assert d["correspondences"].dim() == 2 and d["correspondences"].shape[1] == 2 and d["correspondences"].dtype == torch.int64
        rot = d["rot"].double()
        assert float((rot @ rot.T - torch.eye(3, device=DEV, dtype=torch.float64)).abs().max()) < 1e-6 and abs(float(torch.linalg.det(rot)) - 1) < 1e-6
        for key in ("src_pcd", "tgt_pcd", "rot", "trn", "correspondences"):
            assert torch.equal(d[key], b[p][key]), key                         # the same seed: the same item
        assert bool(torch.isfinite(d["src_pcd"]).all()) and bool(torch.isfinite(d["tgt_pcd"]).all())
    assert not torch.equal(a[0]["src_pcd"], other[0]["src_pcd"])
    # without augmentation the subsampled cloud is the head of a permutation: 100 DISTINCT rows of the raw cloud, bit for bit
    plain = run(5, data_augmentation=False)[0]
    raw = c3["in_src"]
    rows = [int(np.nonzero((raw == r).all(1))[0][0]) for r in plain["src_pcd"].cpu().numpy()]
    assert len(set(rows)) == 100 and rows != sorted(rows) and np.array_equal(plain["rot"].cpu().numpy(), c3["in_rot"].astype(np.float32))
    gen = torch.Generator(device=gen_device)
    gen.manual_seed(7)
    item = item3d.prepare_item_4dmatch(raw_item("4dmatch", c4), generator=gen, device=DEV, **settings("4dmatch", 1))
    assert item[0].shape == (300, 3) and item[7].shape == (300, 3) and bool(torch.isfinite(item[7]).all()) and item[6].shape == (3, 1)
    # the jitter moves a point by at most noise / 2 per axis and the rotation keeps lengths: |flow'| stays within that of |flow|
    assert float((item[7].norm(dim=1) - torch.from_numpy(c4["in_flow"]).to(DEV).norm(dim=1)).abs().max()) <= R.NOISE_4D * 0.5 * 3 ** 0.5 + 1e-6


def test_device_side_status_bits(golden):
    """what Python refuses first, through the binding that does not: a selection index out of range, a pair whose flow rows differ from its
    selected rows, offsets that are no slice; rows of no pair are written as zero"""
    from diffreg_hip import lib
    rng = np.random.default_rng(2)
    src, tgt = T(rng.random((30, 3)).astype(np.float32)), T(rng.random((12, 3)).astype(np.float32))
    rot, trans = torch.eye(3, device=DEV)[None].repeat(2, 1, 1), torch.zeros(2, 3, device=DEV)
    i64 = lambda a: torch.tensor(a, dtype=torch.int64, device=DEV)
    # pair 0: raw rows [0, 10), pair 1: [10, 30); pair 0 selects 3 rows, one of them row 10 of a cloud of 10
    out = lib.item3d_prepare(src, offsets([10, 20]), tgt, offsets([5, 7]), rot, trans, s_offsets=offsets([3, 20]),
                             src_sel=torch.cat([i64([9, 10, 0]), torch.arange(20, device=DEV)]))
    assert out["status"].cpu().tolist() == [4, 0]
    got = out["src"].cpu().numpy()
    assert np.array_equal(got[0], src[9].cpu().numpy()) and not got[1].any() and np.array_equal(got[2], src[0].cpu().numpy())
    assert np.array_equal(got[3:], src[10:].cpu().numpy()) and torch.equal(out["tgt"], tgt)
    # the totals agree (30 = 30) but pair 0 holds 20 selected rows of a cloud of 10: status bit 8 on pair 0 alone
    sel = torch.cat([torch.arange(20, device=DEV) % 10, torch.arange(10, device=DEV)])
    out = lib.item3d_prepare(src, offsets([10, 20]), tgt, offsets([5, 7]), rot, trans, s_offsets=offsets([20, 10]), src_sel=sel, flow_raw=src.clone(),
                             recompute_flow=True, src_jitter=torch.zeros(30, 3, dtype=torch.float64, device=DEV), noise=0.0)
    assert out["status"].cpu().tolist() == [8, 0]
    # the raw offsets of pair 1 run past the cloud: status bit 2, its rows zero, pair 0 as usual; rows behind the last offset are zero too
    bad = torch.tensor([0, 10, 31], dtype=torch.int32, device=DEV)
    out = lib.item3d_prepare(src, bad, tgt, torch.tensor([0, 5, 11], dtype=torch.int32, device=DEV), rot, trans)
    assert out["status"].cpu().tolist() == [0, 2]
    assert torch.equal(out["src"][:10], src[:10]) and not bool(out["src"][10:].any())
    assert torch.equal(out["tgt"][:11], tgt[:11]) and not bool(out["tgt"][11:].any())
    # the pair list: bad offsets of one pair are its status bit 2 and zero counts, the other pair is listed as usual
    s, t = cluster_scene(41, 20, 30, 0.08)
    want = screened(s, t, None, R.OVERLAP_RADIUS)
    s2, t2 = T(np.concatenate([s, s])), T(np.concatenate([t, t]))
    _, _, counts, status = lib.radius_pairs_ragged(s2, torch.tensor([0, 20, 40], dtype=torch.int32, device=DEV), t2,
                                                   torch.tensor([0, 30, 61], dtype=torch.int32, device=DEV), None, R.OVERLAP_RADIUS)
    assert status.cpu().tolist() == [0, 2] and counts.cpu().tolist() == [[0, len(want)], [0, 0]]


def test_pairs_with_rows_of_no_pair_in_front_of_the_first_offset():
    """offsets[0] != 0: the rows in front sort behind every pair's targets, so a pair's targets are not at sorted positions [t0, t1)"""
    from diffreg_hip import lib
    r = R.OVERLAP_RADIUS
    a, b = cluster_scene(51, 40, 70, 0.1), cluster_scene(52, 33, 20, 0.08)
    want = [screened(a[0], a[1], None, r), screened(b[0], b[1], None, r)]
    junk = np.zeros((6, 3), np.float32) + a[1][:1]                              # in front: copies of a real target, which must pair with nothing
    src, tgt = T(np.concatenate([junk[:2], a[0], b[0], junk[:1]])), T(np.concatenate([junk, a[1], b[1], junk[:3]]))
    so = torch.tensor([2, 42, 75], dtype=torch.int32, device=DEV)
    to = torch.tensor([6, 76, 96], dtype=torch.int32, device=DEV)
    _, _, counts, status = lib.radius_pairs_ragged(src, so, tgt, to, None, r)
    assert status.cpu().tolist() == [0, 0] and counts[:, 1].cpu().tolist() == [len(w) for w in want]
    c_off = torch.tensor([0, len(want[0]), len(want[0]) + len(want[1])], dtype=torch.int64, device=DEV)
    o_src, o_tgt, _, _ = lib.radius_pairs_ragged(src, so, tgt, to, None, r, c_off, int(c_off[-1]))
    got = torch.stack([o_src, o_tgt], 1).cpu().numpy()
    assert np.array_equal(got[:len(want[0])], want[0]) and np.array_equal(got[len(want[0]):], want[1])


def test_refusals(golden):
    from diffreg_hip import item3d, lib
    g = golden("item3d")
    c3, c4 = case(g, "3dmatch", 3), case(g, "4dmatch", 3)
    cfg = settings("3dmatch", 3)
    canary = torch.full((16,), 7.0, device=DEV)
    bad = raw_item("3dmatch", c3)
    bad["src_pcd"] = bad["src_pcd"].astype(np.float64)
    with pytest.raises(ValueError, match="float32"):
        item3d.prepare_item_3dmatch(bad, draws=draws_of(c3), device=DEV, **cfg)
    d = draws_of(c3)
    d["src_perm"] = d["src_perm"].copy()
    d["src_perm"][7] = 300
    with pytest.raises(ValueError, match="addresses row 300"):
        item3d.prepare_item_3dmatch(raw_item("3dmatch", c3), draws=d, device=DEV, **cfg)
    d["src_perm"] = draws_of(c3)["src_perm"][::-1][::2]                      # a strided view
    with pytest.raises(ValueError, match="contiguous int64"):
        item3d.prepare_item_3dmatch(raw_item("3dmatch", c3), draws=d, device=DEV, **cfg)
    d["src_perm"] = T(draws_of(c3)["src_perm"])[::2]
    with pytest.raises(ValueError, match="contiguous int64"):
        item3d.prepare_item_3dmatch(raw_item("3dmatch", c3), draws=d, device=DEV, **cfg)
    # the combination the reference itself crashes on
    with pytest.raises(ValueError, match="the reference raises"):
        item3d.prepare_item_4dmatch(raw_item("4dmatch", c4), device=DEV, **dict(settings("4dmatch", 3), data_augmentation=True))
    args, kw = entry_inputs(golden)
    with pytest.raises(ValueError, match="no flow to recompute"):
        lib.item3d_prepare(*args, flow_raw=T(c3["in_src"]), recompute_flow=True, **kw)
    with pytest.raises(ValueError, match="contiguous int64"):
        lib.item3d_prepare(*args, **dict(kw, src_sel=kw["src_sel"].to(torch.int32)))
    # the C entry refuses the same before its first launch
    a = lib.Item3dArgs()
    a.P, a.n_src_raw, a.n_src = 1, 300, 100
    assert lib.raw().dr_item3d_prepare_f32(None, None) == -1 and lib.raw().dr_item3d_prepare_f32(a, None) == -1
    assert lib.raw().dr_radius_pairs_ragged_f32(1, 4, 4, None, None, None, None, None, 0.1, None, 0, None, None, None, None, None, 0, None) == -1
    torch.cuda.synchronize()
    assert bool((canary == 7.0).all())
