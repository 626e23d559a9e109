"""GPU tests of the ground-truth half of the 3D / 4D training collate: dr_coarse_gt_matches_f32 and dr_blend_flow_knn3_f32 through the C ABI
and through diffreg_hip.lib / diffreg_hip.collate, against the fixture minted from the reference's own functions (tests/golden/collate_gt.npz);
the tie scene against the float64 statement; the training dict into models.pipeline.Pipeline; the calibration against the reference's histograms."""
import ctypes

import numpy as np
import pytest
import torch

from diffreg_hip import synth
from tests import collate_gt_ref as cg
from tests.test_collate_gt_cpu import flow_bar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_I64, CANARY_I32, CANARY_F32, PAD = -0x5A5A5A5A5A5A5A5B, -0x5A5A5A5B, -7.25e33, 8
T = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dt is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


def offsets(ns):
    return np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)


def match_scene(g, k):
    return dict(src=g["m%d_src" % k], tgt=g["m%d_tgt" % k], rot=g["m%d_rot" % k], trn=g["m%d_trn" % k],
                flow=g["m%d_flow" % k] if "m%d_flow" % k in g else None, matches=g["m%d_matches" % k])


def raw_matches(scenes, radius, ws_bytes=None):
    """one ragged call of dr_coarse_gt_matches_f32 through the C ABI with canary words behind every output buffer and behind the workspace
    -> (code, per-pair [2, C] arrays, counts, status, every raw buffer); the canaries and the rows behind every pair's count are asserted untouched"""
    from diffreg_hip import lib
    lib.ensure_init()
    raw = lib.raw()
    P = len(scenes)
    s_off, t_off = offsets([len(s["src"]) for s in scenes]), offsets([len(s["tgt"]) for s in scenes])
    ns, nt = int(s_off[-1]), int(t_off[-1])
    src = T(np.concatenate([s["src"] for s in scenes]).reshape(-1, 3))
    tgt = T(np.concatenate([s["tgt"] for s in scenes]).reshape(-1, 3))
    flow = None if scenes[0]["flow"] is None else T(np.concatenate([s["flow"] for s in scenes]).reshape(-1, 3))
    rot = T(np.stack([s["rot"] for s in scenes]).astype(np.float32))
    trn = T(np.stack([np.asarray(s["trn"], np.float32).reshape(3) for s in scenes]))
    o_src = torch.full((ns + PAD,), CANARY_I64, dtype=torch.int64, device=DEV)
    o_tgt = torch.full((ns + PAD,), CANARY_I64, dtype=torch.int64, device=DEV)
    counts = torch.full((P + PAD,), CANARY_I32, dtype=torch.int32, device=DEV)
    status = torch.full((P + PAD,), CANARY_I32, dtype=torch.int32, device=DEV)
    need = raw.dr_coarse_gt_matches_workspace_bytes(ns, nt)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    so, to = T(s_off), T(t_off)
    code = raw.dr_coarse_gt_matches_f32(P, ns, nt, lib.ptr(src), lib.ptr(so), lib.ptr(tgt), lib.ptr(to), lib.ptr(flow), lib.ptr(rot), lib.ptr(trn),
                                        ctypes.c_float(radius), lib.ptr(o_src), lib.ptr(o_tgt), lib.ptr(counts), lib.ptr(status), lib.ptr(ws),
                                        need if ws_bytes is None else ws_bytes, lib.stream_of(src))
    torch.cuda.synchronize()
    bufs = dict(o_src=o_src.cpu().numpy(), o_tgt=o_tgt.cpu().numpy(), counts=counts.cpu().numpy(), status=status.cpu().numpy())
    assert (bufs["o_src"][ns:] == CANARY_I64).all() and (bufs["o_tgt"][ns:] == CANARY_I64).all()
    assert (bufs["counts"][P:] == CANARY_I32).all() and (bufs["status"][P:] == CANARY_I32).all()
    assert (ws[need:].cpu().numpy() == 0xA5).all()
    if code != 0:
        assert (bufs["o_src"] == CANARY_I64).all() and (bufs["counts"] == CANARY_I32).all()          # refused before any launch
        return code, None, None, None, bufs
    out = []
    for p in range(P):
        a, c, n = int(s_off[p]), int(bufs["counts"][p]), int(s_off[p + 1])
        assert 0 <= c <= n - a
        assert (bufs["o_src"][a + c:n] == CANARY_I64).all() and (bufs["o_tgt"][a + c:n] == CANARY_I64).all()   # rows behind the count: not written
        out.append(np.stack([bufs["o_src"][a:a + c], bufs["o_tgt"][a:a + c]]))
    return code, out, bufs["counts"][:P], bufs["status"][:P], bufs


def raw_blend(scenes):
    """one ragged call of dr_blend_flow_knn3_f32 through the C ABI, canaries behind out_flow and status -> (per-pair flow, status, raw out)"""
    from diffreg_hip import lib
    lib.ensure_init()
    raw = lib.raw()
    P = len(scenes)
    q_off, r_off = offsets([len(s["query"]) for s in scenes]), offsets([len(s["ref"]) for s in scenes])
    nq, nr = int(q_off[-1]), int(r_off[-1])
    q = T(np.concatenate([s["query"] for s in scenes]))
    r = T(np.concatenate([s["ref"] for s in scenes]))
    f = T(np.concatenate([s["ref_flow"] for s in scenes]))
    out = torch.full((nq * 3 + PAD,), CANARY_F32, dtype=torch.float32, device=DEV)
    status = torch.full((P + PAD,), CANARY_I32, dtype=torch.int32, device=DEV)
    qo, ro = T(q_off), T(r_off)
    code = raw.dr_blend_flow_knn3_f32(P, nq, nr, lib.ptr(q), lib.ptr(qo), lib.ptr(r), lib.ptr(f), lib.ptr(ro), lib.ptr(out), lib.ptr(status),
                                      lib.stream_of(q))
    torch.cuda.synchronize()
    assert code == 0
    o, s = out.cpu().numpy(), status.cpu().numpy()
    assert (o[nq * 3:] == np.float32(CANARY_F32)).all() and (s[P:] == CANARY_I32).all()
    flows = [o[:nq * 3].reshape(nq, 3)[q_off[p]:q_off[p + 1]] for p in range(P)]
    return flows, s[:P], o


def blend_scene(g, k):
    return dict(query=g["b%d_query" % k], ref=g["b%d_ref" % k], ref_flow=g["b%d_ref_flow" % k], out=g["b%d_out" % k])


# ----------------------------------------------------------------------------------------------------------------
# dr_coarse_gt_matches_f32
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(cg.MATCH_SCENES)))
def test_matches_equal_the_reference_one_pair_per_call(golden, k):
    sc = match_scene(golden("collate_gt"), k)
    code, out, counts, status, _ = raw_matches([sc], cg.RADIUS)
    assert code == 0 and status[0] == 0 and counts[0] == sc["matches"].shape[1]
    assert out[0].dtype == np.int64 and np.array_equal(out[0], sc["matches"])


@pytest.mark.parametrize("name", sorted(cg.MATCH_BATCHES))
def test_matches_ragged_call_equals_single_calls_and_the_reference_twice(golden, name):
    g = golden("collate_gt")
    scenes = [match_scene(g, k) for k in cg.MATCH_BATCHES[name]]
    code, out, counts, status, bufs = raw_matches(scenes, cg.RADIUS)
    assert code == 0 and not status.any()
    for sc, m, c in zip(scenes, out, counts):
        assert c == sc["matches"].shape[1] and np.array_equal(m, sc["matches"])
        _, single, c1, _, _ = raw_matches([sc], cg.RADIUS)
        assert c1[0] == c and np.array_equal(single[0], m)
    if name == "ragged3":
        assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0                # the zero-match pair sits in the middle
    _, _, _, _, again = raw_matches(scenes, cg.RADIUS)
    for key in bufs:
        assert np.array_equal(bufs[key], again[key])                             # two runs bit-equal, unwritten rows included


def test_matches_tie_scene_follows_the_float64_statement():
    t = cg.TIE_MATCH
    want = cg.coarse_gt_matches(t["src"], t["tgt"], t["rot"], t["trn"], t["radius"], dtype=np.float64)
    code, out, counts, status, _ = raw_matches([dict(t, flow=None)], t["radius"])
    assert code == 0 and status[0] == 0 and np.array_equal(out[0], want) and want.shape == (2, 1)


def test_matches_status_and_refusal_paths(golden):
    g = golden("collate_gt")
    ok = match_scene(g, 2)
    one_src = dict(ok, src=ok["src"][:1])
    one_tgt = dict(ok, tgt=ok["tgt"][:1])
    empty = dict(ok, src=ok["src"][:0])
    code, out, counts, status, _ = raw_matches([ok, one_src, one_tgt, empty, ok], cg.RADIUS)
    assert code == 0 and list(status) == [0, 1, 1, 1, 0] and list(counts[1:4]) == [0, 0, 0]
    assert np.array_equal(out[0], ok["matches"]) and np.array_equal(out[4], ok["matches"])           # the neighbours of a refused pair are served
    # a workspace that is too small: DR_EWORKSPACE before any launch (raw_matches asserts that nothing was written)
    from diffreg_hip import lib
    need = lib.raw().dr_coarse_gt_matches_workspace_bytes(len(ok["src"]), len(ok["tgt"]))
    assert need > 0 and raw_matches([ok], cg.RADIUS, ws_bytes=need - 1)[0] == -4
    assert raw_matches([ok], cg.RADIUS, ws_bytes=0)[0] == -4
    # the wrapper: same lists, and offsets that do not describe a slice are reported, not followed
    s_off, t_off = offsets([len(ok["src"])]), offsets([len(ok["tgt"])])
    o_s, o_t, cnt, st = lib.coarse_gt_matches(T(ok["src"]), T(s_off), T(ok["tgt"]), T(t_off), T(ok["rot"][None]), T(ok["trn"][None]), cg.RADIUS)
    c = int(cnt[0])
    assert int(st[0]) == 0 and np.array_equal(torch.stack([o_s[:c], o_t[:c]]).cpu().numpy(), ok["matches"])
    bad = np.array([0, len(ok["src"]) + 5], np.int32)
    _, _, cnt, st = lib.coarse_gt_matches(T(ok["src"]), T(bad), T(ok["tgt"]), T(t_off), T(ok["rot"][None]), T(ok["trn"][None]), cg.RADIUS)
    assert int(st[0]) == 2 and int(cnt[0]) == 0


# ----------------------------------------------------------------------------------------------------------------
# dr_blend_flow_knn3_f32
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(cg.BLEND_SCENES)))
def test_blend_within_the_references_own_float32_deviation(golden, k):
    g = golden("collate_gt")
    sc = blend_scene(g, k)
    flows, status, _ = raw_blend([sc])
    err = np.abs(flows[0].astype(np.float64) - sc["out"]).max()
    print("blend scene %d: max |device - reference| = %.3e, reference's float32 deviation %.3e, ratio %.3f"
          % (k, err, float(g["b%d_dev" % k][0]), err / float(g["b%d_dev" % k][0])))
    assert status[0] == 0 and err <= flow_bar(g, k)


@pytest.mark.parametrize("name", sorted(cg.BLEND_BATCHES))
def test_blend_ragged_call_equals_single_calls_twice(golden, name):
    g = golden("collate_gt")
    scenes = [blend_scene(g, k) for k in cg.BLEND_BATCHES[name]]
    flows, status, raw_out = raw_blend(scenes)
    assert not status.any()
    for k, sc, f in zip(cg.BLEND_BATCHES[name], scenes, flows):
        assert np.abs(f.astype(np.float64) - sc["out"]).max() <= flow_bar(g, k)
        assert np.array_equal(raw_blend([sc])[0][0], f)
    assert np.array_equal(raw_blend(scenes)[2], raw_out)                         # two runs bit-equal


def test_blend_tie_scene_follows_the_float64_statement():
    b = cg.TIE_BLEND
    want = cg.blend_flow_knn3(b["query"], b["ref"], b["ref_flow"], np.float64)
    flows, status, _ = raw_blend([b])
    # the neighbours are decided exactly (integer coordinates); what is left is float32 rounding of three weights and three products: each
    # of 1 / dist, the weight sum, w / sum, f w and the two additions rounds once, under 8 x 2^-24 of the largest |flow| in all
    assert status[0] == 0 and np.abs(flows[0] - want).max() <= 8 * 2.0 ** -24 * np.abs(b["ref_flow"]).max()


def test_blend_status_paths(golden):
    g = golden("collate_gt")
    ok = blend_scene(g, 0)
    few = dict(ok, ref=ok["ref"][:3], ref_flow=ok["ref_flow"][:3])
    none = dict(ok, query=ok["query"][:0])
    flows, status, _ = raw_blend([few, ok, none, few])
    assert list(status) == [1, 0, 0, 1]
    assert (flows[0] == np.float32(CANARY_F32)).all() and (flows[3] == np.float32(CANARY_F32)).all()     # a refused pair's rows stay untouched
    assert np.abs(flows[1].astype(np.float64) - ok["out"]).max() <= flow_bar(g, 0)
    from diffreg_hip import lib
    f, st = lib.blend_flow_knn3(T(ok["query"]), T(offsets([len(ok["query"])])), T(ok["ref"]), T(ok["ref_flow"]), T(offsets([len(ok["ref"])])))
    assert int(st[0]) == 0 and np.array_equal(f.cpu().numpy(), flows[1])
    _, st = lib.blend_flow_knn3(T(ok["query"]), T(np.array([3, 1], np.int32)), T(ok["ref"]), T(ok["ref_flow"]), T(offsets([len(ok["ref"])])))
    assert int(st[0]) == 2


# ----------------------------------------------------------------------------------------------------------------
# the Python layer
# ----------------------------------------------------------------------------------------------------------------
def kpfcn_config(dl0=0.05):
    return dict(synth.KPFCN_CFG, architecture=list(synth.KPFCN_ARCH), first_subsampling_dl=dl0, conv_radius=2.5, deform_radius=5.0,
                coarse_level=-2, coarse_match_radius=cg.RADIUS)


def sheet_pairs(k=0, n_pairs=2):
    """raw pairs for the whole collate: the calibration sheets, the second view brought back near the first by rot / trn"""
    R = synth._rodrigues(np.array([0.1, 0.3, 1.0]), 0.25)
    t = np.array([0.05, -0.02, 0.01])
    return [(T(a), T(b), T(R.astype(np.float32)), T(t.astype(np.float32))) for a, b in cg.calib_dataset(k)[:n_pairs]]


def coarse_clouds(d, p):
    cnt = d["stack_lengths"][-2].view(-1, 2).cpu().numpy()
    start = int(cnt[:p].sum())
    pts = d["points"][-2].cpu().numpy()
    return pts[start:start + cnt[p, 0]], pts[start + cnt[p, 0]:start + cnt[p, 0] + cnt[p, 1]]


def test_training_dict_of_the_3d_collate():
    from diffreg_hip import lib
    from diffreg_hip.collate import batch_grid_subsampling_kpconv, collate_fn_device
    cfg, limits = kpfcn_config(), [30, 30, 30, 30]
    pairs = sheet_pairs()
    corr = [torch.arange(6).view(3, 2), torch.arange(4).view(2, 2)]
    as_dicts = [dict(src_pcd=p[0], tgt_pcd=p[1], rot=p[2], trn=p[3], correspondences=c, gt_cov=torch.eye(2) * i)
                for i, (p, c) in enumerate(zip(pairs, corr))]
    base = collate_fn_device(pairs, cfg, limits, training=False)
    d = collate_fn_device(as_dicts, cfg, limits)
    new = {"coarse_matches", "fine_pts", "fine_length", "fine_ind", "src_pcd_list", "tgt_pcd_list", "correspondences_list", "gt_cov"}
    assert set(d) - set(base) == new and "coarse_matches" not in base
    for key in base:                                                           # the inference half is what it was
        a, b = base[key], d[key]
        assert all(torch.equal(x, y) for x, y in zip(a, b)) if isinstance(a, list) else torch.equal(a, b)
    assert d["correspondences_list"][1] is corr[1] and torch.equal(d["gt_cov"], torch.stack([torch.eye(2) * 0, torch.eye(2)]))
    assert collate_fn_device(pairs, cfg, limits)["gt_cov"] is None
    assert d["src_pcd_list"][0] is pairs[0][0] and d["tgt_pcd_list"][1] is pairs[1][1]
    total = 0
    for p in range(2):
        s, t = coarse_clouds(d, p)
        want = cg.coarse_gt_matches(s, t, pairs[p][2].cpu().numpy(), pairs[p][3].cpu().numpy(), cg.RADIUS)
        m = d["coarse_matches"][p]
        assert m.dtype == torch.int64 and m.is_cuda and m.shape == want.shape and np.array_equal(m.cpu().numpy(), want)
        total += want.shape[1]
    assert total > 0
    # fine_*: the composition of the existing entries on the same clouds (dataloader.py:232-233; `dl` = the last density change's cell size)
    p0, l0 = d["points"][0], d["stack_lengths"][0]
    fine_dl = (2 * (0.05 * 4) * 2.5 / 2.5) * 0.5 * 0.85
    fp, fl = batch_grid_subsampling_kpconv(p0, l0, sampleDl=fine_dl)
    ind, _, _ = lib.radius_neighbors(fp, p0, fl, l0, fine_dl, 1)
    assert torch.equal(d["fine_pts"], fp) and torch.equal(d["fine_length"], fl) and d["fine_length"].dtype == torch.int32
    fi = d["fine_ind"]
    assert fi.dim() == 1 and fi.dtype == torch.int64 and fi.shape[0] == fp.shape[0] and torch.equal(fi, ind[:, 0])
    n = p0.shape[0]
    assert int(fi.min()) >= 0 and int(fi.max()) <= n                           # n itself is the reference's pad for "nobody inside the radius"
    cloud_of = torch.repeat_interleave(torch.arange(4, device=DEV), l0.long())
    fine_cloud = torch.repeat_interleave(torch.arange(4, device=DEV), fl.long())
    found = fi < n
    assert bool(found.any()) and torch.equal(cloud_of[fi[found]], fine_cloud[found])
    with pytest.raises(ValueError, match="coarse_match_radius"):
        collate_fn_device(pairs, {k: v for k, v in cfg.items() if k != "coarse_match_radius"}, limits)


def test_dict_of_the_4d_collate():
    from diffreg_hip.collate import collate_fn_device, collate_fn_device_4dmatch
    cfg, limits = kpfcn_config(), [30, 30, 30, 30]
    pairs = sheet_pairs(k=2)
    flows = [T((0.02 * synth.hash_normal(77 + i, 1, tuple(p[0].shape))).astype(np.float32)) for i, p in enumerate(pairs)]
    metric = [torch.arange(5, device=DEV), torch.arange(7, device=DEV)]
    mk = lambda with_metric: [dict(src_pcd=p[0], tgt_pcd=p[1], rot=p[2], trn=p[3], s2t_flow=f, **({"metric_index": m} if with_metric or i == 0 else {}))
                              for i, (p, f, m) in enumerate(zip(pairs, flows, metric))]
    d = collate_fn_device_4dmatch(mk(True), cfg, limits)
    base = collate_fn_device(pairs, cfg, limits, training=False)
    new = {"coarse_matches", "coarse_flow", "src_pcd_list", "tgt_pcd_list", "correspondences_list", "sflow_list", "metric_index_list"}
    assert set(d) - set(base) == new and not {"fine_pts", "fine_ind", "fine_length"} & set(d)
    assert d["metric_index_list"][1] is metric[1] and collate_fn_device_4dmatch(mk(False), cfg, limits)["metric_index_list"] is None
    for p in range(2):
        s, t = coarse_clouds(d, p)
        raw, fl = pairs[p][0].cpu().numpy(), flows[p].cpu().numpy()
        exact = cg.blend_flow_knn3(s, raw, fl, np.float64)
        stated = cg.blend_flow_knn3(s, raw, fl, np.float32)
        got = d["coarse_flow"][p]
        assert got.shape == (len(s), 3) and got.dtype == torch.float32 and torch.equal(d["sflow_list"][p], flows[p])
        # the statement is held to the reference by tests/test_collate_gt_cpu.py; its own float32 deviation from float64 sets the bar.  A coarse
        # point that is the barycentre of two raw points is equally far from both: such rows (those that fail the fixture's screening) are left
        # out of the DEVIATION, where float64 may order the pair the other way round, and stay in the COMPARISON, where the device and the
        # float32 statement see the same float32 distances and the same lowest-index rule
        rows = cg.screen_blend_rows(s, raw)
        assert rows.sum() >= 8
        bar = max(1e-9, 4.0 * np.abs(stated.astype(np.float64) - exact)[rows].max())
        assert np.abs(got.cpu().numpy().astype(np.float64) - stated).max() <= bar
        want = cg.coarse_gt_matches(s, t, pairs[p][2].cpu().numpy(), pairs[p][3].cpu().numpy(), cg.RADIUS, flow=got.cpu().numpy())
        assert np.array_equal(d["coarse_matches"][p].cpu().numpy(), want)
    with pytest.raises(ValueError, match="s2t_flow"):
        collate_fn_device_4dmatch([dict(src_pcd=p[0], tgt_pcd=p[1], rot=p[2], trn=p[3]) for p in pairs], cfg, limits)


def test_device_training_dict_feeds_the_pipeline(golden):
    """the device 3D training dict into models.pipeline.Pipeline under .train(): a finite loss, and the ground-truth matrix its coarse_matches
    give equals the one the fixture's (= the reference's) list gives.  The pair is fixture scene 9 with a first cell so small that every point
    is its own voxel at every level: the coarse clouds are the scene's clouds in voxel order, and the fixture's list is carried into that order."""
    from diffreg_hip import lib
    from diffreg_hip.collate import collate_fn_device
    from models.loss import MatchMotionLoss
    from models.pipeline import Pipeline
    from tests.helpers import train_weights
    from tests.test_models_api_gpu import StubBackbone, ref_like_config
    from tests.test_train_gpu import LOSS_CFG
    sc = match_scene(golden("collate_gt"), 9)
    cfg = kpfcn_config(dl0=1e-3)
    pair = (T(sc["src"]), T(sc["tgt"]), T(sc["rot"]), T(sc["trn"]))
    ns, nt = len(sc["src"]), len(sc["tgt"])
    C = synth.VARIANTS["3dmatch"]["C"]
    gen = torch.Generator().manual_seed(11)
    feats = (0.5 * torch.randn(ns + nt, C, generator=gen)).to(DEV)
    randn = torch.randn(1, ns, nt, generator=gen).to(DEV)
    model = Pipeline(ref_like_config("3dmatch", 20, 200.0), backbone=StubBackbone())
    sd = model.state_dict()
    sd.update(train_weights())
    model.load_state_dict(sd)
    model = model.to(DEV).train()

    def batch():
        d = collate_fn_device([pair], cfg, [4, 4, 4, 4])
        d.update({"_feats": feats, "ts": torch.tensor([300], device=DEV), "randn": randn})
        return d
    d = batch()
    s, t = coarse_clouds(d, 0)
    assert s.shape == (ns, 3) and t.shape == (nt, 3)
    perm_s = [int(np.nonzero((sc["src"] == row).all(1))[0][0]) for row in s]           # coarse row -> the scene's row (same float32 bits)
    perm_t = [int(np.nonzero((sc["tgt"] == row).all(1))[0][0]) for row in t]
    assert sorted(perm_s) == list(range(ns)) and sorted(perm_t) == list(range(nt))
    inv_s, inv_t = np.argsort(perm_s), np.argsort(perm_t)
    fixture_list = torch.from_numpy(np.stack([inv_s[sc["matches"][0]], inv_t[sc["matches"][1]]])).to(DEV)

    def gt_matrix(m):
        rows = torch.cat([torch.zeros(1, m.shape[1], dtype=torch.int64, device=DEV), m.to(torch.int64)], 0).t().contiguous()
        return lib.match_matrix(rows, 1, ns, nt)
    got, want = gt_matrix(d["coarse_matches"][0]), gt_matrix(fixture_list)
    assert int(want.sum()) == sc["matches"].shape[1] > 0 and torch.equal(got, want)
    crit = MatchMotionLoss(dict(LOSS_CFG, motion_weight=0.1))
    with torch.no_grad():
        out = model(d)
        info = crit(out)
        ref = batch()
        ref["coarse_matches"] = [fixture_list]
        out_ref = model(ref)
    assert bool(torch.isfinite(info["loss"]).all())
    assert torch.equal(out["matrix_gt_disturbed"], out_ref["matrix_gt_disturbed"])


@pytest.mark.parametrize("k", range(len(cg.CALIB_DATASETS)))
def test_calibration_equals_the_reference(golden, k):
    from diffreg_hip.collate import calibrate_neighbors_device, neighbor_histograms_device
    g = golden("collate_gt")
    cfg = dict(cg.CALIB_CFG, architecture=list(synth.KPFCN_ARCH))
    data = cg.calib_dataset(k)
    seen = []

    def samples():
        for item in data:
            seen.append(1)
            yield item
    limits = calibrate_neighbors_device(samples(), cfg, samples_threshold=cg.CALIB_DATASETS[k][3])
    assert limits.dtype.kind == "i" and np.array_equal(limits, g["c%d_limits" % k])
    assert len(seen) == int(g["c%d_used" % k][0])                              # it stops after the same sample as the reference
    hist = neighbor_histograms_device(data, cfg, samples_threshold=cg.CALIB_DATASETS[k][3]).cpu().numpy()
    w = g["c%d_hists" % k]
    assert hist.shape == (4, cg.hist_bins(5.0)) and np.array_equal(hist[:, :w.shape[1]], w) and not hist[:, w.shape[1]:].any()
