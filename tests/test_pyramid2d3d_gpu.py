"""GPU: the 2D-3D loader's graph pyramid and neighbour-limit calibration on the device (csrc/collate.hip: dr_grid_subsample_vision3d_f32,
dr_radius_neighbors_f32, dr_radius_count_hist_f32; diffreg_hip/pyramid2d3d.py; overlay2d3d pyramid=...).

Against tests/golden/pyramid2d3d.npz, recorded from the reference's own collate-time C++ (tools/golden/make_golden_pyramid2d3d.py): barycentres bit
for bit as a row-sorted set, index matrices entry for entry (runs of equal float32 d^2, which only the subsampling matrices hold, in ascending index
order on both sides: tests/pyramid2d3d_ref.canonical_ties), histograms and calibrated limits integer-equal.  The backbone comparison carries the bar
tests/test_pcd_backbone2d3d_gpu.py holds the device backbone to: 1e-4 of the tensor's maximum."""
import numpy as np
import pytest
import torch

from tests import pcd_backbone2d3d_ref as B
from tests import pyramid2d3d_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CACHE = {}


def _golden():
    if "g" not in _CACHE:
        _CACHE["g"] = R.load()
    return _CACHE["g"]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rowsort(p):
    return p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]


def _clouds(p, lengths):
    o = np.concatenate([[0], np.cumsum(lengths)])
    return [p[o[i]:o[i + 1]] for i in range(len(lengths))]


def _device_pyramid(name):
    from diffreg_hip import pyramid2d3d as P
    if name not in _CACHE:
        g = _golden()[0][name]
        d = P.build_grid_and_radius_graph_pyramid_pack_mode(_dev(g["points"][0]), _dev(g["lengths"][0]), R.NUM_STAGES, R.VOXEL, R.RADIUS,
                                                            list(R.LIMITS))
        _CACHE[name] = d
    return _CACHE[name]


@pytest.mark.parametrize("name", R.SCENES)
def test_grid_subsample_bit_exact(name):
    """scene "origin" is the one whose minima tell vision3d's grid origin from KPConv's (tests/pyramid2d3d_ref.py): the KPConv entry fails it"""
    from diffreg_hip import pyramid2d3d as P
    g = _golden()[0][name]
    for i in range(1, R.NUM_STAGES):
        pts, lens = P.grid_subsample_pack_mode(_dev(g["points"][i - 1]), _dev(g["lengths"][i - 1]), R.VOXEL * 2 ** i)
        assert pts.dtype == torch.float32 and lens.dtype == torch.int64
        assert np.array_equal(lens.cpu().numpy(), g["lengths"][i]), (i, lens.cpu().numpy(), g["lengths"][i])
        for got, ref in zip(_clouds(pts.cpu().numpy(), g["lengths"][i]), _clouds(g["points"][i], g["lengths"][i])):
            assert np.array_equal(_rowsort(got).view(np.uint32), _rowsort(ref).view(np.uint32)), (name, i)


def _stage_tol(g, i):
    """how far a stage's device barycentres may lie from the golden's when the stage is subsampled from the DEVICE's previous stage: stages 0
    and 1 are bit-equal (stage 1 sums the given points in the given order).  From stage 2 on the summands arrive in another order (the
    reference's previous stage is in hash-map order, the device's in key order), so the float32 sums round differently: a voxel of stage
    i >= 2 holds at most 8 points of stage i - 1 (one per half-size voxel), 7 additions rounded by at most 2^-24 of a partial sum <= 8 M and one
    product, on either side: E = 2 (8 + 2) 2^-24 M with M the largest coordinate.  A mean moves by no more than its summands do, so stage i
    inherits stage i - 1's distance and adds E: (i - 1) E."""
    return (i - 1) * 20 * 2.0 ** -24 * float(np.abs(g["points"][0]).max()) if i >= 2 else 0.0


def _assert_equal_up_to_moved_points(q, s, got, ref, r, e, what):
    """got (a device matrix in the golden's numbering, searched on points that lie within e per coordinate, queries and supports together, of the
    golden's q and s) against ref: every row holds the same supports, and where the order differs the two entries at a position are equally far
    within what the moved points allow.  d^2 = |q - s|^2 with |q - s| < r changes by at most 2 r sqrt(3) e + 3 e^2 when q - s moves by e per
    coordinate, and each side's float32 evaluation adds 4 roundings of 2^-24 r^2: TAU = 2 sqrt(3) r e + 3 e^2 + 8 2^-24 r^2.  (A support within
    TAU of r^2 or of the limit cut could also change the membership; the fixtures hold no such row, and this check would report one.)"""
    tau = 2 * np.sqrt(3.0) * r * e + 3 * e * e + 8 * 2.0 ** -24 * r * r
    rows = np.nonzero((got != ref).any(1))[0]
    if len(rows) == 0:
        return
    assert np.array_equal(np.sort(got[rows], 1), np.sort(ref[rows], 1)), what
    s_pad = np.concatenate([s.astype(np.float64), np.full((1, 3), np.inf)], 0)
    d2 = lambda m: ((s_pad[m[rows]] - q[rows, None, :].astype(np.float64)) ** 2).sum(-1)
    a, b = d2(got), d2(ref)
    moved = got[rows] != ref[rows]
    with np.errstate(invalid="ignore"):                       # padding against padding: inf - inf at positions that did not move
        worst = float(np.abs(a - b)[moved].max())
    print("%s: %d rows ordered differently, largest d^2 gap %.2e (allowed %.2e)" % (what, len(rows), worst, tau))
    assert worst <= tau, what


def _search(g, kind, i, limit=None):
    """(queries stage, supports stage, radius, limit, golden matrix) of one matrix of the pyramid"""
    r = R.RADIUS * 2 ** i
    if kind == "neighbors":
        return i, i, r, R.LIMITS[i], g["neighbors"][i]
    if kind == "subsampling":
        return i + 1, i, r, R.LIMITS[i], g["subsampling"][i]
    return i, i + 1, 2 * r, R.LIMITS[i + 1], g["upsampling"][i]


@pytest.mark.parametrize("name", R.SCENES)
def test_radius_search_on_golden_points(name):
    from diffreg_hip import pyramid2d3d as P
    g = _golden()[0][name]
    cases = [("neighbors", i) for i in range(R.NUM_STAGES)] + [(k, i) for k in ("subsampling", "upsampling") for i in range(R.NUM_STAGES - 1)]
    tied = 0
    for kind, i in cases + [("narrow", 0)]:
        if kind == "narrow":
            qs, ss, r, limit, ref = 0, 0, R.RADIUS, g["narrow_limit"], g["neighbors0_narrow"]
            assert ref.shape[1] == limit < g["neighbors"][0].shape[1]
        else:
            qs, ss, r, limit, ref = _search(g, kind, i)
        q, s = g["points"][qs], g["points"][ss]
        got = P.radius_search_pack_mode(_dev(q), _dev(s), _dev(g["lengths"][qs]), _dev(g["lengths"][ss]), r, limit)
        assert got.dtype == torch.int64
        got = got.cpu().numpy()
        assert got.shape == ref.shape, (kind, i, got.shape, ref.shape)            # the width: min(longest row, limit)
        if kind == "subsampling":
            canon = R.canonical_ties(q, s, ref)
            tied += int((canon != ref).any(1).sum())
            assert np.array_equal(R.canonical_ties(q, s, got), got), (kind, i)     # the device puts the lower index first
            ref = canon
        assert np.array_equal(got, ref), (kind, i, int((got != ref).any(1).sum()))
        # padding = the total number of supports; no index leaves the query's own cloud
        so = np.concatenate([[0], np.cumsum(g["lengths"][ss])])
        cloud = np.repeat(np.arange(len(g["lengths"][qs])), g["lengths"][qs])
        real = got != len(s)
        assert ((got >= so[cloud][:, None]) & (got < so[cloud + 1][:, None]))[real].all(), (kind, i)
    print("scene %s: %d subsampling rows reordered inside runs of equal d^2 (fixture: %d rows hold such a run)"
          % (name, tied, g["subsampling_tied_rows"]))


@pytest.mark.parametrize("name", R.SCENES)
def test_whole_device_pyramid(name):
    g = _golden()[0][name]
    d = _device_pyramid(name)
    perms = []                                               # device row of stage i -> golden row
    for i in range(R.NUM_STAGES):
        assert d["points"][i].dtype == torch.float32 and d["lengths"][i].dtype == torch.int64
        assert np.array_equal(d["lengths"][i].cpu().numpy(), g["lengths"][i])
        perms.append(R.match_rows(g["points"][i], d["points"][i].cpu().numpy(), _stage_tol(g, i)))
    assert np.array_equal(perms[0], np.arange(len(perms[0])))
    for kind, n in (("neighbors", R.NUM_STAGES), ("subsampling", R.NUM_STAGES - 1), ("upsampling", R.NUM_STAGES - 1)):
        for i in range(n):
            qs, ss, _, _, ref = _search(g, kind, i)
            got = d[kind][i].cpu().numpy()
            assert d[kind][i].dtype == torch.int64 and got.shape == ref.shape, (kind, i, got.shape, ref.shape)
            # the device matrix in the golden's numbering: row j of the device is golden row perm_q[j]; entries through perm_s (padding stays)
            ps = np.concatenate([perms[ss], [len(perms[ss])]])
            mapped = np.empty_like(got)
            mapped[perms[qs]] = ps[got]
            q, s = g["points"][qs], g["points"][ss]
            if kind == "subsampling":                          # runs of equal d^2 in index order on both sides; every other matrix as it is
                mapped, ref = R.canonical_ties(q, s, mapped), R.canonical_ties(q, s, ref)
            eq, es = _stage_tol(g, qs), _stage_tol(g, ss)
            if eq + es == 0.0:
                assert np.array_equal(mapped, ref), (kind, i)
            else:
                _assert_equal_up_to_moved_points(q, s, mapped, ref, _search(g, kind, i)[2], eq + es, (kind, i))


@pytest.mark.parametrize("name", R.SCENES)
def test_count_histogram(name):
    from diffreg_hip import lib
    g = _golden()[0][name]
    hist = torch.zeros(R.NUM_STAGES, R.HIST_N, dtype=torch.int32, device=DEV)
    for i in range(R.NUM_STAGES):
        p, l = _dev(g["points"][i]), _dev(g["lengths"][i])
        counts = torch.full((p.shape[0],), -1, dtype=torch.int32, device=DEV)
        assert int(lib.radius_count_hist(p, p, l, l, R.RADIUS * 2 ** i, hist[i], counts)) == 0
        assert np.array_equal(counts.cpu().numpy(), g["counts"][i]), i
    once = hist.cpu().numpy()
    assert np.array_equal(once, g["hist"])
    again = torch.zeros_like(hist)
    for rep in range(2):                                      # accumulated over two calls; the second run of the same input is bit-equal
        for i in range(R.NUM_STAGES):
            p, l = _dev(g["points"][i]), _dev(g["lengths"][i])
            lib.radius_count_hist(p, p, l, l, R.RADIUS * 2 ** i, again[i])
        assert np.array_equal(again.cpu().numpy(), (rep + 1) * once)


def test_count_histogram_drops_counts_beyond_hist_n():
    """200 points inside one ball of radius 0.0625 next to 40 scattered ones: the cluster's counts (>= 200) fall off a 180-bin histogram, are
    written nowhere (guard bins on either side of the histogram stay as they were), and come back whole in `counts`"""
    from diffreg_hip import lib
    rng = np.random.default_rng(3)
    cluster = (rng.random((200, 3)) * 0.02).astype(np.float32)
    far = (1.0 + rng.random((40, 3)) * 3.0).astype(np.float32)
    p = np.concatenate([cluster, far], 0)
    d2 = ((p[:, None, :].astype(np.float64) - p[None, :, :]) ** 2).sum(-1)
    ref = (d2 < 0.0625 ** 2).sum(1)                           # (no d^2 of this set lies within float32 rounding of r^2: asserted below)
    assert (np.abs(d2 - 0.0625 ** 2) > 1e-6).all() and (ref[:200] >= 200).all() and (ref[200:] < R.HIST_N).all()
    guard = torch.full((R.HIST_N + 128,), 7, dtype=torch.int32, device=DEV)
    hist = guard[64:64 + R.HIST_N]
    hist.zero_()
    counts = torch.empty(len(p), dtype=torch.int32, device=DEV)
    l = torch.tensor([len(p)], device=DEV)
    lib.radius_count_hist(_dev(p), _dev(p), l, l, 0.0625, hist, counts)
    assert np.array_equal(counts.cpu().numpy(), ref)
    assert np.array_equal(hist.cpu().numpy(), np.bincount(ref, minlength=512)[:R.HIST_N])
    assert int(hist.sum()) == 40
    out = guard.cpu().numpy()
    assert (out[:64] == 7).all() and (out[64 + R.HIST_N:] == 7).all()


def test_count_histogram_graph_capture():
    from diffreg_hip import lib
    g = _golden()[0]["two"]
    p, l = _dev(g["points"][0]), _dev(g["lengths"][0]).to(torch.int32)
    eager = torch.zeros(R.HIST_N, dtype=torch.int32, device=DEV)
    lib.radius_count_hist(p, p, l, l, R.RADIUS, eager)
    torch.cuda.synchronize()
    cap = torch.zeros(R.HIST_N, dtype=torch.int32, device=DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.radius_count_hist(p, p, l, l, R.RADIUS, cap)
    cap.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(cap.cpu().numpy(), eager.cpu().numpy()) and np.array_equal(eager.cpu().numpy(), g["hist"][0])


@pytest.mark.parametrize("threshold", R.THRESHOLDS)
def test_calibration(threshold):
    from diffreg_hip import pyramid2d3d as P
    scenes, limits = _golden()
    data = [(torch.from_numpy(scenes[s]["points"][0]), torch.from_numpy(scenes[s]["lengths"][0])) for s in R.SCENES]
    seen = []

    def samples():
        for item in data:
            seen.append(1)
            yield item
    got = P.calibrate_neighbors_pack_mode(samples(), R.NUM_STAGES, R.VOXEL, R.RADIUS, keep_ratio=R.KEEP_RATIO, sample_threshold=threshold,
                                          device=DEV)
    ref, used = limits[threshold]
    assert np.array_equal(np.asarray(got), ref), (got, ref)
    assert len(seen) == used                                  # the reference's stopping rule: no sample is read past the threshold


def _module():
    m = B.PointBackbone()
    m.load_state_dict({**m.state_dict(), **B.make_weights(m)})
    return m.to(DEV)


def _rel(dev, ref):
    dev, ref = dev.detach().double().cpu(), ref.detach().double().cpu()
    assert dev.shape == ref.shape
    return float((dev - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


@pytest.mark.parametrize("name", ["sparse", "dense"])
def test_backbone_on_device_pyramid(name):
    """the device pyramid fed to the device point backbone against the golden pyramid fed to it: fine features row for row, the two coarser
    outputs after the stage's permutation; bar 1e-4 of the tensor's maximum (tests/test_pcd_backbone2d3d_gpu.py)"""
    from diffreg_hip import pcd_backbone2d3d as PB
    g = _golden()[0][name]
    d = _device_pyramid(name)
    ref_pyr = {k: [_dev(a) for a in g[k]] for k in ("points", "neighbors", "subsampling", "upsampling")}
    m = _module()
    feats = torch.ones(g["points"][0].shape[0], 1, device=DEV)
    with torch.no_grad():
        outs = PB.point_backbone(m, feats, d)
        refs = PB.point_backbone(m, feats, ref_pyr)
    for i, (o, r) in enumerate(zip(outs, refs)):
        perm = torch.from_numpy(R.match_rows(g["points"][i], d["points"][i].cpu().numpy(), _stage_tol(g, i))).to(DEV)
        e = _rel(o, r[perm])
        print("scene %s out%d %s: |device pyramid - golden pyramid| / max = %.2e" % (name, i, tuple(o.shape), e))
        assert e <= 1e-4, i


class _StandIn(torch.nn.Module):
    """the attributes of MATR2D3D the overlay touches; forward returns the dict it was given"""

    def __init__(self):
        super().__init__()
        self.transformer, self.coarse_matching = torch.nn.Module(), torch.nn.Module()
        self.denoising_transformer, self.denoising_coarse_matching = torch.nn.Module(), torch.nn.Module()

    def get_warped_from_noising_matching3D3D(self, *a):
        return a

    def forward(self, data_dict):
        return data_dict


def test_overlay_pyramid_flag():
    from diffreg_hip.overlay2d3d import accelerate
    g = _golden()[0]["two"]
    model = _StandIn()
    ov = accelerate(model)
    assert "forward" not in model.__dict__                    # the default touches nothing
    ov.remove()
    ov = accelerate(model, partition=True, pyramid=dict(num_stages=R.NUM_STAGES, voxel_size=R.VOXEL, search_radius=R.RADIUS,
                                                       neighbor_limits=list(R.LIMITS)))
    assert "forward" in model.__dict__
    image = torch.zeros(1, 3, 4, 4, device=DEV)
    out = model({"points": _dev(g["points"][0]), "lengths": _dev(g["lengths"][0]), "image": image})
    want = _device_pyramid("two")
    assert out["image"] is image and set(out) == {"points", "lengths", "neighbors", "subsampling", "upsampling", "image"}
    for k in ("points", "lengths", "neighbors", "subsampling", "upsampling"):
        assert isinstance(out[k], list) and len(out[k]) == len(want[k])
        for a, b in zip(out[k], want[k]):
            assert a.dtype == b.dtype and torch.equal(a, b), k
    lists = dict(out)
    members = {k: list(v) if isinstance(v, list) else v for k, v in lists.items()}
    again = model(lists)                                      # a dict that already carries the lists passes through untouched
    assert again is lists and all(again[k] is lists[k] for k in lists)
    assert all(all(x is y for x, y in zip(again[k], members[k])) for k in members if isinstance(members[k], list))
    ov.remove()
    assert "forward" not in model.__dict__
    raw = {"points": _dev(g["points"][0]), "lengths": _dev(g["lengths"][0])}
    assert torch.is_tensor(model(raw)["points"])              # the model's own forward again


def test_kpconv_origin_entry_does_not_reproduce_the_origin_scene():
    """the reason dr_grid_subsample_vision3d_f32 exists, on the device: dr_grid_subsample_f32 (KPConv's origin) occupies another number of voxels
    at stages 1 and 2 of scene "origin", at every stage the number tests/pyramid2d3d_ref.occupied_voxels gives for that origin in numpy float32"""
    from diffreg_hip import lib
    g = _golden()[0]["origin"]
    for i in range(1, R.NUM_STAGES):
        v, prev = R.VOXEL * 2 ** i, g["points"][i - 1]
        _, ol, tot, status = lib.grid_subsample(_dev(prev), _dev(g["lengths"][i - 1]), v)
        assert int(status) == 0
        assert int(tot) == int(ol[0]) == R.occupied_voxels(prev, R.origin_forms(prev.min(0), v)[1], v), i
        assert i == R.NUM_STAGES - 1 or int(tot) != len(g["points"][i]), i


def test_refusals():
    from diffreg_hip import lib, pyramid2d3d as P
    from diffreg_hip.overlay2d3d import accelerate
    with pytest.raises(NotImplementedError, match="65"):
        P.GraphPyramid2D3DCollate(4, R.VOXEL, R.RADIUS, [40, 65, 36, 36])
    model = _StandIn()
    with pytest.raises(NotImplementedError, match="65"):
        accelerate(model, pyramid=dict(num_stages=1, voxel_size=R.VOXEL, search_radius=R.RADIUS, neighbor_limits=[65]))
    assert "forward" not in model.__dict__ and "_dr_overlay" not in model.__dict__
    p = torch.rand(50, 3, generator=torch.Generator().manual_seed(11)).to(DEV)
    l = torch.tensor([50], device=DEV)
    with pytest.raises(NotImplementedError, match="65"):
        P.radius_search_pack_mode(p, p, l, l, 0.1, 65)
    with pytest.raises(RuntimeError, match="invalid argument"):           # the entry itself: limits above 64 stay DR_EINVAL
        lib.radius_neighbors(p, p, l, l, 0.1, 65)
    raw, ptr = lib.raw(), lib.ptr
    l32 = l.to(torch.int32)
    hist = torch.zeros(8, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    wsb = raw.dr_radius_count_hist_workspace_bytes(50, 50, 1)
    assert wsb == raw.dr_radius_neighbors_workspace_bytes(50, 50, 1) > 0
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    call = lambda nq=50, ns=50, nb=1, q=p, s=p, ql=l32, sl=l32, r=0.25, hn=8, h=hist, st=status, w=ws, wb=wsb: raw.dr_radius_count_hist_f32(
        nq, ns, nb, ptr(q), ptr(s), ptr(ql), ptr(sl), r, hn, ptr(h), None, ptr(st), ptr(w), wb, None)
    EINVAL, EWORKSPACE = -1, -4
    assert call(hn=0) == EINVAL and call(hn=4097) == EINVAL and call(r=0.0) == EINVAL and call(r=float("nan")) == EINVAL
    assert call(nb=0) == EINVAL and call(nq=-1) == EINVAL and call(h=None) == EINVAL and call(st=None) == EINVAL
    assert call(ql=None) == EINVAL and call(q=None) == EINVAL and call(s=None) == EINVAL
    assert call(wb=wsb - 1) == EWORKSPACE and call(w=None) == EWORKSPACE
    torch.cuda.synchronize()
    assert int(hist.sum()) == 0                               # a refused call launched nothing
    assert call() == 0
    torch.cuda.synchronize()
    cnt = ((p[:, None] - p[None]).double().pow(2).sum(-1) < 0.25 ** 2).sum(1)
    assert int(hist.sum()) == int((cnt < 8).sum())
