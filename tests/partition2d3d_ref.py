"""Test-side restatement of the 2D-3D patch partition and ground-truth patch overlaps in plain torch (float64 for the tests, float32 on any device
for tools/partition2d3d_time.py), written against the cited lines in our own words:

    partition            vision3d/ops/point_cloud_partition.py:41-104 (return_count, gather_points)
    patchify             EXP/utils.py:28-56
    node_corr            EXP/utils.py:59-175 (dense k = 1 nearest neighbours in place of KeOps)
    mutual_nn            EXP/utils.py:234-252
    radius_pairs         EXP/utils.py:426-446 (the definition: |T s_i - t_j| < r, ascending (i, j))

EXP = Diff-Reg-2d3d/experiments/2d3dmatr.rgbdv2.stage4.level3.stage1.  Distances are sums of squared differences.  The deterministic scenes the golden
file tests/golden/partition2d3d.npz was minted on (tools/golden/make_golden_partition2d3d.py) are generated here from an integer hash and exactly
rounded arithmetic only (no libm call), so that every platform yields the same float32 inputs; `input_checksum` is stored and checked.

Index outputs are discrete functions of float comparisons: the assert_* helpers demand equality wherever the float64 restatement DECIDES the comparison
and cap the undecided remainder (the rule of tests/helpers.py::assert_match_list_is_the_references).  Margins, from the number formats:
  GAP2   1e-6 m^2  two squared distances closer than this may order either way in float32 (metre-scale coordinates: 1 ulp of 4 m^2 = 4.8e-7)
  GAP3D  1e-6 m    a 3D distance this close to the radius, or two nearest neighbours this close to each other
  GAP2D  1e-4 px   a pixel distance this close to the radius (coordinates up to 630: 1 ulp = 6.1e-5)
  GAPR   1e-5 m    radius_pairs: T s_i in float32 carries three products and three sums at <= 4 m (<= 1e-6 per coordinate) before the distance
"""
import numpy as np
import torch

GAP2, GAP3D, GAP2D, GAPR = 1e-6, 1e-6, 1e-4, 1e-5
CAP_POINTS, CAP_PAIRS, TOL_CENTER = 0.01, 0.05, 1e-5
R2D, R3D, R_MUTUAL = 8.0, 0.0375, 0.06

# rotation with rational entries (no trigonometry): rows are orthonormal, det = +1
_ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])
_TRN = np.array([0.25, -0.5, 0.75])

SCENES = {
    # H, W, coarse grid, stride, points, nodes, point_limit, zero-depth boxes (h0, h1, w0, w1) of the depth and of the second ("_da") depth
    "a": dict(H=476, W=630, Hc=34, Wc=45, stride=2, Nf=20000, Nc=1024, limit=128, holes=[(98, 182, 196, 336)], holes_da=[(300, 360, 60, 150)], seed=1),
    "b": dict(H=476, W=630, Hc=34, Wc=45, stride=2, Nf=20000, Nc=1024, limit=32, holes=[(98, 182, 196, 336)], holes_da=[(300, 360, 60, 150)], seed=1),
    "c": dict(H=56, W=60, Hc=4, Wc=5, stride=2, Nf=600, Nc=40, limit=16, holes=[(14, 28, 24, 36)], holes_da=[(0, 14, 0, 12)], seed=2, far_nodes=6, sparse=True),
    # not in the golden file: the device is held to the float64 restatement alone
    "d": dict(H=64, W=80, Hc=8, Wc=10, stride=1, Nf=3000, Nc=150, limit=64, holes=[(16, 24, 40, 56)], holes_da=[(40, 48, 8, 16)], seed=3),
}


def _hash01(idx, seed):
    """uniform [0, 1) doubles from an integer hash of (idx, seed): 32 mixed bits / 2^32 (exact)"""
    with np.errstate(over="ignore"):
        x = np.asarray(idx, dtype=np.uint64) + np.uint64((seed * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(32)).astype(np.float64) / 4294967296.0


def _depth(h, w, H, W):
    u, v = w / W, h / H
    return 1.5 + 0.4 * (u - 0.5) * (u - 0.5) + 0.3 * u * v - 0.2 * v * v + 0.15 * u * u * u


def make_scene(name):
    """-> dict of float32 / bool CPU tensors: the inputs of EXP/model.py:403-495 for one synthetic RGB-D frame and a cloud sampled from its surface"""
    s = SCENES[name]
    H, W, Nf, Nc, seed = s["H"], s["W"], s["Nf"], s["Nc"], s["seed"]
    f, cx, cy = 0.9 * W, 0.5 * W, 0.5 * H
    hh, ww = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")

    def frame(scale, shift, holes):
        z = _depth(hh, ww, H, W) * scale + shift
        for (h0, h1, w0, w1) in holes:
            z[h0:h1, w0:w1] = 0.0
        pts = np.stack([(ww - cx) * z / f, (hh - cy) * z / f, z], -1).reshape(-1, 3)
        return pts, (z > 0).reshape(-1)
    img_points, img_masks = frame(1.0, 0.0, s["holes"])
    img_points_da, img_masks_da = frame(1.02, 0.01, s["holes_da"])
    img_pixels = np.stack([hh, ww], -1).reshape(-1, 2)
    # the cloud: continuous pixel positions over the whole image (the zero-depth boxes included: there the cloud has points and the image none),
    # on the surface plus millimetre noise, then taken into its own frame by the inverse of `transform`
    i = np.arange(Nf)
    ph, pw = _hash01(4 * i, seed) * (H - 1), _hash01(4 * i + 1, seed) * (W - 1)
    if s.get("sparse"):          # a third of the image holds a twentieth of the points: small nodes
        thin = pw > 0.66 * (W - 1)
        pw = np.where(thin & (_hash01(4 * i + 3, seed + 7) > 0.15), pw * 0.6, pw)
    z = _depth(ph, pw, H, W) + (_hash01(4 * i + 2, seed) - 0.5) * 0.004
    cam = np.stack([(pw - cx) * z / f, (ph - cy) * z / f, z], -1)
    cam[:, :2] += (np.stack([_hash01(4 * i + 3, seed), _hash01(4 * i + 3, seed + 1)], -1) - 0.5) * 0.002
    transform = np.eye(4)
    transform[:3, :3], transform[:3, 3] = _ROT, _TRN
    pcd_points = (cam - _TRN) @ _ROT                                     # R^T (cam - t)
    pcd_points = pcd_points.astype(np.float32)
    transform = transform.astype(np.float32)
    moved = pcd_points.astype(np.float64) @ transform[:3, :3].astype(np.float64).T + transform[:3, 3].astype(np.float64)
    pcd_pixels = np.stack([f * moved[:, 1] / moved[:, 2] + cy, f * moved[:, 0] / moved[:, 2] + cx], -1)      # (h, w), as render(..., rounding=False)
    step = Nf // Nc
    nodes = pcd_points[::step][:Nc].astype(np.float64) + 0.003
    far = s.get("far_nodes", 0)
    if far:                      # nodes that no point is nearest to
        nodes[-far:] += 50.0
    T = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    return dict(img_points=T(img_points), img_points_da=T(img_points_da), img_pixels=T(img_pixels), img_masks=T(img_masks, torch.bool),
                img_masks_da=T(img_masks_da, torch.bool), pcd_points=T(pcd_points), pcd_pixels=T(pcd_pixels), nodes=T(nodes), transform=T(transform),
                H=H, W=W, Hc=s["Hc"], Wc=s["Wc"], stride=s["stride"], limit=s["limit"])


def input_checksum(sc):
    return np.array([float(sc[k].double().sum()) for k in sorted(sc) if torch.is_tensor(sc[k])])


# ------------------------------------------------------------------------------------------------------------------------------------------
# the restatement (dtype / device generic)
# ------------------------------------------------------------------------------------------------------------------------------------------
def _sqdist(a, b):
    """(A, B) squared distances as sums of squared differences, one coordinate at a time (no (A, B, 3) temporary)"""
    d = None
    for k in range(a.shape[1]):
        t = a[:, k, None] - b[None, :, k]
        d = t * t if d is None else d + t * t
    return d


def partition(points, nodes, point_limit, dtype=torch.float64, want_gaps=False):
    """-> dict(point_to_node, node_sizes, node_masks, node_knn_indices (width min(largest node, limit), padding Nf), node_knn_masks[, gap2 per point: second
    nearest node minus nearest, members: per node the full ascending (index, squared distance) lists])"""
    p, n = points.to(dtype), nodes.to(dtype)
    Nf, Nc = p.shape[0], n.shape[0]
    d = _sqdist(n, p)                                                    # (Nc, Nf)
    two = d.topk(min(2, Nc), dim=0, largest=False)
    p2n = two.indices[0]
    own = two.values[0]
    sizes = torch.bincount(p2n, minlength=Nc)
    order = torch.argsort(own, stable=True)
    order = order[torch.argsort(p2n[order], stable=True)]                # by node, then distance, then index
    starts = torch.cumsum(sizes, 0) - sizes
    width = int(min(int(sizes.max()), point_limit))
    col = torch.arange(width, device=p.device)[None]
    valid = col < sizes[:, None]
    at = (starts[:, None] + col).clamp(max=Nf - 1)
    knn = torch.where(valid, order[at], torch.full_like(at, Nf))
    out = dict(point_to_node=p2n, node_sizes=sizes, node_masks=sizes > 0, node_knn_indices=knn, node_knn_masks=valid)
    if want_gaps:
        out["gap2"] = (two.values[1] - two.values[0]) if Nc > 1 else torch.full_like(own, float("inf"))
        out["second"] = two.indices[1] if Nc > 1 else p2n
        o, s, z = order.cpu().numpy(), starts.cpu().numpy(), sizes.cpu().numpy()
        ow = own.cpu().numpy()
        out["members"] = [(o[s[c]:s[c] + z[c]], ow[o[s[c]:s[c] + z[c]]]) for c in range(Nc)]
    return out


def patchify(sc_or_points, points_da=None, pixels=None, masks=None, masks_da=None, H=None, W=None, Hc=None, Wc=None, stride=1):
    """-> the reference's 8-tuple (exact index work: dtype-free)"""
    pts = sc_or_points
    idx = torch.arange(H * W, device=pts.device).view(Hc, H // Hc, Wc, W // Wc).permute(0, 2, 1, 3)[:, :, ::stride, ::stride].reshape(Hc * Wc, -1)
    km, kmd = masks[idx], masks_da[idx]
    return pts[idx], points_da[idx], pixels[idx], idx, km, kmd, km.any(1), kmd.any(1)


def _masked_mean(x, m):
    mf = m.to(x.dtype)[..., None]
    return (x * mf).sum(1) / (mf.sum(1) + 1e-6)


def _nn1(q, s_, chunk):
    """k = 1 (and the runner-up distance) of q (B, A, 3) in s_ (B, C, 3), dense, in chunks of B -> (nearest distance, index, second distance)"""
    d1, ix, d2 = [], [], []
    for b0 in range(0, q.shape[0], chunk):
        qq, ss = q[b0:b0 + chunk], s_[b0:b0 + chunk]
        d = None
        for k in range(3):
            t = qq[:, :, None, k] - ss[:, None, :, k]
            d = t * t if d is None else d + t * t
        v = d.sqrt().topk(min(2, d.shape[-1]), dim=-1, largest=False)
        d1.append(v.values[..., 0]); ix.append(v.indices[..., 0]); d2.append(v.values[..., -1])
    return torch.cat(d1), torch.cat(ix), torch.cat(d2)


def node_corr(img_masks, img_kp, img_kp_da, img_kx, img_km, img_km_da, pcd_masks, pcd_kp, pcd_kx, pcd_km, transform, r2d=R2D, r3d=R3D,
              dtype=torch.float64, chunk=256, want_undecided=False):
    """-> dict(pcd_centers, img_centers, img_centers_da, cand_i, cand_j (row-major), ratio_img, ratio_pcd per candidate (float32 quotients of the counts),
    keep, and the final four lists[, undecided per candidate: see GAP3D / GAP2D])"""
    f = lambda x: x.to(dtype)
    T = f(transform)
    ikp, ikd, ikx, pkx = f(img_kp), f(img_kp_da), f(img_kx), f(pcd_kx)
    pkp = f(pcd_kp) @ T[:3, :3].T + T[None, :3, 3]
    ic, icd, pc = _masked_mean(ikp, img_km), _masked_mean(ikd, img_km_da), _masked_mean(pkp, pcd_km)
    ir = torch.where(img_km, (ikp - ic[:, None]).norm(dim=-1), torch.zeros((), dtype=dtype, device=ikp.device)).max(1).values
    pr = torch.where(pcd_km, (pkp - pc[:, None]).norm(dim=-1), torch.zeros((), dtype=dtype, device=ikp.device)).max(1).values
    hit = (ir[:, None] + pr[None] + r3d - _sqdist(ic, pc).sqrt() > 0) & img_masks[:, None] & pcd_masks[None]
    ci, cj = torch.nonzero(hit, as_tuple=True)
    A, Pp = ikp[ci], pkp[cj]
    Ax, Px, Am, Pm = ikx[ci], pkx[cj], img_km[ci], pcd_km[cj]
    bi = torch.arange(ci.shape[0], device=ci.device)[:, None]

    def side(q, s_, qx, sx, qm, sm):
        d1, ix, d2 = _nn1(q, s_, chunk)
        dx = (qx - sx[bi, ix]).norm(dim=-1)
        ov = (d1 < r3d) & (dx < r2d) & sm[bi, ix] & qm
        und = None
        if want_undecided:
            und = (((d1 - r3d).abs() < GAP3D) | ((dx - r2d).abs() < GAP2D) | (d2 - d1 < GAP3D)) & qm
            und = und.any(1)
        return ov.sum(1), qm.sum(1), und
    oi, ti, ui = side(A, Pp, Ax, Px, Am, Pm)
    op, tp, up = side(Pp, A, Px, Ax, Pm, Am)
    ri, rp = oi.float() / ti.float(), op.float() / tp.float()
    keep = (ri > 0) & (rp > 0)
    out = dict(pcd_centers=pc, img_centers=ic, img_centers_da=icd, cand_i=ci, cand_j=cj, ratio_img=ri, ratio_pcd=rp, keep=keep,
               img_corr_indices=ci[keep], pcd_corr_indices=cj[keep], img_corr_overlaps=ri[keep], pcd_corr_overlaps=rp[keep])
    if want_undecided:
        out["undecided"] = ui | up
    return out


def mutual_nn(src, tgt, radius, dtype=torch.float64, want_undecided=False):
    """-> (2, C) pairs in ascending source order[, per source: undecided]"""
    d = _sqdist(src.to(dtype), tgt.to(dtype)).sqrt()
    s2t = d.topk(min(2, d.shape[1]), dim=1, largest=False)
    t2s = d.topk(min(2, d.shape[0]), dim=0, largest=False)
    j = s2t.indices[:, 0]
    i = torch.arange(d.shape[0], device=d.device)
    ok = (t2s.indices[0][j] == i) & (s2t.values[:, 0] < radius)
    pairs = torch.stack([i[ok], j[ok]], 0)
    if not want_undecided:
        return pairs
    und = ((s2t.values[:, 0] - radius).abs() < GAP3D) | (s2t.values[:, -1] - s2t.values[:, 0] < GAP3D) | ((t2s.values[-1] - t2s.values[0]) < GAP3D)[j]
    return pairs, und


def radius_pairs(src, tgt, transform, radius, dtype=torch.float64):
    """-> ((C, 2) pairs ascending (i, j), the (ns, nt) distance matrix)"""
    s_, t_ = src.to(dtype), tgt.to(dtype)
    if transform is not None:
        T = transform.to(dtype)
        s_ = s_ @ T[:3, :3].T + T[None, :3, 3]
    d = _sqdist(s_, t_).sqrt()
    return torch.nonzero(d < radius), d


def stage_inputs(sc, device="cpu", limit=None):
    """the model's glue between the entries (EXP/model.py:412-416) on the restatement's float64 partition -> the arguments of node_corr"""
    g = lambda k: sc[k].to(device)
    part = partition(g("pcd_points"), g("nodes"), limit or sc["limit"])
    return part, node_corr_inputs(sc, part, device)


def node_corr_inputs(sc, part, device="cpu", patches=None):
    """part: any partition result (dict with node_sizes, node_masks, node_knn_indices, node_knn_masks); patches: a patchify 8-tuple (default: the restatement's)"""
    g = lambda k: sc[k].to(device)
    pm = part["node_masks"] & (part["node_sizes"] > 5)                   # pcd_min_node_size
    pad = lambda x: torch.cat([x, torch.full_like(x[:1], 1e10)], 0)
    kp, kx = pad(g("pcd_points"))[part["node_knn_indices"]], pad(g("pcd_pixels"))[part["node_knn_indices"]]
    if patches is None:
        patches = patchify(g("img_points"), g("img_points_da"), g("img_pixels"), g("img_masks"), g("img_masks_da"), sc["H"], sc["W"], sc["Hc"], sc["Wc"], sc["stride"])
    ip, ipd, ix, _, im, imd, nm, nmd = patches
    return dict(img_masks=nm, img_masks_da=nmd, img_kp=ip, img_kp_da=ipd, img_kx=ix, img_km=im, img_km_da=imd, pcd_masks=pm, pcd_kp=kp, pcd_kx=kx,
                pcd_km=part["node_knn_masks"], transform=g("transform"))


def reference_args(a):
    """node_corr_inputs -> the positional arguments of get_2d3d_node_correspondences (EXP/utils.py:59-74)"""
    return (a["img_masks"], a["img_masks_da"], a["img_kp"], a["img_kp_da"], a["img_kx"], a["img_km"], a["img_km_da"], a["pcd_masks"], a["pcd_kp"], a["pcd_kx"],
            a["pcd_km"], a["transform"], R2D, R3D)


def ref_node_corr(a, **kw):
    return node_corr(a["img_masks"], a["img_kp"], a["img_kp_da"], a["img_kx"], a["img_km"], a["img_km_da"], a["pcd_masks"], a["pcd_kp"], a["pcd_kx"], a["pcd_km"],
                     a["transform"], **kw)


# ------------------------------------------------------------------------------------------------------------------------------------------
# comparisons: `got` = the reference's golden arrays or the device's outputs (numpy), `ref` = the float64 restatement with its gaps
# ------------------------------------------------------------------------------------------------------------------------------------------
def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def assert_partition_matches(got, ref, Nf, limit, label=""):
    """got: dict(point_to_node, node_sizes, node_masks, node_knn_indices, node_knn_masks) -> (undecided points, nodes they touch, positions compared as sets)"""
    p2n, gap, second = _np(ref["point_to_node"]), _np(ref["gap2"]), _np(ref["second"])
    und = gap < GAP2
    assert und.mean() <= CAP_POINTS, (label, "undecided points over the cap", float(und.mean()))
    g_p2n = _np(got["point_to_node"])
    assert np.array_equal(g_p2n[~und], p2n[~und]), (label, "a decided point sits in another node", int((g_p2n[~und] != p2n[~und]).sum()))
    assert ((g_p2n[und] == p2n[und]) | (g_p2n[und] == second[und])).all(), (label, "an undecided point went to a third node")
    touched = np.zeros(len(ref["members"]), dtype=bool)
    touched[p2n[und]] = True
    touched[second[und]] = True
    sizes, g_sizes = _np(ref["node_sizes"]), _np(got["node_sizes"])
    assert np.array_equal(g_sizes[~touched], sizes[~touched]), (label, "node_sizes")
    assert np.array_equal(_np(got["node_masks"])[~touched], sizes[~touched] > 0), (label, "node_masks")
    assert int(g_sizes.sum()) == Nf and np.array_equal(g_sizes, np.bincount(g_p2n, minlength=len(sizes))), (label, "node_sizes are not the counts of point_to_node")
    knn, km = _np(got["node_knn_indices"]), _np(got["node_knn_masks"])
    width = knn.shape[1]
    if not touched[np.argmax(sizes)]:
        assert width == min(int(sizes.max()), limit), (label, "width", width)
    n_set = 0
    for c in np.nonzero(~touched)[0]:
        idx, dist = ref["members"][c]
        n = min(len(idx), width)
        assert np.array_equal(km[c], np.arange(width) < n) and (knn[c, n:] == Nf).all(), (label, "padding / masks of node", int(c))
        if n == 0:
            continue
        brk = np.nonzero(np.diff(dist) >= GAP2)[0] + 1                  # a run of neighbours closer than GAP2 to each other compares as a set
        a = 0
        for b in list(brk) + [len(idx)]:
            if a >= n:
                break
            e = min(b, n)
            if b - a == 1:
                assert knn[c, a] == idx[a], (label, "order inside node", int(c), a)
            else:
                seg = knn[c, a:e]
                assert len(set(seg.tolist())) == e - a and set(seg.tolist()) <= set(idx[a:b].tolist()), (label, "tie run of node", int(c), a, b)
                n_set += e - a
            a = b
    return int(und.sum()), int(touched.sum()), n_set


def assert_overlaps_match(got, ref, N, label=""):
    """got: dict(img_corr_indices, pcd_corr_indices, img_corr_overlaps, pcd_corr_overlaps, pcd_centers, img_centers, img_centers_da); ref: node_corr(...,
    want_undecided=True) -> (pairs, undecided among them)"""
    for k in ("pcd_centers", "img_centers", "img_centers_da"):
        e = float(np.abs(_np(got[k]).astype(np.float64) - _np(ref[k])).max())
        assert e <= TOL_CENTER, (label, k, e)
    ck = _np(ref["cand_i"]).astype(np.int64) * N + _np(ref["cand_j"])            # ascending: row-major order
    und, keep = _np(ref["undecided"]), _np(ref["keep"])
    assert und[keep].mean() <= CAP_PAIRS if keep.any() else True, (label, "undecided pairs over the cap", float(und[keep].mean()))
    gk = _np(got["img_corr_indices"]).astype(np.int64) * N + _np(got["pcd_corr_indices"])
    assert (np.diff(gk) > 0).all(), (label, "pairs are not in row-major order")
    at = np.searchsorted(ck, gk)
    assert (at < len(ck)).all() and np.array_equal(ck[np.minimum(at, len(ck) - 1)], gk), (label, "a pair that is no candidate of the float64 restatement")
    g_dec = ~und[at]
    r_dec = keep & ~und
    assert np.array_equal(gk[g_dec], ck[r_dec]), (label, "decided pairs differ", int(g_dec.sum()), int(r_dec.sum()))
    for k, r in (("img_corr_overlaps", "ratio_img"), ("pcd_corr_overlaps", "ratio_pcd")):
        a, b = _np(got[k])[g_dec].astype(np.float32), _np(ref[r])[r_dec].astype(np.float32)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (label, k, "not bit-equal on decided pairs", int((a != b).sum()))
    return len(gk), int(und[keep].sum())


def assert_mutual_matches(got, src, tgt, radius, label=""):
    pairs, und = mutual_nn(src, tgt, radius, want_undecided=True)
    pairs, und, got = _np(pairs), _np(und), _np(got)
    assert got.shape[0] == 2 and (np.diff(got[0]) > 0).all(), (label, "sources not ascending")
    gd, rd = ~und[got[0]], ~und[pairs[0]]
    assert np.array_equal(got[:, gd], pairs[:, rd]), (label, "decided mutual pairs differ")
    return pairs.shape[1], int(und.sum())


def assert_radius_pairs_match(got, src, tgt, transform, radius, label=""):
    """got (C, 2): every pair decidedly inside is present, none decidedly outside, ascending (i, j), no duplicates"""
    _, d = radius_pairs(src, tgt, transform, radius)
    d, got = _np(d), _np(got).reshape(-1, 2)
    key = got[:, 0].astype(np.int64) * d.shape[1] + got[:, 1]
    assert (np.diff(key) > 0).all(), (label, "pairs not in ascending (i, j) order")
    m = np.zeros(d.shape, dtype=bool)
    m[got[:, 0], got[:, 1]] = True
    assert m[d < radius - GAPR].all(), (label, "a pair inside the radius is missing")
    assert not m[d > radius + GAPR].any(), (label, "a pair outside the radius is listed")
    return int((d < radius).sum()), int((np.abs(d - radius) <= GAPR).sum())
