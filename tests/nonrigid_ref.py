"""Float64 numpy statement of the non-rigid ICP path (2D-3D vision3d/ops/deformation_graph.py:26-103, embedded_deformation.py:31-66,
nonrigid_icp_adam.py:9-131), the scenes of tests/golden/nonrigid.npz, and the bar the device entries are held to.

The gradient is written out by hand (the solver has to run without autograd); torch_cost() states the same cost in torch so that a test can hold
both this file's gradient and the device's to float64 autograd.  The kNN is brute force, ascending by distance and by index on ties."""
import numpy as np

STEPS = (1, 2, 10, 11, 50, 500)      # iteration counts whose full Adam state the fixture records (2 and 11: the teacher-forced step's targets)
STATES = (0, 1, 10)                  # iteration counts at whose state cost, gradient and warp are recorded
WEIGHTS = (1.0, 0.1, 0.1)            # landmark, ARAP, orthogonality (nonrigid_icp_adam.py:72)
ADAM = dict(lr=0.5, gamma=0.999, beta1=0.9, beta2=0.999, eps=1e-8)
SCENES = ("a", "b", "c", "d", "e")


# ------------------------------------------------------------------------------------------------ scenes
def _deform(p, rng):
    """a smooth non-rigid motion: a small rotation about z, a translation and a sine bend"""
    a = 0.25
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    q = p @ R.T + np.array([0.30, -0.20, 0.15])
    q[:, 2] += 0.15 * np.sin(2.0 * p[:, 0])
    return q + 0.002 * rng.standard_normal(p.shape)


def make_scene(name):
    """float32 inputs of scene `name`: cloud [C, 3] (the points the graph is built on), nodes [M, 3], corr (rows of the cloud), tgt [N, 3], K, coverage.
    "e" is "c" with hand-set -1 anchors (see holes())."""
    spec = {"a": (3, 1, 3, 1, 11), "b": (700, 2, 700, 4, 12), "c": (300, 40, 120, 4, 13), "d": (1, 67, 1, 6, 14), "e": (300, 40, 120, 4, 13)}[name]
    C, M, N, K, seed = spec
    rng = np.random.default_rng(seed)
    cloud = rng.uniform(-1.0, 1.0, (C, 3))
    if name in ("c", "e"):
        nodes = cloud[rng.choice(C, M, replace=False)].copy()
    else:
        nodes = rng.uniform(-1.0, 1.0, (M, 3))
    corr = np.sort(rng.choice(C, N, replace=False))
    tgt = _deform(cloud[corr], rng)
    return dict(cloud=cloud.astype(np.float32), nodes=nodes.astype(np.float32), corr=corr.astype(np.int64), tgt=tgt.astype(np.float32), K=K,
                coverage=0.6 if name != "b" else 1.5)


def holes(anchor_indices):
    """scene "e": the anchors of scene "c"'s correspondences with hand-set -1 entries -- every fifth row loses its last column, every eleventh (from row 3) its
    first, and row 5 loses all of them (the graph builder never emits that)"""
    ai = anchor_indices.copy()
    ai[::5, -1] = -1
    ai[3::11, 0] = -1
    ai[5, :] = -1
    return ai


def screen(cloud, nodes, K):
    """the fixture's condition on a scene: in float64 the sorted node distances of every point, up to rank K + 1, differ by more than 1e-5 relative"""
    d = np.sqrt(((cloud[:, None, :].astype(np.float64) - nodes[None].astype(np.float64)) ** 2).sum(-1))
    d = np.sort(d, axis=1)[:, :min(K + 1, nodes.shape[0])]
    if d.shape[1] < 2:
        return np.inf
    gap = (d[:, 1:] - d[:, :-1]) / d[:, 1:]
    return float(gap.min())


def scene_inputs(gold, name):
    """the solver's inputs of scene `name` as the fixture records them (float64 graph of the reference, rounded to float32 where the device reads
    float32)"""
    g = lambda k: gold["%s_%s" % (name, k)]
    corr = g("in_corr")
    return dict(cloud=g("in_cloud"), nodes=g("in_nodes"), tgt=g("in_tgt"), src=g("in_cloud")[corr], corr=corr,
                ai=g("corr_anchor_indices").astype(np.int64), aw=g("graph_anchor_weights")[corr],
                edges=g("graph_edge_indices").astype(np.int64), ew=g("graph_edge_weights"), all_ai=g("graph_anchor_indices").astype(np.int64),
                all_aw=g("graph_anchor_weights"))


# ------------------------------------------------------------------------------------------------ the three functions
def knn(points, nodes, k):
    d = np.sqrt(((points[:, None, :] - nodes[None]) ** 2).sum(-1))
    k = min(k, nodes.shape[0])
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, idx, 1), idx.astype(np.int64)


def skinning(d, c):
    return np.exp(-(d ** 2) / (2.0 * c ** 2))


def build_graph(points, nodes, K, coverage, eps=1e-6):
    points, nodes = points.astype(np.float64), nodes.astype(np.float64)
    ad, ai = knn(points, nodes, K)
    aw = skinning(ad, coverage)
    aw = aw / aw.sum(1, keepdims=True)
    M = nodes.shape[0]
    n2p = np.zeros((M, points.shape[0]))
    n2p[ai, np.arange(points.shape[0])[:, None]] = 1.0
    adj = (n2p @ n2p.T) > 0
    x2 = (nodes ** 2).sum(1)
    dm = np.sqrt(np.clip(x2[:, None] - 2.0 * (nodes @ nodes.T) + x2[None], 0.0, None) + 1e-8)
    wm = skinning(dm, coverage) * adj
    wm = wm / np.clip(wm.sum(-1, keepdims=True), eps, None)
    ei = np.argwhere(adj).astype(np.int64)
    return dict(anchor_indices=ai, anchor_weights=aw, anchor_distances=ad, edge_indices=ei, edge_weights=wm[adj], edge_distances=dm[adj])


def apply_deformation(points, nodes, transforms, ai, aw, eps=1e-6):
    points, nodes, transforms, aw = (np.asarray(x, np.float64) for x in (points, nodes, transforms, aw))
    w = aw / (aw.sum(1, keepdims=True) + eps)
    out = np.zeros_like(points)
    for k in range(ai.shape[1]):
        m = ai[:, k] != -1
        a = ai[m, k]
        R, t = transforms[a, :3, :3], transforms[a, :3, 3]
        out[m] += (np.einsum("nij,nj->ni", R, points[m] - nodes[a]) + t + nodes[a]) * w[m, k:k + 1]
    return out


def to_transforms(rot, trn):
    T = np.tile(np.eye(4), (rot.shape[0], 1, 1))
    T[:, :3, :3] = rot
    T[:, :3, 3] = trn
    return T


def cost_grad(rot, trn, nodes, src, tgt, ai, aw, edges, ew, weights=WEIGHTS, eps=1e-6):
    """-> (terms [3], grad_rot, grad_trn of the weighted sum), all float64"""
    rot, trn, nodes, src, tgt, aw, ew = (np.asarray(x, np.float64) for x in (rot, trn, nodes, src, tgt, aw, ew))
    M, N, E = nodes.shape[0], src.shape[0], edges.shape[0]
    w = aw / (aw.sum(1, keepdims=True) + eps)
    res = apply_deformation(src, nodes, to_transforms(rot, trn), ai, aw, eps) - tgt
    g_r, g_t = np.zeros_like(rot), np.zeros_like(trn)
    with np.errstate(invalid="ignore", divide="ignore"):
        lm = (res ** 2).sum(1).mean() if N else np.nan
        for k in range(ai.shape[1]):
            m = ai[:, k] != -1
            a = ai[m, k]
            wr = res[m] * w[m, k:k + 1] * (2.0 / N) * weights[0]
            np.add.at(g_r, a, wr[:, :, None] * (src[m] - nodes[a])[:, None, :])
            np.add.at(g_t, a, wr)
        i, j = edges[:, 0], edges[:, 1]
        dl = nodes[j] - nodes[i]
        df = np.einsum("eij,ej->ei", rot[i], dl) + nodes[i] + trn[i] - (nodes[j] + trn[j])
        ar = ((df ** 2).sum(1) * ew).mean() if E else np.nan
        if E:
            we = df * ew[:, None] * (2.0 / E) * weights[1]
            np.add.at(g_r, i, we[:, :, None] * dl[:, None, :])
            np.add.at(g_t, i, we)
            np.add.at(g_t, j, -we)
        G = np.einsum("mab,mac->mbc", rot, rot) - np.eye(3)             # columns' Gram matrix minus identity
        orth = ((np.triu(G, 1) ** 2).sum((1, 2)) + (np.diagonal(G, axis1=1, axis2=2) ** 2).sum(1)).mean()
        H = 2.0 * np.triu(G, 1) + 2.0 * np.triu(G, 1).transpose(0, 2, 1)
        H[:, [0, 1, 2], [0, 1, 2]] = 4.0 * np.diagonal(G, axis1=1, axis2=2)
        g_r += np.einsum("mac,mbc->mab", rot, H) * (weights[2] / M)
    return np.array([lm, ar, orth]), g_r, g_t


def adam_run(nodes, src, tgt, ai, aw, edges, ew, num_iterations, record=STEPS, state=None, weights=WEIGHTS, lr=0.5, gamma=0.999, beta1=0.9,
             beta2=0.999, eps=1e-8):
    """torch.optim.Adam + ExponentialLR on the cost above.  -> (states {n: dict(rot, trn, m_rot, m_trn, v_rot, v_trn)}, trace [n, 3]);
    state: a dict of the same names plus step, to start from."""
    M = nodes.shape[0]
    if state is None:
        p = [np.tile(np.eye(3), (M, 1, 1)), np.zeros((M, 3))]
        m, v, step = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p], 0
    else:
        p = [np.array(state["rot"], np.float64), np.array(state["trn"], np.float64)]
        m = [np.array(state["m_rot"], np.float64), np.array(state["m_trn"], np.float64)]
        v = [np.array(state["v_rot"], np.float64), np.array(state["v_trn"], np.float64)]
        step = int(state["step"])
    for _ in range(step):
        lr = lr * gamma
    states, trace = {}, np.zeros((num_iterations, 3))
    for it in range(num_iterations):
        terms, g_r, g_t = cost_grad(p[0], p[1], nodes, src, tgt, ai, aw, edges, ew, weights)
        trace[it] = terms
        step += 1
        bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
        for q, g in enumerate((g_r, g_t)):
            m[q] = m[q] + (g - m[q]) * (1.0 - beta1)
            v[q] = v[q] * beta2 + (1.0 - beta2) * g * g
            p[q] = p[q] - (lr / bc1) * m[q] / (np.sqrt(v[q]) / np.sqrt(bc2) + eps)
        lr = lr * gamma
        if it + 1 in record:
            states[it + 1] = dict(rot=p[0].copy(), trn=p[1].copy(), m_rot=m[0].copy(), m_trn=m[1].copy(), v_rot=v[0].copy(), v_trn=v[1].copy())
    return states, trace


def torch_cost(rot, trn, nodes, src, tgt, ai, aw, edges, ew, weights=WEIGHTS, eps=1e-6):
    """the weighted cost in torch (any dtype), for autograd"""
    import torch
    w = aw / (aw.sum(1, keepdim=True) + eps)
    mask = ai != -1
    a = ai.clamp(min=0)
    warped = (torch.einsum("nkij,nkj->nki", rot[a], src[:, None] - nodes[a]) + trn[a] + nodes[a]) * (w * mask)[..., None]
    lm = ((warped.sum(1) - tgt) ** 2).sum(1).mean()
    i, j = edges[:, 0], edges[:, 1]
    df = torch.einsum("eij,ej->ei", rot[i], nodes[j] - nodes[i]) + nodes[i] + trn[i] - (nodes[j] + trn[j])
    ar = ((df ** 2).sum(1) * ew).mean()
    G = torch.einsum("mab,mac->mbc", rot, rot) - torch.eye(3, dtype=rot.dtype)
    orth = ((torch.triu(G, 1) ** 2).sum((1, 2)) + (torch.diagonal(G, dim1=1, dim2=2) ** 2).sum(1)).mean()
    return weights[0] * lm + weights[1] * ar + weights[2] * orth


# ------------------------------------------------------------------------------------------------ the bar
def bar(ref64, dev32=None):
    """largest allowed deviation from the reference's float64: max(one float32 ulp at the tensor's largest magnitude, 4 x the reference's own
    recorded float32 deviation)"""
    ref64 = np.asarray(ref64, np.float64)
    finite = ref64[np.isfinite(ref64)]
    ulp = float(np.spacing(np.float32(np.abs(finite).max()))) if finite.size else 0.0
    own = 4.0 * float(np.nanmax(np.abs(dev32))) if dev32 is not None and np.size(dev32) else 0.0
    return max(ulp, own)


def ratio(got, ref64, dev32=None):
    """deviation of `got` from ref64 over the bar (<= 1 passes); NaN positions must agree"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref64))
    if not got.size:
        return 0.0
    err = np.abs(got - ref64)
    err = float(np.nanmax(err)) if np.isfinite(err).any() else 0.0
    b = bar(ref64, dev32)
    return err / b if b > 0 else (0.0 if err == 0 else np.inf)
