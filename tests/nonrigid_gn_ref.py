"""Float64 numpy statement of the Gauss-Newton non-rigid ICP (2D-3D vision3d/layers/nonrigid_icp.py:18-154, so3.py:107-133 and :389-406,
numeric.py:7-9), the scenes and forms of tests/golden/nonrigid_gn.npz, and helpers the CPU and GPU tests share.

The normal equations are accumulated as 6 x 6 blocks per (node, partner node), the way the device gathers them: the Jacobian is never built.  The
unknowns are ordered as the reference's permute(1, 3, 0, 2, 4) orders them: axis-angle increments (3 n + d), then translations (3 M + 3 n + d)."""
import numpy as np

from tests import nonrigid_ref as R

BLOCK = 64                           # the factorisation's block width (csrc/nonrigid_gn_index.h: NRG_B)
ITERS = (1, 2, 5)                    # iteration counts whose transforms the fixture records
RECORD = 2                           # A / b / x are recorded for the first RECORD iterations (states: identity, after iteration 1)
# new scenes, chosen for BLOCK: name -> (cloud points, nodes, correspondences, K, seed)
#   f: 6 M = 60, the largest below one block;  g: 6 M = 192 = 3 blocks exactly;  h: 6 M = 66, the smallest above one block;
#   i: 6 M = 150, three block columns with a ragged last one (22)
NEW = {"f": (200, 10, 80, 4, 21), "g": (300, 32, 120, 6, 23), "h": (200, 11, 80, 3, 22), "i": (300, 25, 150, 4, 23)}
# (seeds: the first from 21 / 22 on whose scene passes the kNN gap screen of the mint tool)
SCENES = R.SCENES + tuple(NEW)
# forms: name -> (corr_lambda, arap_lambda, lm_lambda, corr_weights given, edge_weights given)
FORMS = {"fn": (1.0, 0.1, 0.1, False, True),         # the function's defaults
         "mod": (1.0, 1.0, 0.01, True, True),        # the module's defaults, per-correspondence weights
         "now": (1.0, 0.1, 0.1, False, False),       # edge_weights=None
         "noarap": (1.0, 0.0, 0.1, True, True)}      # arap_lambda = 0: no ARAP rows
A_FULL = 70                          # A is recorded in full for scenes with 6 M <= A_FULL (all forms) ...
A_PACKED = {"c": ("fn", "mod"), "e": ("mod",), "g": ("fn", "mod"), "i": ("fn", "mod", "now", "noarap")}   # ... and as its packed lower triangle here
WARP = ("c", "i")                    # scenes whose whole cloud is warped by the reference with its transforms after 5 iterations (form "fn")
FILES = ("nonrigid_gn.npz", "nonrigid_gn_A.npz")     # inputs, b, x, transforms, warps | the recorded A (each file below 1 MiB)


def has_A(scene, form, M):
    return 6 * M <= A_FULL or form in A_PACKED.get(scene, ())


def load(golden_dir):
    """both fixture files as one dict-like of arrays"""
    import os
    out = {}
    for f in FILES:
        with np.load(os.path.join(golden_dir, f)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def make_scene(name):
    if name in R.SCENES:
        return R.make_scene(name)
    C, M, N, K, seed = NEW[name]
    rng = np.random.default_rng(seed)
    cloud = rng.uniform(-1.0, 1.0, (C, 3))
    nodes = cloud[rng.choice(C, M, replace=False)].copy()
    corr = np.sort(rng.choice(C, N, replace=False))
    tgt = R._deform(cloud[corr], rng)
    return dict(cloud=cloud.astype(np.float32), nodes=nodes.astype(np.float32), corr=corr.astype(np.int64), tgt=tgt.astype(np.float32), K=K,
                coverage=0.6)


def corr_weights(n, seed=5):
    """per-correspondence weights in (0.05, 1], one exact zero when there are at least three"""
    w = np.random.default_rng(seed).uniform(0.05, 1.0, n).astype(np.float32)
    if n >= 3:
        w[2] = 0.0
    return w


def scene_inputs(gold, name):
    """the solver's float32 inputs of scene `name` as the fixture records them"""
    g = lambda k: gold["%s_in_%s" % (name, k)]
    return dict(nodes=g("nodes"), src=g("src"), tgt=g("tgt"), ai=g("ai").astype(np.int64), aw=g("aw"), edges=g("edges").astype(np.int64),
                ew=g("ew"), cw=g("cw"), cloud=g("cloud"), all_ai=g("all_ai").astype(np.int64), all_aw=g("all_aw"))


def form_args(inp, form):
    lc, la, lm, has_cw, has_ew = FORMS[form]
    return dict(corr_lambda=lc, arap_lambda=la, lm_lambda=lm, corr_weights=inp["cw"] if has_cw else None,
                edge_weights=inp["ew"] if has_ew else None)


# ------------------------------------------------------------------------------------------------ the algorithm
def skew(v):
    x, y, z = v
    return np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])


def exp_so3(phi):
    """axis_angle_to_rotation_matrix: omega = phi / max(|phi|, 1e-6), I + sin K + (1 - cos) K^2"""
    theta = np.sqrt((phi * phi).sum())
    K = skew(phi / max(theta, 1e-6))
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def unknown(M, n, i):
    return 3 * n + i if i < 3 else 3 * M + 3 * n + (i - 3)


def normal_blocks(rot, trn, nodes, src, tgt, ai, aw, edges, corr_lambda=1.0, arap_lambda=0.1, lm_lambda=0.1, corr_weights=None,
                  edge_weights=None, later_column_wins=True):
    """-> (blocks {(n, m): 6 x 6}, rhs [M, 6]) of one iteration: A = J^T J + lm I, b = -J^T r, accumulated block by block"""
    rot, trn, nodes, src, tgt, aw = (np.asarray(x, np.float64) for x in (rot, trn, nodes, src, tgt, aw))
    M, N = nodes.shape[0], src.shape[0]
    blocks, rhs = {}, np.zeros((M, 6))

    def add(n, m, v):
        blocks[(n, m)] = blocks.get((n, m), np.zeros((6, 6))) + v

    T = R.to_transforms(rot, trn)
    res = corr_lambda * (R.apply_deformation(src, nodes, T, ai, aw) - tgt) if N else np.zeros((0, 3))
    for c in range(N):
        cols = {}
        for k in range(ai.shape[1]):
            if ai[c, k] != -1 and aw[c, k] > 0.0:
                if later_column_wins or int(ai[c, k]) not in cols:
                    cols[int(ai[c, k])] = k
        J = {}
        for n, k in cols.items():
            w = aw[c, k] * (np.sqrt(np.float64(corr_weights[c])) if corr_weights is not None else 1.0)
            J[n] = np.concatenate([-corr_lambda * w * skew(rot[n] @ (src[c] - nodes[n])), corr_lambda * w * np.eye(3)], axis=1)
        for n in J:
            rhs[n] -= J[n].T @ res[c]
            for m in J:
                add(n, m, J[n].T @ J[m])
    if arap_lambda > 0:
        for e in range(edges.shape[0]):
            u, v = int(edges[e, 0]), int(edges[e, 1])
            if u == v:
                continue
            s = arap_lambda * (np.sqrt(np.float64(edge_weights[e])) if edge_weights is not None else 1.0)
            d = rot[u] @ (nodes[v] - nodes[u])
            r = s * (d + trn[u] + nodes[u] - nodes[v] - trn[v])
            Ju = np.concatenate([-s * skew(d), s * np.eye(3)], axis=1)
            Jv = np.concatenate([np.zeros((3, 3)), -s * np.eye(3)], axis=1)
            rhs[u] -= Ju.T @ r
            rhs[v] -= Jv.T @ r
            add(u, u, Ju.T @ Ju); add(u, v, Ju.T @ Jv); add(v, u, Jv.T @ Ju); add(v, v, Jv.T @ Jv)
    for n in range(M):
        add(n, n, lm_lambda * np.eye(6))
    return blocks, rhs


def dense(blocks, rhs):
    """the blocks scattered into A [6 M, 6 M] and b [6 M] in the reference's order of the unknowns (for the solve only)"""
    M = rhs.shape[0]
    A, b = np.zeros((6 * M, 6 * M)), np.zeros(6 * M)
    idx = lambda n: [unknown(M, n, i) for i in range(6)]
    for (n, m), v in blocks.items():
        A[np.ix_(idx(n), idx(m))] += v
    for n in range(M):
        b[idx(n)] = rhs[n]
    return A, b


def update(rot, trn, x):
    M = rot.shape[0]
    rot2 = np.stack([exp_so3(x[3 * n:3 * n + 3]) @ rot[n] for n in range(M)]) if M else rot.copy()
    return rot2, trn + x[3 * M:].reshape(M, 3)


def gauss_newton(nodes, src, tgt, ai, aw, edges, num_iterations=5, record=None, state=None, **kw):
    """-> (rot, trn, trace); trace[it] = dict(A, b, x) for it < record; state: (rot, trn) to start from"""
    M = nodes.shape[0]
    rot, trn = (np.tile(np.eye(3), (M, 1, 1)), np.zeros((M, 3))) if state is None else (np.array(state[0], np.float64), np.array(state[1], np.float64))
    trace = []
    for it in range(num_iterations):
        A, b = dense(*normal_blocks(rot, trn, nodes, src, tgt, ai, aw, edges, **kw))
        x = np.linalg.solve(A, b)
        if record is not None and it < record:
            trace.append(dict(A=A, b=b, x=x))
        rot, trn = update(rot, trn, x)
    return rot, trn, trace


def tril_pack(A):
    return A[np.tril_indices(A.shape[0])]


def to34(rot, trn):
    return np.concatenate([rot, trn[:, :, None]], axis=2)


def to44(T34):
    T = np.tile(np.eye(4), (T34.shape[0], 1, 1))
    T[:, :3, :] = T34
    return T
