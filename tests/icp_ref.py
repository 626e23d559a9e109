"""The statement of dr_icp_p2p_f32's rule (include/diffreg_hip.h) in numpy, in float64 and in float32, with brute-force nearest neighbours and
ties to the lowest index; the float64 statement of dr_grid_subsample_open3d_f32; and the scenes, screens and margins of tests/golden/icp.npz.

The reference's multi_scale_icp (vision3d/utils/open3d.py:378-396) calls Open3D only, and Open3D is not part of this project's environment:
parity with Open3D itself is not claimed.  The published loop of registration_icp with TransformationEstimationPointToPoint(False) is stated
here, and the kernels are held to this statement."""
import numpy as np

RANK_TOL = 1e-12
ST_DEGENERATE, ST_EMPTY = 16, 32
GAP, CONV_LO, CONV_HI = 1e-5, 1e-7, 1e-5        # the screens' margins


def move(T, src, dtype):
    T, s = np.asarray(T, dtype), np.asarray(src, dtype)
    return np.stack([((T[i, 0] * s[:, 0] + T[i, 1] * s[:, 1]) + T[i, 2] * s[:, 2]) + T[i, 3] for i in range(3)], 1).reshape(-1, 3)


def sq_dists(moved, tgt, dtype):
    t = np.asarray(tgt, dtype)
    dx, dy, dz = moved[:, None, 0] - t[None, :, 0], moved[:, None, 1] - t[None, :, 1], moved[:, None, 2] - t[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def evaluate(T, src, tgt, r, dtype, want_d2=False):
    moved = move(T, src, dtype)
    n_src, n_tgt = len(moved), len(tgt)
    corr, best = np.full(n_src, -1, np.int64), np.zeros(n_src, dtype)
    d2 = None
    if n_src and n_tgt:
        d2 = sq_dists(moved, tgt, dtype)
        j = d2.argmin(1)                                     # numpy: the first of equal minima
        v = d2[np.arange(n_src), j]
        ok = v < dtype(r) * dtype(r)
        corr, best = np.where(ok, j, -1), np.where(ok, v, dtype(0))
    n = int((corr >= 0).sum())
    fitness = dtype(n / n_src) if n_src else dtype(0)
    rmse = dtype(np.sqrt(best.astype(np.float64).sum() / n)) if n else dtype(0)
    out = dict(moved=moved, corr=corr, n=n, fitness=fitness, rmse=rmse)
    if want_d2:
        out["d2"] = d2
    return out


def fit(p, q):
    """rule 1 with unit weights and eps = 0, in double -> (4 x 4 update, status bits)"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    pc, qc = p.sum(0) / len(p), q.sum(0) / len(p)
    H = (p - pc).T @ (q - qc) / len(p)
    U4, flags = np.eye(4), 0
    if not np.any(H):
        flags = ST_DEGENERATE
    else:
        U, S, Vt = np.linalg.svd(H)
        if S[1] <= RANK_TOL * S[0]:
            flags = ST_DEGENERATE
        V = Vt.T
        U4[:3, :3] = V @ np.diag([1.0, 1.0, np.sign(np.linalg.det(V @ U.T))]) @ U.T
    U4[:3, 3] = qc - U4[:3, :3] @ pc
    return U4, flags


def icp(src, tgt, init, r, max_iteration, relative_fitness, relative_rmse, dtype=np.float64, trace=None):
    """the loop -> dict(transform, fitness, rmse, iterations, status, corr); trace receives every evaluation (with its d2 matrix)"""
    T = np.eye(4, dtype=dtype) if init is None else np.array(init, dtype)
    T[3] = [0, 0, 0, 1]
    tgt_d = np.asarray(tgt, dtype)
    res = evaluate(T, src, tgt, r, dtype, trace is not None)
    if trace is not None:
        trace.append(dict(res, T=T.copy()))
    its, status = 0, 0
    while True:
        if res["n"] == 0:
            status |= ST_EMPTY
            break
        if its >= max_iteration:
            break
        keep = res["corr"] >= 0
        U4, flags = fit(res["moved"][keep], tgt_d[res["corr"][keep]])
        status |= flags
        T = (U4 @ T.astype(np.float64)).astype(dtype)
        T[3] = [0, 0, 0, 1]
        its += 1
        new = evaluate(T, src, tgt, r, dtype, trace is not None)
        if trace is not None:
            trace.append(dict(new, T=T.copy()))
        stop = abs(res["fitness"] - new["fitness"]) < dtype(relative_fitness) and abs(res["rmse"] - new["rmse"]) < dtype(relative_rmse)
        res = new
        if stop:
            if res["n"] == 0:
                status |= ST_EMPTY
            break
    return dict(transform=T, fitness=res["fitness"], rmse=res["rmse"], iterations=its, status=status, corr=res["corr"])


def voxel_down_sample(points, voxel, dtype=np.float64):
    """Open3D's origin, min - 0.5 voxel; the barycentres in ascending (iz, iy, ix) -> (points, the voxel of every input row, the least
    distance of a coordinate to a voxel wall in voxels)"""
    p = np.asarray(points, dtype)
    if len(p) == 0:
        return p.reshape(0, 3), np.zeros(0, np.int64), 1.0
    v = dtype(voxel)
    f = (p - (p.min(0) - dtype(0.5) * v)) / v
    idx = np.floor(f).astype(np.int64)
    wall = float(np.minimum(f - np.floor(f), np.floor(f) + 1 - f).min())
    key = (idx[:, 2] << 42) | (idx[:, 1] << 21) | idx[:, 0]
    uniq, inv = np.unique(key, return_inverse=True)
    out = np.zeros((len(uniq), 3), dtype)
    cnt = np.zeros(len(uniq), np.int64)
    for i in range(len(p)):                                  # input order: the float32 form adds as the kernel does
        out[inv[i]] = out[inv[i]] + p[i]
        cnt[inv[i]] += 1
    inv_cnt = (1.0 / cnt.astype(np.float64)).astype(dtype)
    return out * inv_cnt[:, None], inv, wall


def multi_scale(src, tgt, init, cfgs, r, dtype=np.float64, trace=None):
    T = np.array(init, dtype)
    walls = []
    for cfg in cfgs:
        s, _, ws = voxel_down_sample(src, cfg["voxel_size"], dtype)
        t, _, wt = voxel_down_sample(tgt, cfg["voxel_size"], dtype)
        walls += [ws, wt]
        tr = [] if trace is not None else None
        T = icp(s, t, T, r, cfg["max_iteration"], cfg.get("rel", 1e-6), cfg.get("rel", 1e-6), dtype, tr)["transform"]
        if trace is not None:
            trace.append(dict(src=s, tgt=t, T=T.copy(), evals=tr))
    return T, min(walls)


# ------------------------------------------------------------------------------------------------ scenes
def rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def pose(axis, deg, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rot(axis, deg), t
    return T


# name, kind, pairs [(n_src, n_tgt)], r, iterations, options.  kind "fixed": relative_* = 0 and exactly `iterations` fits; "converge":
# relative_* = 1e-6, at most `iterations`; "scales": a two-scale multi_scale_icp
SCENES = [
    ("rigid_copy", "fixed", [(500, 500)], 0.15, 8, dict(noise=0.0)),
    ("partial_overlap", "fixed", [(600, 700)], 0.12, 8, dict(noise=0.002, crop=0.7)),
    ("outlier_shell", "fixed", [(560, 640)], 0.12, 8, dict(noise=0.002, shell=60)),
    ("two_pairs", "fixed", [(257, 300), (600, 449)], 0.15, 6, dict(noise=0.003)),
    ("noisy", "fixed", [(400, 650)], 0.2, 10, dict(noise=0.01)),
    ("tight_threshold", "fixed", [(450, 450)], 0.05, 6, dict(noise=0.004)),
    ("big_turn", "fixed", [(600, 600)], 0.25, 12, dict(noise=0.0, deg=6.0, shift=0.04)),
    ("converge_clean", "converge", [(400, 400)], 0.15, 30, dict(noise=0.0)),
    ("converge_noisy", "converge", [(500, 600)], 0.15, 30, dict(noise=0.004)),
    ("two_scales", "scales", [(600, 700)], 0.15, 0, dict(noise=0.002, voxels=(0.16, 0.09), its=(6, 6))),
]
REL = 1e-6


def make_scene(spec, seed):
    name, kind, pairs, r, its, o = spec
    rng = np.random.default_rng(seed)
    src, tgt, so, to, init, gt = [], [], [0], [0], [], []
    for ns, nt in pairs:
        base = rng.uniform(0.0, 1.0, (max(ns, nt) + 200, 3))
        G = pose(rng.normal(size=3), rng.uniform(10, 40), rng.uniform(-0.5, 0.5, 3))
        shell = o.get("shell", 0)
        if "crop" in o:                                      # two overlapping crops along x
            s = base[base[:, 0] < o["crop"]][:ns]
            t = base[base[:, 0] > 1 - o["crop"]][:nt]
        else:
            s, t = base[:ns - shell], base[:nt - shell] if o.get("noise", 0) == 0 and ns == nt else base[rng.permutation(len(base))[:nt - shell]]
        if shell:                                            # a shell of outliers far outside the threshold of every point of the other side
            d = rng.normal(size=(shell, 3))
            s = np.concatenate([s, 0.5 + 1.5 * d / np.linalg.norm(d, axis=1, keepdims=True)])
            d = rng.normal(size=(shell, 3))
            t = np.concatenate([t, 0.5 + 2.5 * d / np.linalg.norm(d, axis=1, keepdims=True)])
        t = t @ G[:3, :3].T + G[:3, 3] + rng.normal(size=t.shape) * o.get("noise", 0.0)
        D = pose(rng.normal(size=3), o.get("deg", 2.0), rng.normal(size=3) * o.get("shift", 0.015) / np.sqrt(3))
        src.append(s.astype(np.float32)), tgt.append(t.astype(np.float32))
        so.append(so[-1] + len(s)), to.append(to[-1] + len(t))
        init.append((D @ G).astype(np.float32)), gt.append(G)
    return dict(name=name, kind=kind, r=r, its=its, src=np.concatenate(src), tgt=np.concatenate(tgt), s_off=np.array(so, np.int32),
                t_off=np.array(to, np.int32), init=np.stack(init), gt=np.stack(gt), opts=o)


def run(sc, dtype, traces=None):
    """the statement on every pair of a scene -> per pair the result (and the trace)"""
    out = []
    for p in range(len(sc["s_off"]) - 1):
        s, t = sc["src"][sc["s_off"][p]:sc["s_off"][p + 1]], sc["tgt"][sc["t_off"][p]:sc["t_off"][p + 1]]
        tr = [] if traces is not None else None
        if sc["kind"] == "scales":
            cfgs = [dict(voxel_size=v, max_iteration=i, rel=0.0) for v, i in zip(sc["opts"]["voxels"], sc["opts"]["its"])]
            T, wall = multi_scale(s, t, sc["init"][p], cfgs, sc["r"], dtype, tr)
            out.append(dict(transform=T, wall=wall))
        else:
            rel = REL if sc["kind"] == "converge" else 0.0
            out.append(icp(s, t, sc["init"][p], sc["r"], sc["its"], rel, rel, dtype, tr))
        if traces is not None:
            traces.append(tr)
    return out


def screen_evals(evals, r, converge):
    """margins over the evaluations of one float64 run: (least relative gap between a row's nearest and second-nearest d2 that is not an exact
    tie, least relative distance of a nearest d2 to r^2, and for a convergence run the |delta| nearest to the band (1e-7, 1e-5))"""
    gap, edge, band_ok = np.inf, np.inf, True
    r2 = r * r
    for k, e in enumerate(evals):
        d2 = e["d2"]
        if d2 is not None and d2.shape[1] >= 1:
            part = np.partition(d2, min(1, d2.shape[1] - 1), axis=1)
            near = part[:, 0]
            edge = min(edge, float(np.abs(near - r2).min() / r2))
            if d2.shape[1] >= 2:
                second = part[:, 1]
                live = near < r2 * (1 + GAP)
                g = (second - near)[live] / np.maximum(second[live], 1e-300)
                g = g[(second - near)[live] != 0]            # an exact tie goes to the lowest index on both sides
                if len(g):
                    gap = min(gap, float(g.min()))
        if converge and k > 0:
            for key in ("fitness", "rmse"):
                d = abs(float(evals[k - 1][key]) - float(e[key]))
                band_ok = band_ok and (d < CONV_LO or d > CONV_HI)
    return gap, edge, band_ok


def screens(sc):
    traces = []
    res = run(sc, np.float64, traces)
    gap, edge, ok, wall = np.inf, np.inf, True, 1.0
    for p, tr in enumerate(traces):
        groups = [s["evals"] for s in tr] if sc["kind"] == "scales" else [tr]
        for ev in groups:
            g, e, b = screen_evals(ev, sc["r"], sc["kind"] == "converge")
            gap, edge, ok = min(gap, g), min(edge, e), ok and b
        if sc["kind"] == "scales":
            wall = min(wall, res[p]["wall"])
    good = gap >= GAP and edge >= GAP and ok and wall >= GAP
    if sc["kind"] == "converge":                             # the scene is about stopping early
        good = good and all(r["iterations"] < sc["its"] for r in res)
    return dict(ok=bool(good), gap=gap, edge=edge, band=ok, wall=wall), res, traces
