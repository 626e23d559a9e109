"""Deterministic inputs and a numpy restatement of the geometry head of MATR2D3D.forward (EXP/model.py:302-351): vision3d.ops.back_project,
MATR2D3D.back_project_depth, vision3d.ops.render (rounding=False) and create_meshgrid.  The restatement takes the dtype, so the float64 and
the float32 run of the reference are both reproduced (tests/test_front2d3d_oracle.py pins it to tests/golden/front2d3d.npz).

Fixture rules (asserted by `fixture_rules`, on the CPU): every z of a back-projection case is at least MARGIN away from 0 and from the depth
limit, and every z render clamps or keeps is at least a factor 2 away from eps -- so no mask entry and no clamp is undecided between float32
and float64."""
import numpy as np

DEPTH_LIMIT = 6.0
MARGIN = 1e-3
EPS = 1e-8

# name -> (H, W, mode, seed).  1 x 1; 5 x 7 (fewer pixels than a wave, not a multiple of the 4-pixel vector); 33 x 65 (2 145 pixels: more than
# one workgroup of 256 x 4, odd, not a multiple of the wave nor of the vector)
BACK_PROJECT_CASES = {"bp%d_%dx%d" % (mode, H, W): dict(H=H, W=W, mode=mode, seed=11 + 7 * mode + H)
                      for mode in (0, 1) for (H, W) in ((1, 1), (5, 7), (33, 65))}
# name -> (N, extrinsics kind, seed): "none", "full" (a general rotation; z < 0 only: the other two clamp cases cannot be placed exactly behind
# a general rotation), "axis" (a rotation about z with t_z = 0.5: z = 0 after the transform is exact in either precision)
RENDER_CASES = {"rd_%s_%d" % (ext, N): dict(N=N, ext=ext, seed=5 + N) for N in (1, 65, 257) for ext in ("none", "full")}
RENDER_CASES["rd_axis_65"] = dict(N=65, ext="axis", seed=99)
MESHGRID_SIZES = ((3, 5), (34, 45))


def intrinsics(H, W):
    return np.array([[525.3, 0.0, (W - 1) / 2 + 0.25], [0.0, 531.7, (H - 1) / 2 - 0.125], [0.0, 0.0, 1.0]], dtype=np.float32)


def make_back_project(H, W, mode, seed):
    """-> dict(depth [1,H,W] float32, intrinsics [1,3,3] float32, a, b (float32 scalars), z64 (the float64 z the case was built from))"""
    rng = np.random.default_rng(seed)
    n = H * W
    z = rng.uniform(0.3, 5.5, n)
    if n >= 35:
        z[rng.choice(n, n // 7, replace=False)] = rng.uniform(6.5, 9.0, n // 7)        # above the limit
        kinds = rng.permutation(n)
        z[kinds[: n // 9]] = 0.0                                                          # no depth (mode 1: handled below)
        z[kinds[n // 9: n // 9 + n // 11]] = -rng.uniform(0.2, 3.0, n // 11)              # negative
    if mode == 0:
        a, b = np.float32(1000.0), np.float32(0.0)
        depth = np.round(z * 1000.0).astype(np.float32)                                   # millimetres, as the sensor's uint16
    else:
        a, b = np.float32(73.5), np.float32(0.25)                                         # depth_coffa, depth_coffb; b != 0
        depth = ((z - float(b)) / float(a)).astype(np.float32)
        depth[z == 0.0] = 0.0                                                             # a depth of zero is z = b here
    return dict(depth=depth.reshape(1, H, W), intrinsics=intrinsics(H, W)[None], a=a, b=b)


def z_of(case, mode, dt=np.float64):
    d = case["depth"].astype(dt)
    return d / dt(1000.0) if mode == 0 else d * case["a"].astype(dt) + case["b"].astype(dt)


def make_render(N, ext, seed):
    """-> dict(points [N,3], intrinsics [3,3], extrinsics [4,4] or None), float32"""
    rng = np.random.default_rng(seed)
    q = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.2, 1.2, N), rng.uniform(0.5, 4.0, N)], 1)      # in the camera frame
    K = intrinsics(480, 640)
    if N >= 65:
        q[3::16, 2] = -rng.uniform(0.2, 2.0, q[3::16].shape[0])                          # behind the camera
    if ext == "none":
        if N >= 65:
            q[5::16, 2] = 0.0
            q[7::16, 2] = 5e-9                                                            # 0 < z < eps
        return dict(points=q.astype(np.float32), intrinsics=K, extrinsics=None)
    T = np.eye(4)
    if ext == "axis":
        c, s = np.cos(0.7), np.sin(0.7)
        T[:3, :3] = [[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]
        T[:3, 3] = [0.125, -0.25, 0.5]
        q[5::16, 2] = 0.0
        T = T.astype(np.float32)
        p = (q - T[:3, 3].astype(np.float64)) @ T[:3, :3].astype(np.float64)              # R^T (q - t)
        p = p.astype(np.float32)
        p[5::16, 2] = -T[2, 3]                                                            # z * 1 + t_z == 0 exactly
        return dict(points=p, intrinsics=K, extrinsics=T)
    A = rng.normal(size=(3, 3))
    Q, _ = np.linalg.qr(A)
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    T[:3, :3], T[:3, 3] = Q, rng.uniform(-0.5, 0.5, 3)
    p = (q - T[:3, 3]) @ T[:3, :3]
    return dict(points=p.astype(np.float32), intrinsics=K, extrinsics=T.astype(np.float32))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def back_project(depth, K, mode, a, b, depth_limit, dt):
    """depth [H,W] -> points [H*W,3] (dt), mask [H*W] bool: ops/back_project.py:29-53 (mode 0), EXP/model.py:875-899 (mode 1), transposed=True"""
    H, W = depth.shape
    d, K = depth.astype(dt), K.astype(dt)
    idx = np.arange(H * W).reshape(H, W)
    u, v = (idx % W).astype(dt), (idx // W).astype(dt)
    z = d / dt(a) if mode == 0 else d * dt(a) + dt(b)
    if depth_limit is not None:
        z = np.where(z > dt(depth_limit), dt(0.0), z)
    x = (u - K[0, 2]) * z / K[0, 0]
    y = (v - K[1, 2]) * z / K[1, 1]
    return np.stack([x, y, z], -1).reshape(-1, 3), (z > 0).reshape(-1)


def render(points, K, T, dt, eps=EPS):
    """points [N,3] -> pixels [N,2] (h, w) and depth [N]: ops/render.py:34-52 with rounding=False, ops/se3.py:49-52"""
    p, K = points.astype(dt), K.astype(dt)
    if T is not None:
        T = T.astype(dt)
        p = p @ T[:3, :3].T + T[None, :3, 3]
    zc = np.maximum(p[:, 2], dt(eps))
    w = K[0, 0] * p[:, 0] / zc + K[0, 2]
    h = K[1, 1] * p[:, 1] / zc + K[1, 2]
    return np.stack([h, w], -1), p[:, 2]


def create_meshgrid(height, width, normalized=False, flatten=False, centering=False):
    """ops/meshgrid.py:18-37: cartesian_prod of the row and column values.  Values only (int64 when neither flag is set); the normalised,
    uncentred values are torch.linspace's and are taken from torch in the GPU test -- create_meshgrid calls .cuda() and cannot be minted offline"""
    if normalized and not centering:
        raise NotImplementedError("torch.linspace values: see the GPU test")
    h, w = np.arange(height), np.arange(width)
    if centering:
        h, w = h.astype(np.float32) + np.float32(0.5), w.astype(np.float32) + np.float32(0.5)
    if normalized:
        h, w = h.astype(np.float32) / np.float32(height), w.astype(np.float32) / np.float32(width)
    hh, ww = np.meshgrid(h, w, indexing="ij")
    out = np.stack([hh, ww], -1)
    return out.reshape(-1, 2) if flatten else out


def fixture_rules():
    """-> list of broken rules (empty: the fixture decides every mask entry and every clamp in both precisions)"""
    bad = []
    for name, kw in BACK_PROJECT_CASES.items():
        c = make_back_project(**kw)
        for dt in (np.float32, np.float64):
            z = z_of(c, kw["mode"], dt).astype(np.float64)
            if np.min(np.abs(z)) < MARGIN and kw["mode"] == 1:
                bad.append((name, "z within the margin of 0"))
            if kw["mode"] == 0 and np.any((z != 0.0) & (np.abs(z) < MARGIN)):
                bad.append((name, "z within the margin of 0"))
            if np.min(np.abs(z - DEPTH_LIMIT)) < MARGIN:
                bad.append((name, "z within the margin of the limit"))
        if kw["H"] * kw["W"] >= 35:
            z = z_of(c, kw["mode"])
            if not (np.any(z > DEPTH_LIMIT) and np.any(z < 0) and np.any(c["depth"] == 0)):
                bad.append((name, "a kind of depth is missing"))
    for name, kw in RENDER_CASES.items():
        c = make_render(**kw)
        for dt in (np.float32, np.float64):
            z = render(c["points"], c["intrinsics"], c["extrinsics"], dt)[1].astype(np.float64)
            if np.any((z != 0.0) & (z > EPS / 2) & (z < 2 * EPS)):
                bad.append((name, "z undecided against eps"))
            if np.any((z != 0.0) & (np.abs(z) < 1e-9)):
                bad.append((name, "z undecided against 0"))
        z = render(c["points"], c["intrinsics"], c["extrinsics"], np.float64)[1]
        if kw["N"] >= 65 and not np.any(z < 0):
            bad.append((name, "no point behind the camera"))
        if kw["N"] >= 65 and kw["ext"] != "full" and not np.any(z == 0.0):
            bad.append((name, "no point at z = 0"))
        if kw["N"] >= 65 and kw["ext"] == "none" and not np.any((z > 0) & (z < EPS)):
            bad.append((name, "no point with 0 < z < eps"))
    return bad


def rel_dev(a, ref):
    """max over the elements of |a - ref| / max(1, |ref|): the measure both the reference's own float32 deviation and the device error take"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - ref) / np.maximum(1.0, np.abs(ref))))
