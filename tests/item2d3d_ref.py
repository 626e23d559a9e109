"""The 2D-3D dataset item's pixel-point ground truth: the deterministic cases and a float64 numpy statement of the definition
(include/diffreg_hip.h, thirteenth set) -- brute force over the P x N distance matrix, no KD-tree.  Shared by tools/golden/make_golden_item2d3d.py
(which runs the reference's own functions on these cases), tests/test_item2d3d_cpu.py and tests/test_item2d3d_gpu.py.

A case: depth [H, W] float32 in raw units (millimetres, whole numbers; about 10 % zeros, a depth step down the middle, a few values beyond the
depth limit and a few very near ones), intrinsics K with a principal point off the pixel centres, a rigid transform T, and a cloud whose points
are image points pulled back through T with noise of the order of radius_3d, mixed with the edge populations: points nearer to the camera than
radius_3d (the whole-image window), points behind the camera, points projecting outside the image, points off every border and corner (clipped
windows), and pairs of points a hair apart (they share a nearest pixel)."""
import numpy as np

SCALING = 1000.0
LIMIT = 6.0
REL = 1e-9          # the screening margin: every decision the definition makes is this far (relative) from its threshold

# (H, W, N, points dtype, kind, radius_2d, radius_3d).  N: 1, 63, 64, 65, 300 and 513 = one LDS stage of the reverse check + 1.  W = 67 is no
# multiple of 4, 16 or 64; 24 x 40 spans 2 x 3 image tiles, 7 x 5 less than one.
CASES = [
    (24, 40, 300, "f4", "mixed", 8.0, 0.12),
    (24, 40, 513, "f8", "mixed", 2.5, 0.12),
    (24, 40, 65, "f4", "mixed", 2.5, 0.20),
    (7, 5, 64, "f8", "mixed", 1.5, 0.15),
    (7, 5, 63, "f4", "mixed", 8.0, 0.15),
    (7, 5, 1, "f4", "one", 8.0, 0.30),
    (1, 67, 65, "f4", "mixed", 3.5, 0.10),
    (1, 67, 300, "f8", "mixed", 8.0, 0.10),
    (24, 40, 64, "f4", "far", 8.0, 0.05),        # every point farther than radius_3d from every pixel: a result of length 0
    (7, 5, 63, "f8", "blank", 8.0, 0.15),        # all depth zero: no image point at all
    (24, 40, 300, "f4", "near", 8.0, 0.12),      # a quarter of the cloud within radius_3d of the camera plane or behind it
]


def intrinsics(H, W):
    f = 0.75 * max(H, W)
    return np.array([[f, 0.0, (W - 1) / 2.0 + 0.13], [0.0, 1.1 * f, (H - 1) / 2.0 + 0.21], [0.0, 0.0, 1.0]])


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rigid(rng, angle=0.4, shift=0.5):
    T = np.eye(4)
    T[:3, :3] = rodrigues(rng.randn(3), angle * rng.rand())
    T[:3, 3] = shift * rng.randn(3)
    return T


def make_depth(rng, H, W, kind):
    if kind == "blank":
        return np.zeros((H, W), np.float32)
    col = np.arange(W)[None, :]
    row = np.arange(H)[:, None]
    d = 1500.0 + 6.0 * col + 9.0 * row + np.where(col >= W // 2, 600.0, 0.0) + rng.randint(-40, 41, size=(H, W))
    u = rng.rand(H, W)
    d = np.where(u < 0.10, 0.0, d)                       # holes
    d = np.where((u >= 0.10) & (u < 0.14), 7000.0 + rng.randint(0, 500, size=(H, W)), d)      # beyond the limit
    d = np.where((u >= 0.14) & (u < 0.18), rng.randint(30, 120, size=(H, W)), d)              # a few centimetres from the camera
    return np.round(d).astype(np.float32)


def image_points(depth, K, scaling=SCALING, limit=LIMIT):
    """back_project(return_pixels=True): -> (points [P, 3] float64, pixels [P, 2] int64 (h, w)), row-major over the pixels with z > 0;
    v = flat / W keeps its fraction"""
    H, W = depth.shape
    flat = np.arange(H * W)
    z = depth.reshape(-1).astype(np.float64) / scaling
    if limit is not None:
        z = np.where(z > limit, 0.0, z)
    x = ((flat % W) - K[0, 2]) * z / K[0, 0]
    y = ((flat / W) - K[1, 2]) * z / K[1, 1]
    keep = z > 0
    return np.stack([x, y, z], 1)[keep], np.stack([flat // W, flat % W], 1)[keep].astype(np.int64)


def make_case(k, seed):
    H, W, N, dt, kind, r2d, r3d = CASES[k]
    rng = np.random.RandomState(seed)
    K = intrinsics(H, W)
    depth = make_depth(rng, H, W, kind)
    T = rigid(rng)
    shown = make_depth(rng, H, W, "mixed") if kind == "blank" else depth
    ip, px = image_points(shown, K)
    base = ip[rng.randint(0, len(ip), size=N)] + (0.6 * r3d) * rng.randn(N, 3)
    if kind == "far":
        base[:, 2] += 10 * r3d + rng.rand(N)
    if kind in ("mixed", "near") and N >= 63:
        n = N // (4 if kind == "near" else 12)
        base[0:n, 2] = (rng.rand(n) * 2 - 1) * r3d                               # |z| <= radius_3d: the whole-image window
        base[n:2 * n, 2] = -rng.rand(n) * 2.0 - r3d                              # behind the camera
        base[2 * n:3 * n, 0] += (3.0 + rng.rand(n)) * np.sign(rng.randn(n))      # projecting outside the image, left and right
        corners = np.array([[0, 0], [0, W - 1], [H - 1, 0], [H - 1, W - 1], [0, W // 2], [H - 1, W // 2], [H // 2, 0], [H // 2, W - 1]])
        zc = 1.6 + 0.3 * rng.rand(len(corners))
        off = np.array([[-1, -1], [-1, 1], [1, -1], [1, 1], [-1, .53], [1, .53], [.53, -1], [.53, 1]]) * 0.7      # 0.7 of a pixel off the border
        base[3 * n:3 * n + 8] = np.stack([(corners[:, 1] + off[:, 1] - K[0, 2]) * zc / K[0, 0],
                                          (corners[:, 0] + off[:, 0] - K[1, 2]) * zc / K[1, 1], zc], 1)
        base[3 * n + 8:3 * n + 12] = base[3 * n + 12:3 * n + 16] + 1e-3 * rng.randn(4, 3)                 # pairs a hair apart
    R, t = T[:3, :3], T[:3, 3]
    pts = (base - t) @ R                                                         # T^-1: the cloud in its own frame
    pts = pts.astype(np.float32 if dt == "f4" else np.float64)
    return dict(depth=depth, points=pts, K=K, T=T, r2d=float(r2d), r3d=float(r3d), limit=LIMIT)


def transformed(points, T):
    return points.astype(np.float64) @ T[:3, :3].T + T[:3, 3]


def render(q, K):
    """array_ops.render: truncation toward zero, (h, w)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        w = K[0, 0] * q[:, 0] / q[:, 2] + K[0, 2]
        h = K[1, 1] * q[:, 1] / q[:, 2] + K[1, 2]
    return np.stack([np.trunc(h), np.trunc(w)], 1), np.stack([h, w], 1)


def _tables(c):
    ip, px = image_points(c["depth"], c["K"], limit=c["limit"])
    q = transformed(c["points"], c["T"])
    d = ip[:, None, :] - q[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    rp, raw = render(q, c["K"])
    dp = px[:, None, :].astype(np.float64) - rp[None, :, :]
    s2 = dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1]
    return px, d2, s2, raw


def corr_mutual(c):
    """-> (img_corr_pixels [C, 2] int64, pcd_corr_indices [C] int64): the definition, ties to the lowest index (np.argmin takes the first)"""
    px, d2, s2, _ = _tables(c)
    P, N = d2.shape
    if P == 0 or N == 0:
        return np.zeros((0, 2), np.int64), np.zeros((0,), np.int64)
    nn_i = d2.argmin(1)
    nn_j = d2.argmin(0)
    i = np.arange(P)
    keep = (nn_j[nn_i] == i) & (np.sqrt(d2[i, nn_i]) < c["r3d"]) & (np.sqrt(s2[i, nn_i]) < c["r2d"])
    return px[keep], nn_i[keep].astype(np.int64)


def corr_radius(c):
    """-> the radius variant's pairs in ascending (i, j)"""
    px, d2, s2, _ = _tables(c)
    with np.errstate(invalid="ignore"):
        i, j = np.nonzero((np.sqrt(d2) < c["r3d"]) & (np.sqrt(s2) < c["r2d"]))
    return px[i].reshape(-1, 2), j.astype(np.int64)


def overlap(c):
    """-> (img_overlap_indices, pcd_overlap_indices): np.unique of h W + w and of j over the radius pairs"""
    pix, idx = corr_radius(c)
    return np.unique(pix[:, 0] * c["depth"].shape[1] + pix[:, 1]), np.unique(idx)


def screen(c):
    """the screening rules, from the float64 tables alone -> None when the case passes, else the rule it breaks"""
    px, d2, s2, raw = _tables(c)
    P, N = d2.shape
    if P and N:
        for axis, n in ((1, N), (0, P)):
            if n >= 2:
                two = np.partition(d2, 1, axis=axis)
                a, b = np.take(two, 0, axis=axis), np.take(two, 1, axis=axis)
                if not np.all(b - a >= REL * b):
                    return "nearest / second-nearest gap"
        if not np.all(np.abs(np.sqrt(d2) - c["r3d"]) >= REL * c["r3d"]):
            return "a distance at radius_3d"
        with np.errstate(invalid="ignore"):
            if np.any((s2 == c["r2d"] * c["r2d"]) & (np.sqrt(d2) < c["r3d"])):          # the 2D test is only asked of pairs inside radius_3d
                return "a 2D squared distance at radius_2d^2"
    fin = np.isfinite(raw)
    if not np.all(np.abs(raw[fin] - np.round(raw[fin])) >= REL * np.maximum(1.0, np.abs(raw[fin]))):
        return "a render argument at an integer"
    if not np.all(np.abs(raw[fin]) < 2.0 ** 30):
        return "a render argument beyond 2^30"
    return None


def draw_case(k):
    """the first seed from 3000 + 50 k whose case passes the screening -> (case, seed); cases that fail are drawn again, never skipped"""
    for seed in range(3000 + 50 * k, 3050 + 50 * k):
        c = make_case(k, seed)
        if screen(c) is None:
            return c, seed
    raise RuntimeError("case %d: no seed passes the screening" % k)


# ------------------------------------------------------------------------------------------------------------
# prepare_item: the body of SevenScenes2D3DHardPairDataset.__getitem__ behind its file reads (sevenscenes_hard.py:128-206), float64 numpy
# ------------------------------------------------------------------------------------------------------------
# (H, W, cloud size, options)
ITEMS = [
    (24, 40, 400, dict(max_points=300, use_augmentation=True, augmentation_noise=0.005, return_corr_indices=True,
                       matching_method="mutual_nearest", matching_radius_2d=8.0, matching_radius_3d=0.12, return_overlap_indices=True)),
    (7, 5, 63, dict(max_points=None, use_augmentation=False, augmentation_noise=0.005, return_corr_indices=True,
                    matching_method="radius", matching_radius_2d=1.5, matching_radius_3d=0.15, return_overlap_indices=False)),
    (24, 40, 200, dict(max_points=500, use_augmentation=True, augmentation_noise=0.01, return_corr_indices=False,
                       matching_method="mutual_nearest", matching_radius_2d=2.5, matching_radius_3d=0.12, return_overlap_indices=True)),
]


def make_item(k, seed):
    """-> (raw, options, draws): raw as the dataset holds it after its file reads; the draws np.random would make, fixed"""
    H, W, N, opt = ITEMS[k]
    rng = np.random.RandomState(seed)
    K = intrinsics(H, W)
    depth = make_depth(rng, H, W, "mixed").astype(np.float64)
    T = rigid(rng)
    ip, _ = image_points(depth.astype(np.float32), K)
    base = ip[rng.randint(0, len(ip), size=N)] + (0.6 * opt["matching_radius_3d"]) * rng.randn(N, 3)
    pts = ((base - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    ori = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    raw = dict(depth=depth, image=ori.astype(np.float64) / 255.0, image_gray=(ori.astype(np.float64) @ np.array([0.2125, 0.7154, 0.0721])) / 255.0,
               ori_image=ori, points=pts, intrinsics=K, cloud_to_image=T, scene_name="scene", image_file="scene/seq-01/color_000003.png",
               depth_file="scene/seq-01/depth_000003.png", cloud_file="scene/seq-01/cloud_bin_0.npy", overlap=0.5, image_id="01-000003",
               cloud_id="01-0")
    draws = {}
    n = N
    if opt["max_points"] is not None and N > opt["max_points"]:
        draws["sel_indices"] = rng.permutation(N)[:opt["max_points"]].astype(np.int64)
        n = opt["max_points"]
    if opt["use_augmentation"]:
        A = np.eye(4)
        A[:3, :3] = rodrigues(rng.randn(3), rng.rand() * 0.1 * np.pi / np.sqrt(3.0))
        A[:3, 3] = rng.randn(3) * 0.1 / np.sqrt(3.0)
        draws["aug_transform"] = A
        draws["noise"] = rng.rand(n, 3)
    return raw, opt, draws


def item_statement(raw, opt, draws):
    """the item in float64 numpy (the reference's order of operations), correspondences by the brute-force statement above"""
    out = {}
    depth, image = raw["depth"].astype(np.float64), raw["image"].copy()
    K, T = raw["intrinsics"].astype(np.float64), raw["cloud_to_image"].astype(np.float64)
    pts = raw["points"]
    if "sel_indices" in draws:
        pts = pts[draws["sel_indices"]]
    if opt["use_augmentation"]:
        center = pts.mean(axis=0)
        sub, add = np.eye(4), np.eye(4)
        sub[:3, 3], add[:3, 3] = -center, center
        A = add @ (draws["aug_transform"] @ sub)
        pts = pts @ A[:3, :3].T + A[:3, 3]
        inv = np.eye(4)
        inv[:3, :3] = A[:3, :3].T
        inv[:3, 3] = -(A[:3, :3].T @ A[:3, 3])
        T = T @ inv
        pts = pts + (draws["noise"] - 0.5) * opt["augmentation_noise"]
    image = image - image.mean()
    W = image.shape[1]
    c = dict(depth=depth.astype(np.float32), points=pts, K=K, T=T, r2d=opt["matching_radius_2d"], r3d=opt["matching_radius_3d"], limit=LIMIT)
    if opt["return_corr_indices"]:
        pix, idx = corr_mutual(c) if opt["matching_method"] == "mutual_nearest" else corr_radius(c)
        out["img_corr_pixels"], out["img_corr_indices"], out["pcd_corr_indices"] = pix, pix[:, 0] * W + pix[:, 1], idx
    if opt["return_overlap_indices"]:
        io, po = overlap(c)
        out["img_overlap_pixels"], out["img_overlap_indices"], out["pcd_overlap_indices"] = np.stack([io // W, io % W], 1), io, po
    out.update(intrinsics=K.astype(np.float32), transform=T.astype(np.float32), image=image.astype(np.float32), depth=depth.astype(np.float32),
               image_gray=raw["image_gray"].astype(np.float32), ori_image=raw["ori_image"].astype(np.float32), points=pts.astype(np.float32),
               feats=np.ones((pts.shape[0], 1), np.float32))
    out["_case"] = c
    return out


def draw_item(k):
    for seed in range(5000 + 50 * k, 5050 + 50 * k):
        raw, opt, draws = make_item(k, seed)
        if screen(item_statement(raw, opt, draws)["_case"]) is None:
            return raw, opt, draws, seed
    raise RuntimeError("item %d: no seed passes the screening" % k)


INT_KEYS = ("img_corr_pixels", "img_corr_indices", "pcd_corr_indices", "img_overlap_pixels", "img_overlap_indices", "pcd_overlap_indices")
