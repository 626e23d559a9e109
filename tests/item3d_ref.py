"""Float64 restatement of the 3D / 4D dataset item (3D/datasets/_3dmatch.py:55-135, 3D/datasets/_4dmatch.py:58-146, 3D/lib/benchmark_utils.py:
166-185), operation by operation in numpy, and the synthetic scenes of tests/golden/item3d.npz (minted by tools/golden/make_golden_item3d.py,
which runs the reference's own two __getitem__ bodies on files made from these scenes and records every draw).

`draws` is what the reference took from np.random, in its order: src_perm / tgt_perm (the whole permutation; absent when the cloud is not
subsampled), euler [3] = np.random.rand(3) * pi * 2 / rot_factor, coin (np.random.rand(1)[0]), src_jitter / tgt_jitter ([n, 3] in [0, 1)).

Screening of the pair list (GAPR of tests/partition2d3d_ref.py): a scene is kept only when no |T src_i - tgt_j| lies within GAPR of the radius, so
the float32 device predicate and the float64 reference agree on EVERY pair: the excluded share is 0.
"""
import numpy as np

from tests.partition2d3d_ref import GAPR

OVERLAP_RADIUS = 0.0375          # _3dmatch.py:38
NOISE_3D, NOISE_4D = 0.005, 0.002  # augment_noise of configs/train/3dmatch.yaml, 4dmatch.yaml

# (n_src, n_tgt, max_points, data_augmentation, source turned (None: no draw), trans as [3, 1])
CASES_3D = [
    (1, 3, 30000, True, True, False),
    (3, 1, 30000, True, False, True),
    (65, 300, 65, True, True, True),
    (300, 65, 100, True, False, False),
    (300, 300, 30000, False, None, False),
    (65, 65, 40, False, None, True),
]
# (n_src, n_tgt, max_points, data_augmentation, source turned, metric_index present, trans as [3, 1])
CASES_4D = [
    (65, 300, 30000, True, True, True, False),
    (300, 65, 30000, True, False, False, True),
    (3, 1, 30000, True, True, False, False),
    (300, 300, 100, False, None, True, False),      # the flow comes back unselected
    (1, 3, 30000, False, None, False, True),
]


def euler_zyx(angles):
    """Rotation.from_euler('zyx', angles).as_matrix(): extrinsic rotations about z, then y, then x -> Rx(c) Ry(b) Rz(a)"""
    a, b, c = (float(v) for v in angles)
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rz = np.array([[ca, -sa, 0.0], [sa, ca, 0.0], [0.0, 0.0, 1.0]])
    Ry = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, cc, -sc], [0.0, sc, cc]])
    return Rx @ Ry @ Rz


def scene(kind, k, seed):
    """raw arrays of case k as the dataset's files hold them: float32 clouds, float64 rot / trans; the target is the moved source plus a small
    displacement, so a good share of the rows has partners inside OVERLAP_RADIUS"""
    case = (CASES_3D if kind == "3dmatch" else CASES_4D)[k]
    ns, nt = case[0], case[1]
    rng = np.random.default_rng(seed)
    rot = euler_zyx(rng.random(3) * 2 * np.pi)
    trans = rng.normal(size=3) * 0.3
    trans = trans[:, None] if case[-1] else trans
    src = (rng.random((ns, 3)) * 0.3).astype(np.float32)
    flow = (rng.normal(size=(ns, 3)) * 0.01).astype(np.float32) if kind == "4dmatch" else np.zeros((ns, 3), np.float32)
    pick = rng.integers(0, ns, size=nt)
    tgt = ((src[pick].astype(np.float64) + flow[pick]) @ rot.T + trans.reshape(3) + rng.normal(size=(nt, 3)) * 0.02).astype(np.float32)
    raw = dict(src=src, tgt=tgt, rot=rot, trans=trans)
    if kind == "4dmatch":
        raw["flow"] = flow
        raw["correspondences"] = np.stack([pick[: min(ns, nt)], np.arange(min(ns, nt))], 1).astype(np.int64)
        if case[5]:
            raw["metric_index"] = rng.integers(0, ns, size=(1, 7)).astype(np.int64)
    return raw


def _subsample(cloud, perm, max_points):
    return cloud[perm[:max_points]] if cloud.shape[0] > max_points else cloud


def prepare(kind, raw, draws, max_points, data_augmentation, noise):
    """-> dict(src, tgt, rot, trans[, flow]) as the reference's __getitem__ leaves them BEFORE its final float32 casts (so a turned cloud is
    float64), with the same numpy operations on the same dtypes"""
    src, tgt = raw["src"].copy(), raw["tgt"].copy()
    rot, trans = raw["rot"], raw["trans"]
    flow = deformed = None
    if kind == "4dmatch":
        flow = raw["flow"]
        deformed = src + flow                                                # _4dmatch.py:77 (float32)
    src = _subsample(src, draws.get("src_perm"), max_points)
    tgt = _subsample(tgt, draws.get("tgt_perm"), max_points)
    if data_augmentation:
        rot_ab = euler_zyx(draws["euler"])
        if draws["coin"] > 0.5:
            src = np.matmul(rot_ab, src.T).T
            if deformed is not None:
                deformed = np.matmul(rot_ab, deformed.T).T
            rot = np.matmul(rot, rot_ab.T)
        else:
            tgt = np.matmul(rot_ab, tgt.T).T
            rot = np.matmul(rot_ab, rot)
            trans = np.matmul(rot_ab, trans)
        src += (draws["src_jitter"] - 0.5) * noise                           # in place: an unturned cloud stays float32
        tgt += (draws["tgt_jitter"] - 0.5) * noise
        if deformed is not None:
            flow = deformed - src
    out = dict(src=src, tgt=tgt, rot=rot, trans=trans if trans.ndim == 2 else trans[:, None])
    if flow is not None:
        out["flow"] = flow
    return out


def prepare_f64(kind, raw, draws, max_points, data_augmentation, noise):
    """the same item with every cloud promoted to float64 first: what the float32 in-place steps of the reference deviate from"""
    raw64 = dict(raw)
    for k in ("src", "tgt", "flow"):
        if k in raw:
            raw64[k] = raw[k].astype(np.float64)
    return prepare(kind, raw64, draws, max_points, data_augmentation, noise)


def distances(src, tgt, rot, trans):
    """|rot src_i + trans - tgt_j| in float64, [ns, nt]"""
    moved = src.astype(np.float64) @ np.asarray(rot, np.float64).T + np.asarray(trans, np.float64).reshape(1, 3)
    return np.sqrt(((moved[:, None, :] - tgt.astype(np.float64)[None, :, :]) ** 2).sum(-1))


def radius_pairs(src, tgt, rot, trans, radius):
    """KDTree_corr's predicate by brute force in float64 -> [C, 2] int64 in ascending (i, j)"""
    return np.argwhere(distances(src, tgt, rot, trans) < radius).astype(np.int64).reshape(-1, 2)


def near_radius(src, tgt, rot, trans, radius):
    """number of (i, j) whose distance lies within GAPR of the radius: 0 for every screened scene"""
    return int((np.abs(distances(src, tgt, rot, trans) - radius) <= GAPR).sum())


def bar(ref64, ref32):
    """the project's bar for a float32 result held to a float64 reference: max(one float32 ulp at the array's largest magnitude, 4 x the
    reference's own float32 deviation from its float64 statement)"""
    ref64 = np.asarray(ref64, np.float64)
    ulp = float(np.spacing(np.float32(np.abs(ref64).max() if ref64.size else 0.0)))
    dev = float(np.abs(np.asarray(ref32, np.float64) - ref64).max()) if ref64.size else 0.0
    return max(ulp, 4.0 * dev), dev
