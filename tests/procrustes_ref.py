"""Plain float64 reference of the Procrustes fit (csrc/procrustes.hip) and host mirrors of its selection rules, for
test_procrustes_paths_oracle.py (CPU) and test_procrustes_paths_gpu.py.

The fit is compared on the DEVICE's own selected set (read back through want_topk=True), so which tied entries a path chose cannot leak
into the arithmetic check; the selection check stands alone (expected_set).  reg_branch / launch_form decide nothing about pass or fail:
they are input conditions -- each case names the branch and form it was built for and the tests first assert that the mirror agrees."""
import collections

import numpy as np
import torch

PK_MAX = 4096          # largest K the entry accepts (DR_ENOSUP beyond)
CAND_MAX = 4096        # candidate list of procrustes_kernel<true>
REG_MAX = 65536        # largest register-resident tile (N M)
EPS = 1e-4             # oracle.diffreg_oracle.kabsch

Fit = collections.namedtuple("Fit", "R t cond S det_uv")


def fit64(conf_f32, src, tgt, idx):
    """float64 weighted Kabsch on the flat indices `idx` of conf_f32 [N,M] (src [N,3], tgt [M,3]): weights conf[idx] promoted to double,
    Sxy NOT rounded to fp32, numpy's SVD.  -> Fit(R [3,3], t [3], cond, singular values [3], det(U) det(V))"""
    conf = np.asarray(conf_f32, dtype=np.float32)
    M = conf.shape[1]
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    w = conf.reshape(-1)[idx].astype(np.float64)
    X = np.asarray(src, dtype=np.float64)[idx // M]
    Y = np.asarray(tgt, dtype=np.float64)[idx % M]
    wn = w / (np.abs(w).sum() + EPS)
    mx = (wn[:, None] * X).sum(0)
    my = (wn[:, None] * Y).sum(0)
    S = (Y - my).T @ (wn[:, None] * (X - mx))
    U, D, Vt = np.linalg.svd(S)
    dd = np.linalg.det(U) * np.linalg.det(Vt)
    R = U @ np.diag([1.0, 1.0, dd]) @ Vt
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = D[0] / D[2]
    return Fit(R, my - R @ mx, float(cond), D, float(dd))


def expected_set(conf, K):
    """flat indices (sorted ascending, int64 tensor) of the K largest values of conf (any shape), ties at the K-th value resolved to the lowest
    flat indices (include/diffreg_hip.h): a stable descending sort keeps index order among equals"""
    flat = torch.as_tensor(conf).reshape(-1)
    order = torch.sort(flat, stable=True, descending=True)[1]
    return order[:K].sort()[0]


def pair_k(N, M, rate, n_src=None, n_tgt=None):
    """K of one pair as the wrapper and the kernels compute it: float32 product truncated, clipped to N M and to PK_MAX.  n_src / n_tgt: the
    mask sums of the 4D variant (use_mask_len)"""
    longest = max(N, M) if n_src is None else max(n_src, n_tgt)
    k = int(float(torch.tensor(float(longest), dtype=torch.float32) * rate))
    return min(k, N * M, PK_MAX)


def reg_candidates(conf, K):
    """host mirror of level 1 of procrustes_kernel<true>: element e = 4 (1024 q + t) + c lives in thread t.  -> (L, ncand): the K-th largest
    per-thread maximum and how many entries reach it (needs 1 <= K <= 1024)"""
    flat = torch.as_tensor(conf).reshape(-1).float()
    thread = (torch.arange(flat.numel()) // 4) % 1024
    tmax = torch.full((1024,), -1.0).scatter_reduce(0, thread, flat, "amax")
    tmax = tmax[tmax >= 0]                                       # threads that own no element are not enumerated
    L = tmax.sort(descending=True)[0][K - 1]
    return float(L), int((flat >= L).sum())


def reg_branch(conf, K):
    """which selection branch procrustes_kernel<true> takes for this tile and this K: "all" (K >= N M), "k_gt_1024" (the per-thread maxima do not bound the K-th largest entry: K > 1024, or K beyond the
    (N M + 3) / 4 threads that own elements), "list" (at most CAND_MAX
    entries reach L, the K-th largest per-thread maximum) or "bisect" """
    NM = torch.as_tensor(conf).numel()
    assert 1 <= K <= min(NM, PK_MAX) and NM <= REG_MAX
    if K >= NM:
        return "all"
    if K > 1024 or K > (NM + 3) // 4:                             # (or more than the threads that own elements: the same arm of the kernel)
        return "k_gt_1024"
    return "list" if reg_candidates(conf, K)[1] <= CAND_MAX else "bisect"


def slice_len(P, NM):
    """proc_slice_len of procrustes.hip: elements per slice of a sliced (N M > 65536) tile"""
    S = min(max(512 // max(P, 1), 1), 256)
    SL = (NM + S - 1) // S
    SL = (SL + 1023) // 1024 * 1024
    return max(SL, 4096)


def launch_form(P, N, M):
    """dr_debug_procrustes_last_form of a launch: 0 the register kernel, 1 sliced with the take pass's keys in registers, 2 re-read"""
    if N * M <= REG_MAX:
        return 0
    return 1 if slice_len(P, N * M) <= 32768 else 2


def scalar_arm(P, N, M, base_ptr=0):
    """the causes that send pair b of a register-resident batch to the scalar load arm: {"nm"} (N M % 4 != 0), {"ptr"} (its conf pointer is not
    16-byte aligned), both, or empty"""
    out = []
    for b in range(P):
        c = set()
        if (N * M) % 4:
            c.add("nm")
        if (base_ptr + 4 * b * N * M) % 16:
            c.add("ptr")
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the selection cases: (N, M), kind, sample_rate -> a batch of three tiles (pair 1 is the flat one, so a neighbour's fallback cannot disturb
# pairs 0 and 2) with the branch each pair was built for
# ---------------------------------------------------------------------------------------------------------------------------------------
KINDS = ("distinct", "quantised", "flat", "sparse", "sharp_on_quantised")


def tile(kind, N, M, K, seed):
    """one [N,M] float32 tile.  distinct: a random permutation of N M different values; quantised: 16 levels, the upper ones more frequent
    (floor(16 sqrt(u)) / 16: the top level fills 12 % of the tile, which overflows the candidate list from 34 k entries on); flat: one value;
    sparse: K // 2 non-zero entries (at least one), so the K-th value is +0.0; sharp_on_quantised: K large distinct entries packed into the
    elements of consecutive threads (16 per thread on a 128 x 128 tile) over 4 levels below 0.1 whose top level fills 44 % of the tile"""
    g = torch.Generator().manual_seed(seed)
    NM = N * M
    if kind == "distinct":
        v = (torch.randperm(NM, generator=g).float() + 1.0) / float(NM)      # exact in float32 below 2^24 entries
    elif kind == "quantised":
        v = (torch.rand(NM, generator=g).sqrt() * 16).floor().clamp_(max=15) / 16
    elif kind == "flat":
        v = torch.full((NM,), 1.0 / (M + seed % 7))
    elif kind == "sparse":
        v = torch.zeros(NM)
        n = max(1, K // 2)
        v[torch.randperm(NM, generator=g)[:n]] = 0.5 + (torch.randperm(n, generator=g).float() + 1.0) / (2.0 * n + 2.0)
    elif kind == "sharp_on_quantised":
        v = (torch.rand(NM, generator=g).sqrt() * 4).floor().clamp_(max=3) / 40
        e = torch.arange(NM)
        order = torch.argsort(((e // 4) % 1024) * 64 + (e // 4096) * 4 + e % 4)          # thread-major: thread 0's elements first
        own = order[:K]
        v[own] = 0.5 + (torch.randperm(K, generator=g).float() + 1.0) / (2.0 * K + 2.0)
    else:
        raise KeyError(kind)
    return v.reshape(N, M)


SELECTION_CASES = [
    # (N, M), kind, rate, branch of pairs 0 and 2 (None: a sliced tile), branch of the flat pair 1
    ((5, 7), "distinct", 0.7, "list", "list"),
    ((5, 7), "quantised", 1.0, "list", "list"),
    ((5, 7), "flat", 0.3, "list", "list"),
    ((5, 7), "distinct", 20.0, "all", "all"),                     # K = 140 clipped to N M = 35
    ((3, 100), "distinct", 1.0, "k_gt_1024", "k_gt_1024"),      # K = 100 <= 1024 but only 75 threads own elements
    ((3, 100), "quantised", 1.0, "k_gt_1024", "k_gt_1024"),
    ((64, 64), "distinct", 1.0, "list", "list"),
    ((64, 64), "quantised", 0.7, "list", "list"),
    ((64, 64), "flat", 0.3, "list", "list"),                      # 4096 tied candidates: list entries beyond the first 1024
    ((64, 64), "sparse", 1.0, "list", "list"),
    ((64, 64), "distinct", 20.0, "k_gt_1024", "k_gt_1024"),
    ((64, 64), "flat", 20.0, "k_gt_1024", "k_gt_1024"),
    ((64, 65), "distinct", 1.0, "list", "bisect"),
    ((64, 65), "quantised", 1.0, "list", "bisect"),
    ((64, 65), "flat", 0.7, "bisect", "bisect"),
    ((64, 65), "sparse", 1.0, "bisect", "bisect"),
    ((64, 65), "sharp_on_quantised", 1.0, "list", "bisect"),
    ((64, 65), "distinct", 20.0, "k_gt_1024", "k_gt_1024"),
    ((127, 129), "distinct", 0.3, "list", "bisect"),
    ((127, 129), "quantised", 1.0, "list", "bisect"),
    ((127, 129), "flat", 1.0, "bisect", "bisect"),
    ((127, 129), "sparse", 0.7, "bisect", "bisect"),
    ((127, 129), "sharp_on_quantised", 1.0, "bisect", "bisect"),
    ((127, 129), "quantised", 20.0, "k_gt_1024", "k_gt_1024"),
    ((128, 128), "distinct", 1.0, "list", "bisect"),
    ((128, 128), "quantised", 0.7, "list", "bisect"),
    ((128, 128), "flat", 1.0, "bisect", "bisect"),
    ((128, 128), "sparse", 1.0, "bisect", "bisect"),
    ((128, 128), "sharp_on_quantised", 1.0, "bisect", "bisect"),
    ((128, 128), "distinct", 20.0, "k_gt_1024", "k_gt_1024"),
    ((128, 128), "flat", 20.0, "k_gt_1024", "k_gt_1024"),
    ((128, 128), "sparse", 20.0, "k_gt_1024", "k_gt_1024"),
    ((128, 128), "sharp_on_quantised", 20.0, "k_gt_1024", "k_gt_1024"),
    ((255, 257), "distinct", 1.0, "list", "bisect"),
    ((255, 257), "quantised", 1.0, "bisect", "bisect"),
    ((255, 257), "flat", 0.3, "bisect", "bisect"),
    ((255, 257), "sparse", 1.0, "bisect", "bisect"),
    ((255, 257), "sharp_on_quantised", 0.7, "bisect", "bisect"),
    ((256, 256), "distinct", 1.0, "list", "bisect"),
    ((256, 256), "quantised", 1.0, "bisect", "bisect"),
    ((256, 256), "flat", 1.0, "bisect", "bisect"),
    ((256, 256), "sparse", 0.3, "bisect", "bisect"),
    ((256, 256), "sharp_on_quantised", 1.0, "bisect", "bisect"),
    ((256, 257), "distinct", 1.0, None, None),
    ((256, 257), "quantised", 1.0, None, None),
    ((256, 257), "flat", 1.0, None, None),
    ((256, 257), "sparse", 1.0, None, None),
    ((256, 257), "sharp_on_quantised", 1.0, None, None),
    ((2, 2048), "distinct", 0.7, "k_gt_1024", "k_gt_1024"),
    ((2, 2048), "quantised", 1.0, "k_gt_1024", "k_gt_1024"),
    ((1, 4096), "distinct", 0.3, "k_gt_1024", "k_gt_1024"),
    ((1, 4096), "quantised", 1.0, "all", "all"),                  # K = 4096 = N M = PK_MAX
]


def case_id(case):
    (N, M), kind, rate = case[:3]
    return "%dx%d-%s-%g" % (N, M, kind, rate)


def selection_batch(case):
    """-> conf [3,N,M] float32, src [3,N,3], tgt [3,M,3] (CPU) of a selection case"""
    (N, M), kind, rate = case[:3]
    K = pair_k(N, M, rate)
    seed = 1000 * N + M + int(rate * 10) + 17 * KINDS.index(kind)
    conf = torch.stack([tile(kind, N, M, K, seed), tile("flat", N, M, K, seed + 1), tile(kind, N, M, K, seed + 2)])
    g = torch.Generator().manual_seed(seed + 3)
    return conf, torch.rand(3, N, 3, generator=g), torch.rand(3, M, 3, generator=g)


def rank_deficient_by_construction(idx, conf, M):
    """fewer than four different source rows or target columns among the selected entries that carry weight: the centred clouds span at
    most a plane, so Sxy has rank <= 2 and R is not unique"""
    idx = torch.as_tensor(idx).long().reshape(-1)
    idx = idx[torch.as_tensor(conf).reshape(-1)[idx] != 0]
    return (idx // M).unique().numel() < 4 or (idx % M).unique().numel() < 4


# ---------------------------------------------------------------------------------------------------------------------------------------
# constructed geometries: conf carries a permutation matching of K entries with chosen weights over a background of 1e-12
# ---------------------------------------------------------------------------------------------------------------------------------------
BACKGROUND = 1e-12
GEOM_TILES = ((64, 64), (200, 190))
GEOM_RATE = 0.5                                                   # K = 32 and 100, exact in float32


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def matching_tile(N, M, src_pts, tgt_pts, w, seed):
    """-> conf [N,M], src [N,3], tgt [M,3] float32 and the flat indices of the matching: entry k couples a random row with a random column
    (no row or column twice), carries weight w[k] and the points src_pts[k], tgt_pts[k]; everything else is BACKGROUND and random points"""
    K = len(w)
    g = torch.Generator().manual_seed(seed)
    rows, cols = torch.randperm(N, generator=g)[:K], torch.randperm(M, generator=g)[:K]
    conf = torch.full((N, M), BACKGROUND)
    conf[rows, cols] = torch.as_tensor(np.asarray(w), dtype=torch.float32)
    src, tgt = torch.rand(N, 3, generator=g), torch.rand(M, 3, generator=g)
    src[rows] = torch.as_tensor(np.asarray(src_pts), dtype=torch.float32)
    tgt[cols] = torch.as_tensor(np.asarray(tgt_pts), dtype=torch.float32)
    return conf, src, tgt, (rows * M + cols).sort()[0]


def cloud(K, seed, scale=(1.0, 1.0, 1.0), offset=0.0):
    rng = np.random.RandomState(seed)
    return rng.randn(K, 3) * np.asarray(scale) + offset


def six_points(K, stretch=1.0):
    """the points +-e_i (axis 0 stretched), each K // 6 times, the rest at the origin: mean 0 and a diagonal second moment exactly"""
    p = np.concatenate([np.eye(3), -np.eye(3)]) * np.array([stretch, 1.0, 1.0])
    return np.concatenate([np.tile(p, (K // 6, 1)), np.zeros((K % 6, 3))])


R_RANDOM = rotation([0.3, -0.5, 0.8], 1.234)
T0 = np.array([0.11, -0.07, 0.05])


def geometry_cases(K, seed):
    """name -> (src_pts [K,3], tgt_pts [K,3], weights [K], group).  Groups: "motion", "reflection", "equal_sv", "deficient", "near_coplanar",
    "far", "weights" """
    rng = np.random.RandomState(seed)
    w = 0.5 + 0.5 * rng.rand(K)
    ones = np.full(K, 0.75)
    out = {}
    X = cloud(K, seed + 1)
    for name, R0 in (("motion_1e-4rad", rotation([1, 2, 3], 1e-4)), ("motion_90deg", rotation([1, 2, 3], np.pi / 2)),
                     ("motion_180deg", rotation([1, 2, 3], np.pi)), ("motion_random", R_RANDOM)):
        out[name] = (X, X @ R0.T + T0, w, "motion")
    Xa = cloud(K, seed + 2, scale=(3.0, 2.0, 1.0))
    out["reflection"] = (Xa, (Xa * np.array([1.0, 1.0, -1.0])) @ R_RANDOM.T + T0, w, "reflection")
    X6 = six_points(K)
    out["equal_sv_axis"] = (X6, X6 @ rotation([0, 0, 1], np.pi / 2).T + T0, ones, "equal_sv")      # Sxy = c R0, a signed permutation: ga = 0
    out["equal_sv_random"] = (X6, X6 @ R_RANDOM.T + T0, ones, "equal_sv")
    X62 = six_points(K, stretch=2.0)
    out["two_equal_sv_axis"] = (X62, X62 @ rotation([0, 0, 1], np.pi / 2).T + T0, ones, "equal_sv")
    out["two_equal_sv_random"] = (X62, X62 @ R_RANDOM.T + T0, ones, "equal_sv")
    Xp = cloud(K, seed + 3, scale=(1.0, 1.0, 0.0))
    out["coplanar"] = (Xp, Xp @ R_RANDOM.T + T0, w, "deficient")
    s = rng.randn(K, 1)
    for name, d in (("collinear_x", [1.0, 0, 0]), ("collinear_y", [0, 1.0, 0]), ("collinear_oblique", [0.6, -0.48, 0.64])):
        Xl = s * np.asarray(d)
        out[name] = (Xl, Xl @ (np.eye(3) if name != "collinear_oblique" else R_RANDOM).T, w, "deficient")
    Xn = cloud(K, seed + 4, scale=(1.0, 1.0, 0.01))
    out["near_coplanar"] = (Xn, Xn @ R_RANDOM.T + T0, w, "near_coplanar")
    Xf = cloud(K, seed + 5, scale=(0.3, 0.3, 0.3), offset=1e3)
    out["far"] = (Xf, (Xf - 1e3) @ R_RANDOM.T + 1e3 + T0, w, "far")
    out["weights_1e-6_to_1"] = (X, X @ R_RANDOM.T + T0, 10.0 ** (-6.0 * np.arange(K) / (K - 1)), "weights")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# bars of the fit: the yardstick is the reference's own float32 arithmetic (oracle.diffreg_oracle.kabsch) on the same index set
# ---------------------------------------------------------------------------------------------------------------------------------------
def oracle_fit(conf, src, tgt, idx):
    """orc.kabsch on the entries idx of conf [N,M] -> R [3,3], t [3], cond (numpy float64 views of its float32 results)"""
    from oracle import diffreg_oracle as orc
    idx = torch.as_tensor(idx).long().reshape(-1)
    M = conf.shape[1]
    w = conf.reshape(-1)[idx].float()
    R, t, cond = orc.kabsch(src[idx // M][None].float(), tgt[idx % M][None].float(), w[None, :, None])
    return R[0].double().numpy(), t[0, :, 0].double().numpy(), float(cond[0])


def fit_bars(conf, src, tgt, idx):
    """-> (Fit in float64, e_ref of R, t, cond (relative), bars of R, t, cond): bar = max(4 e_ref, floor) with the floors of
    test_ops_gpu.py::test_procrustes (atol 1e-5, for t times the largest |coordinate|; rtol 1e-4 for cond)"""
    f = fit64(conf.numpy(), src.numpy(), tgt.numpy(), np.asarray(idx))
    Ro, to, co = oracle_fit(conf, src, tgt, idx)
    eR, et = np.abs(Ro - f.R).max(), np.abs(to - f.t).max()
    ec = abs(co / f.cond - 1.0) if np.isfinite(f.cond) and f.cond > 0 and np.isfinite(co) else float("inf")
    sel = torch.as_tensor(idx).long().reshape(-1)
    M = conf.shape[1]
    big = max(1.0, float(src[sel // M].abs().max()), float(tgt[sel % M].abs().max()))
    return f, (eR, et, ec), (max(4 * eR, 1e-5), max(4 * et, 1e-5 * big), max(4 * ec, 1e-4))
