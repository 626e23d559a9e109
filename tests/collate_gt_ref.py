"""The project's own numpy statement of the ground-truth collate entries (dr_blend_flow_knn3_f32, dr_coarse_gt_matches_f32) and of the 3D / 4D
neighbour calibration -- TEST INFRASTRUCTURE ONLY.  It restates 3D/datasets/utils.py:23-80 and dataloader.py:253-257, 512-520, 563-591 in float32
(`dtype=np.float32`, the device's arithmetic, operation by operation) or float64 (the exact statement the float32 deviation is measured from),
with the one rule the reference leaves open pinned: equal squared distances go to the lowest index.  It also carries the screening conditions
under which that rule, and the rounding of the reference's BLAS warp, cannot change a result.
"""
import numpy as np

F = np.float32


def d2_matrix(query, reference, dtype=F):
    """[nq, nr]: ((dx dx + dy dy) + dz dz) with d = reference - query"""
    q, r = np.asarray(query, dtype), np.asarray(reference, dtype)
    d = r[None, :, :] - q[:, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest(d2, k):
    """the k smallest per row in ascending order, equal values to the lowest index -> (idx [n, k], val [n, k])"""
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return idx, np.take_along_axis(d2, idx, axis=1)


def warp(src, rot, trn, flow=None, dtype=F):
    """p' = p + flow (4D), then ((r0 x + r1 y) + r2 z) + t per row"""
    p = np.asarray(src, dtype)
    if flow is not None:
        p = p + np.asarray(flow, dtype)
    R, t = np.asarray(rot, dtype).reshape(3, 3), np.asarray(trn, dtype).reshape(3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r] for r in range(3)], axis=1)


def blend_flow_knn3(query, reference, reference_flow, dtype=F):
    """blend_scene_flow(query, reference, reference_flow, knn=3); None when the pair has fewer than 4 references (the reference raises)"""
    if len(reference) < 4:
        return None
    idx, val = nearest(d2_matrix(query, reference, dtype), 3)
    dist = np.sqrt(val)
    dist[dist < 1e-10] = 1e-10
    w = dtype(1.0) / dist
    w = w / ((w[:, 0] + w[:, 1]) + w[:, 2])[:, None]
    f = np.asarray(reference_flow, dtype)[idx]                      # [nq, 3, 3]
    return (f[:, 0] * w[:, 0:1] + f[:, 1] * w[:, 1:2]) + f[:, 2] * w[:, 2:3]


def coarse_gt_matches(src, tgt, rot, trn, radius, flow=None, dtype=F):
    """-> int64 [2, C] (pair-local, ascending source), or None when a cloud has fewer than 2 points (the reference raises)"""
    if len(src) < 2 or len(tgt) < 2:
        return None
    w = warp(src, rot, trn, flow, dtype)
    d2 = d2_matrix(w, tgt, dtype)                                   # [ns, nt]; the reverse pass sees the same squares (a - b)^2 == (b - a)^2
    j, v = nearest(d2, 1)
    i_of_j, _ = nearest(np.ascontiguousarray(d2.T), 1)
    j, i_of_j = j[:, 0], i_of_j[:, 0]
    src_idx = np.arange(len(src))
    keep = (i_of_j[j] == src_idx) & (np.sqrt(v[:, 0]) < dtype(radius))
    return np.stack([src_idx[keep], j[keep]]).astype(np.int64)


# ----------------------------------------------------------------------------------------------------------------
# the screening conditions of the fixtures: conditions on the INPUTS, stated in float64
# ----------------------------------------------------------------------------------------------------------------
GAP, RADIUS_GAP = 1e-4, 1e-4


def _gap_rows(d2, k):
    """per row: the relative gaps between its k + 1 smallest values exceed GAP (neighbours 1 .. k + 1)"""
    s = np.sort(d2, axis=1)[:, :k + 1]
    a, b = s[:, :-1], s[:, 1:]
    return np.all(b - a > GAP * np.maximum(b, 1e-300), axis=1)


def _gaps_ok(d2, k):
    return bool(np.all(_gap_rows(d2, k)))


def screen_matches(src, tgt, rot, trn, radius, flow=None):
    """nearest and second-nearest d^2 of every point (both directions) differ by more than GAP relatively, and no nearest distance lies within
    RADIUS_GAP * radius of the radius"""
    d2 = d2_matrix(warp(src, rot, trn, flow, np.float64), tgt, np.float64)
    near = np.sqrt(d2.min(1))
    return _gaps_ok(d2, 1) and _gaps_ok(d2.T, 1) and bool(np.all(np.abs(near - radius) > RADIUS_GAP * radius))


def screen_blend_rows(query, reference):
    """the queries (a bool per row) whose four nearest references are separated by more than GAP relatively"""
    return _gap_rows(d2_matrix(query, reference, np.float64), 3)


def screen_blend(query, reference):
    """the four nearest references of every query are separated by more than GAP relatively"""
    return _gaps_ok(d2_matrix(query, reference, np.float64), 3)


# ----------------------------------------------------------------------------------------------------------------
# calibrate_neighbors (dataloader.py:563-591) over neighbour COUNTS
# ----------------------------------------------------------------------------------------------------------------
def hist_bins(deform_radius):
    return int(np.ceil(4 / 3 * np.pi * (deform_radius + 1) ** 3))


def calibrate_from_counts(per_sample_counts, num_layers, hist_n, keep_ratio=0.8, samples_threshold=2000):
    """per_sample_counts: per sample a list over the layers of int arrays (neighbours of every point inside the layer's radius, itself
    included) -> (hists int32 [num_layers, hist_n], limits, samples used): bincount below hist_n, the stop rule, the percentile"""
    hists = np.zeros((num_layers, hist_n), np.int32)
    used = 0
    for counts in per_sample_counts:
        hists += np.vstack([np.bincount(np.minimum(c, hist_n), minlength=hist_n)[:hist_n] for c in counts]).astype(np.int32)
        used += 1
        if np.min(np.sum(hists, axis=1)) > samples_threshold:
            break
    cumsum = np.cumsum(hists.T, axis=0)
    return hists, np.sum(cumsum < (keep_ratio * cumsum[hist_n - 1, :]), axis=0), used


# ----------------------------------------------------------------------------------------------------------------
# the scenes of tests/golden/collate_gt.npz (minted by tools/golden/make_golden_collate_gt.py), from the project's integer hash
# ----------------------------------------------------------------------------------------------------------------
RADIUS = 0.05
STAGE = 1024            # csrc/collate_gt_index.h: CG_STAGE (reference points per LDS stage); CG_BLOCK = 128 queries per workgroup

# (n_s, n_t, kind): "overlap" = the target holds noisy warped copies of some sources plus strays, "none" = the target lies far away (radius below
# every distance), "all" = every source has its own target (n_s == n_t there), "flow" = overlap with a per-source flow (the 4D form)
MATCH_SCENES = [(2, 3, "overlap"), (3, 2, "overlap"), (63, 65, "overlap"), (64, 63, "overlap"), (65, 64, "overlap"),
                (STAGE + 1, 65, "overlap"), (65, STAGE + 1, "overlap"), (64, 70, "none"), (65, 65, "all"), (130, 257, "overlap"),
                (63, 64, "flow"), (65, 130, "flow")]
# one ragged call each (one radius, flow for all pairs or none): the zero-match pair in the middle of a P = 3 call; every 3D scene; the 4D scenes
MATCH_BATCHES = {"ragged3": [2, 7, 4], "all3d": list(range(10)), "flow4d": [10, 11]}
# (n_query, n_reference, coincident): exactly 4 references; 1 023 / 1 024 / 1 025 around the stage; several stages and two query tiles;
# `coincident` queries ARE reference points (distance 0: the 1e-10 clamp)
BLEND_SCENES = [(5, 4, 0), (64, STAGE - 1, 0), (65, STAGE, 0), (63, STAGE + 1, 0), (130, 2 * STAGE + 52, 0), (40, 300, 12)]
BLEND_BATCHES = {"ragged": [0, 3, 5], "all": list(range(6))}


def _hash():
    from diffreg_hip import synth
    return synth


def match_scene(k, seed):
    """-> dict(src, tgt, rot, trn, flow or None): scene k of MATCH_SCENES under `seed` (the mint script advances the seed until the scene passes
    screen_matches and records it)"""
    sy = _hash()
    ns, nt, kind = MATCH_SCENES[k]
    src = sy.hash_uniform(seed, 1, (ns, 3), 0.0, 1.0).astype(F)
    rot = sy._rodrigues(sy.hash_uniform(seed, 2, (3,)) + np.array([0.0, 0.0, 1.5]), 0.2 + 0.5 * float(sy.hash_u01(seed, 3, 1)[0])).astype(F)
    trn = sy.hash_uniform(seed, 4, (3,), -0.2, 0.2).astype(F)
    flow = (0.03 * sy.hash_normal(seed, 5, (ns, 3))).astype(F) if kind == "flow" else None
    w = warp(src, rot, trn, flow, np.float64)
    if kind == "none":
        tgt = sy.hash_uniform(seed, 6, (nt, 3), 0.0, 1.0) + 3.0
    elif kind == "all":
        tgt = w[np.argsort(sy.hash_u01(seed, 7, nt), kind="stable")] + 0.002 * sy.hash_normal(seed, 8, (nt, 3))
    else:
        m = min(ns, nt, max(1, (2 * min(ns, nt)) // 3))                  # sources that have a noisy copy among the targets
        pick = np.argsort(sy.hash_u01(seed, 7, ns), kind="stable")[:m]
        near = w[pick] + 0.004 * sy.hash_normal(seed, 8, (m, 3))
        stray = sy.hash_uniform(seed, 9, (nt - m, 3), 0.0, 1.0) @ rot.astype(np.float64).T + trn
        tgt = np.concatenate([near, stray])[np.argsort(sy.hash_u01(seed, 10, nt), kind="stable")]
    return dict(src=src, tgt=tgt.astype(F), rot=rot, trn=trn, flow=flow)


def blend_scene(k, seed):
    """-> dict(query, ref, ref_flow): scene k of BLEND_SCENES under `seed`"""
    sy = _hash()
    nq, nr, co = BLEND_SCENES[k]
    ref = sy.hash_uniform(seed, 11, (nr, 3), 0.0, 1.0).astype(F)
    ref_flow = (0.05 * sy.hash_normal(seed, 12, (nr, 3))).astype(F)
    query = sy.hash_uniform(seed, 13, (nq, 3), 0.0, 1.0).astype(F)
    if co:
        query[:co] = ref[np.argsort(sy.hash_u01(seed, 14, nr), kind="stable")[:co]]
    return dict(query=query, ref=ref, ref_flow=ref_flow)


# the hand-made tie scene: equal distances everywhere, every coordinate a small integer.  PINNED TO THE STATED RULE (lowest index) by the float64
# statement above, NOT to the reference, whose argpartition order is unspecified at equal distances.
TIE_MATCH = dict(src=np.array([[0, 0, 0], [2, 0, 0], [4, 0, 0]], F), tgt=np.array([[1, 0, 0], [3, 0, 0], [1, 0, 0], [5, 0, 0]], F),
                 rot=np.eye(3, dtype=F), trn=np.zeros(3, F), radius=1.5)
TIE_BLEND = dict(query=np.array([[0, 0, 0], [1, 1, 0]], F),
                 ref=np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [2, 0, 0], [2, 1, 0], [1, 2, 0]], F),
                 ref_flow=np.array([[1, 0, 0], [0, 2, 0], [0, 0, 4], [8, 0, 0], [0, 16, 0], [0, 0, 32], [64, 0, 0], [0, 128, 0]], F))


# calibration "datasets": (seed, pairs, points per cloud, samples_threshold).  The first stops early under its threshold, the second runs to its
# end (asserted by the mint script), the third has clouds of unequal density
CALIB_CFG = dict(num_layers=4, first_subsampling_dl=0.05, conv_radius=2.5, deform_radius=5.0)
CALIB_DATASETS = [(301, 6, 500, 60), (302, 4, 420, 2000), (303, 5, 640, 150)]


def calib_dataset(k):
    """-> list of (src [n,3], tgt [m,3]) float32: points on a wavy sheet inside the unit cube, a second view rotated a little"""
    sy = _hash()
    seed, pairs, n, _ = CALIB_DATASETS[k]
    out = []
    for p in range(pairs):
        s = seed * 100 + p
        m = n - 37 * p if k == 2 else n
        uv = sy.hash_uniform(s, 1, (m, 2), 0.0, 1.0)
        a = np.stack([uv[:, 0], uv[:, 1], 0.5 + 0.2 * np.sin(5 * uv[:, 0]) * np.cos(4 * uv[:, 1])], 1) + 0.01 * sy.hash_normal(s, 2, (m, 3))
        uv = sy.hash_uniform(s, 3, (m + 11, 2), 0.0, 1.0)
        b = np.stack([uv[:, 0], uv[:, 1], 0.5 + 0.2 * np.sin(5 * uv[:, 0]) * np.cos(4 * uv[:, 1])], 1) + 0.01 * sy.hash_normal(s, 4, (m + 11, 3))
        R = sy._rodrigues(np.array([0.1, 0.3, 1.0]), 0.25)
        out.append((a.astype(F), (b @ R.T + np.array([0.05, -0.02, 0.01])).astype(F)))
    return out


def calib_counts(src, tgt, cfg=None):
    """one sample's neighbour counts per layer along the level loop of collate_fn_3dmatch (synth.KPFCN_ARCH: every level at the normal radius):
    float32 d^2 < float32(r)^2 inside the point's own cloud, grid subsampling by oracle/collate_oracle.py between the levels"""
    from diffreg_hip.collate import encoder_levels
    from oracle import collate_oracle as co
    cfg = cfg or CALIB_CFG
    pts, lens = np.concatenate([src, tgt]).astype(F), np.array([len(src), len(tgt)], np.int32)
    out = []
    for L, (wide_conv, down, _) in enumerate(encoder_levels(_hash().KPFCN_ARCH)):
        cell = cfg["first_subsampling_dl"] * 2 ** L
        r = F(cell * cfg["conv_radius"] * cfg["deform_radius"] / cfg["conv_radius"] if wide_conv else cell * cfg["conv_radius"])
        c, s = [], 0
        for n in lens:
            c.append((d2_matrix(pts[s:s + n], pts[s:s + n]) < r * r).sum(1))
            s += n
        out.append(np.concatenate(c))
        if down:
            pts, lens = co.grid_subsample_batch(pts, lens, 2 * cell * cfg["conv_radius"] / cfg["conv_radius"])
    return out
