"""Plain float32 numpy statements of the two furthest-point sampling loops of vision3d, as the device states them (include/diffreg_hip.h,
seventeenth set), and the scenes of tests/golden/fps.npz.

nodes():  sample_nodes_with_fps (2D-3D vision3d/csrc/cpu/node_sampling/node_sampling.cpp:10-78) / native_furthest_point_sample
          (vision3d/array_ops/furthest_point_sample.py:22-66): d = sqrt((dx dx + dy dy) + dz dz) in float32, the running minimum from +inf,
          selection by strict > from 0, the num_samples test before the scan, the stop at best < min_distance.
batch():  furthest_point_sample_kernel (vision3d/csrc/cuda/furthest_point_sample/furthest_point_sample_cuda.cuh:29-88): the squared distance,
          the running minimum from 1e10, strict > from -1, no stop.
Both include the device's two stated rules: among equal distances the LOWEST index wins (np.argmax returns the first maximum), and a point
with a NaN or Inf coordinate has the distance key -inf for good: it is never selected and never enters the stop test."""
import numpy as np

ST_SIZE, ST_OFFSETS, ST_NONFINITE, ST_CAP, ST_START = 1, 2, 8, 64, 128
F32 = np.float32


def _dist(pts, last, squared):
    with np.errstate(all="ignore"):
        diff = pts[last][None, :] - pts                              # cur - point, float32
        s = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
        return s if squared else np.sqrt(s)


def nodes(points, min_distance=None, num_samples=None, sample_cap=None, squared=False, margins=None):
    """-> (indices int64 [count], distances float32 [count], status).  margins: a list that receives per selection (winner's distance,
    runner-up's distance), for the fixture's screen."""
    pts = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    n = pts.shape[0]
    md = F32(-1.0 if min_distance is None else min_distance)
    ns = -1 if num_samples is None else int(num_samples)
    if not md > 0 and ns <= 0:
        raise ValueError("neither stop rule")
    cap = int(sample_cap) if sample_cap is not None else (ns if ns > 0 else max(n, 1))
    if cap < 1:
        raise ValueError("sample_cap")
    empty = (np.zeros(0, np.int64), np.zeros(0, F32))
    if n == 0:
        return empty + (0,)
    fin = np.isfinite(pts).all(axis=1)
    status = 0 if fin.all() else ST_NONFINITE
    if not fin[0]:
        return empty + (status | ST_START,)
    d = np.where(fin, F32(np.inf), F32(-np.inf)).astype(F32)
    sel, dist, last = [0], [F32(0)], 0
    while not (ns > 0 and len(sel) >= ns):
        d = np.fmin(d, _dist(pts, last, squared))                    # -inf stays -inf whatever the distance evaluates to
        best = int(np.argmax(d))                                     # the first maximum: the lowest index
        bd = d[best]
        if margins is not None:
            rest = np.delete(d, best)
            margins.append((float(bd), float(rest.max()) if rest.size else 0.0))
        if not bd > 0:                                               # no candidate: every remaining distance is 0
            break
        if bd < md:
            break
        if len(sel) >= cap:
            status |= ST_CAP
            break
        sel.append(best)
        dist.append(bd)
        last = best
    return np.asarray(sel, np.int64), np.asarray(dist, F32), status


def batch(points, num_samples):
    """points [B, N, 3] -> indices int64 [B, num_samples]"""
    pts = np.ascontiguousarray(points, dtype=F32)
    B, N, M = pts.shape[0], pts.shape[1], int(num_samples)
    out = np.zeros((B, M), np.int64)
    for b in range(B):
        fin = np.isfinite(pts[b]).all(axis=1)
        d = np.where(fin, F32(1e10), F32(-np.inf)).astype(F32)
        last = 0
        for s in range(1, M):
            d = np.fmin(d, _dist(pts[b], last, True))                # a non-finite point 0 updates nothing: fmin ignores NaN, 1e10 < inf
            best = int(np.argmax(d))
            last = best if d[best] > -1 else 0
            out[b, s] = last
    return out


# ---- the scenes of tests/golden/fps.npz: (name, points, kind, min_distance, num_samples); the seed is found when minting (the screen) and
# the points are stored, so a test never regenerates them
BLOCK = 1024     # FPS_BLOCK of csrc/fps_index.h
SCENES = (
    ("n1", 1, "uniform", 0.1, None),
    ("n2", 2, "uniform", None, 2),
    ("n63", 63, "uniform", 0.3, None),
    ("n64", 64, "uniform", None, 20),
    ("n65", 65, "uniform", 0.2, 30),
    ("n1023", BLOCK - 1, "uniform", 0.15, None),
    ("n1024", BLOCK, "uniform", None, 100),
    ("n1025", BLOCK + 1, "uniform", 0.3, 200),         # both rules given, min_distance stops (about 160 nodes)
    ("surface9000", 9000, "surface", 0.06, 512),       # both rules given, num_samples stops (as n65)
)
STOPPED_BY_MIN_DISTANCE_WITH_BOTH_RULES = "n1025"      # the minting script and the CPU test hold the fixture to this


def scene_points(n, kind, seed):
    """uniform: [-1, 1]^3; surface: a 4DMatch-like smooth sheet over [-1, 1]^2 (diffreg_hip.synth's hash streams), float32"""
    from diffreg_hip import synth
    if kind == "uniform":
        return synth.hash_uniform(seed, 0, (n, 3)).astype(F32)
    xy = synth.hash_uniform(seed, 1, (n, 2)).astype(np.float64)
    z = 0.3 * np.sin(2.1 * xy[:, 0] + 0.4) * np.cos(1.7 * xy[:, 1]) + 0.1 * xy[:, 0] * xy[:, 1]
    z = z + 0.004 * synth.hash_uniform(seed, 2, (n,)).astype(np.float64)
    return np.concatenate([xy, z[:, None]], axis=1).astype(F32)
