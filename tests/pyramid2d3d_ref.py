"""Test-side definitions of the 2D-3D graph-pyramid fixture (tests/golden/pyramid2d3d.npz, minted by tools/golden/make_golden_pyramid2d3d.py from the
reference's own collate-time C++): the scenes, the storage of the index matrices, and the calibration rule of vision3d/utils/dataloader.py:42-67 on
recorded histograms, in our own words.  The pyramid constants are those of tests/pcd_backbone2d3d_ref.py.

Every scene is a batch of clouds cut from the scenes of tests/partition2d3d_ref.make_scene ("c": 600 points, sparse; "d": 3 000 points, denser):
    sparse  [c]                                 dense  [d]
    two     [c[:300], d[:500]]                  one    [c[:200], one point of d, d[:300]]        (a 1-point cloud inside a batch)
    empty   [d[:400], no points, c[:250]]       neg    [d[:500] - (2, 3, 2.5)]                   (every coordinate negative)
    faces   [c[:300], one hash-chosen coordinate of two points in three moved onto a multiple of the stage-1 voxel, rounded to float32]
    origin  [three lone points carrying the cloud's minimum 2.6 on one axis each, then d[:400] moved into [2.9, 4.8)^3 with face coordinates as
             in `faces`, no multiple of 0.2]: float32(2.6) = 52 x 0.05 = 26 x 0.1 = 13 x 0.2 is a minimum at which vision3d's grid origin floor(min / v) * v and
             KPConv's floor(min * (1 / v)) * v are different floats at every stage's voxel size (2.55 / 2.6000001, 2.5 / 2.6000001, 2.4 / 2.6000001),
             and the lone points are alone in their voxels, so they carry the minimum unchanged into every stage.  With KPConv's origin the
             minimum lies below the origin and the face points fall into other voxels: the number of occupied voxels differs at stages 1 and 2
             (tests/test_pyramid2d3d_oracle.py asserts both; at stage 3 the two origins lie a whole voxel apart and no point sits on a face), so
             the scene tells the two device entries apart.
seed > 0 (the minting script's re-seeding after a tied neighbour row) adds a hash-drawn jitter of +-1e-4 to every coordinate before the cuts.
"""
import os

import numpy as np

from tests.partition2d3d_ref import _hash01, make_scene
from tests.pcd_backbone2d3d_ref import LIMITS, NUM_STAGES, RADIUS, VOXEL  # noqa: F401  (re-exported)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pyramid2d3d.npz")
SCENES = ("sparse", "dense", "two", "one", "empty", "neg", "faces", "origin")
HIST_N = int(np.ceil(4 / 3 * np.pi * (RADIUS / VOXEL + 1) ** 3))          # 180 (dataloader.py:46)
KEEP_RATIO = 0.8
THRESHOLDS = (2000, 300)         # sample_threshold: the default (never reached by eight small scenes) and one that stops the loop early
INDEX_KEYS = ("neighbors", "subsampling", "upsampling")

_BASE = {}


def _base(name, seed):
    if (name, seed) not in _BASE:
        p = make_scene(name)["pcd_points"].numpy().astype(np.float32).copy()
        if seed > 0:
            j = _hash01(np.arange(p.size), 9000 + seed).reshape(p.shape) * 2.0 - 1.0
            p = (p.astype(np.float64) + 1e-4 * j).astype(np.float32)
        _BASE[(name, seed)] = p
    return _BASE[(name, seed)]


def _on_faces(p, v, hash_seed, coarsest=None):
    """one hash-chosen coordinate of two points in three moved onto a multiple of v, rounded to float32 (a point with all three coordinates on
    faces sits on a lattice, whose symmetric neighbourhoods tie in d^2).  Kept where the float32 rounding of k v does not fall below k v: there the
    float64 statement of the voxel grid (tests/pcd_backbone2d3d_ref.grid_subsample, faces at multiples of the double v) and the reference's float32
    one name the same voxel, which the CPU oracle test asserts; a face value rounded downwards belongs to voxel k - 1 in float64, k in float32.
    coarsest = n: no k that is a multiple of n, so that no coordinate is a face of the stage with voxel n v (a point alone in its voxels carries
    its coordinates into the coarser stages, whose float32 origin is another one; on an exact face there float32 and float64 can part ways again)"""
    p = p.copy()
    axis = np.floor(_hash01(np.arange(len(p)), hash_seed) * 4.5).astype(np.int64)
    pick = axis[:, None] == np.arange(3)[None, :]
    face = np.rint(p.astype(np.float64) / v) * v
    snapped = face.astype(np.float32)
    pick &= snapped.astype(np.float64) >= face
    if coarsest:
        pick &= np.rint(face / v).astype(np.int64) % coarsest != 0
    p[pick] = snapped[pick]
    return p


def scene(name, seed=0):
    """-> (points float32 [n, 3], lengths int64 [B])"""
    c, d = _base("c", seed), _base("d", seed)
    if name == "sparse":
        clouds = [c]
    elif name == "dense":
        clouds = [d]
    elif name == "two":
        clouds = [c[:300], d[:500]]
    elif name == "one":
        clouds = [c[:200], d[1234:1235], d[:300]]
    elif name == "empty":
        clouds = [d[:400], d[:0], c[:250]]
    elif name == "neg":
        clouds = [d[:500] - np.array([2.0, 3.0, 2.5], dtype=np.float32)]
    elif name == "faces":
        clouds = [_on_faces(c[:300], 2 * VOXEL, 4242)]
    elif name == "origin":
        body = d[:400] - d[:400].min(0) + np.float32(0.3) + np.float32(2.6)
        lone = np.array([[2.6, 3.43, 3.43], [3.43, 2.6, 3.43], [3.43, 3.43, 2.6]], dtype=np.float32)
        clouds = [np.concatenate([lone, _on_faces(body.astype(np.float32), 2 * VOXEL, 777, coarsest=4)], 0)]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(np.concatenate(clouds, 0)), np.array([len(x) for x in clouds], dtype=np.int64)


def pack(key, a):
    """index matrices are stored as the two byte planes of uint16 values (every index and every padding value of the fixture is below 65 536; the
    high bytes compress)"""
    if key.startswith(INDEX_KEYS):
        assert a.size == 0 or (a.min() >= 0 and a.max() < 65536)
        return np.stack([(a >> 8).astype(np.uint8), (a & 255).astype(np.uint8)])
    return a


def unpack(planes):
    return (planes[0].astype(np.int64) << 8) | planes[1].astype(np.int64)


def load():
    """-> {scene: dict(points [4], lengths [4], neighbors [4], subsampling [3], upsampling [3], neighbors0_narrow, narrow_limit, counts [4], hist, ...)},
    {threshold: (limits, samples used)}; index matrices back as int64"""
    z = np.load(GOLDEN)
    out = {}
    for s in SCENES:
        g = lambda k: z[s + "/" + k]
        i64 = lambda k: unpack(g(k))
        # neighbors0_narrow: radius_search_pack_mode cuts the columns of one and the same matrix (radius_search.py:24-26), so the narrow matrix
        # is the stored one's first narrow_limit columns
        out[s] = dict(points=[g("points%d" % i) for i in range(NUM_STAGES)], lengths=[g("lengths%d" % i) for i in range(NUM_STAGES)],
                      neighbors=[i64("neighbors%d" % i) for i in range(NUM_STAGES)],
                      subsampling=[i64("subsampling%d" % i) for i in range(NUM_STAGES - 1)],
                      upsampling=[i64("upsampling%d" % i) for i in range(NUM_STAGES - 1)],
                      narrow_limit=int(g("narrow_limit").item()), subsampling_tied_rows=int(g("tied_subsampling_rows").item()),
                      counts=[g("counts%d" % i) for i in range(NUM_STAGES)], hist=g("hist"), seed=int(g("seed").item()))
        out[s]["neighbors0_narrow"] = out[s]["neighbors"][0][:, :out[s]["narrow_limit"]]
    limits = {t: (z["limits_t%d" % t], int(z["used_t%d" % t][0])) for t in THRESHOLDS}
    return out, limits


def calibrate_from_hists(hists, keep_ratio, sample_threshold):
    """dataloader.py:53-65 on per-sample histograms [num_stages, hist_n]: accumulate sample after sample, stop after the first sample that leaves
    every stage with more than sample_threshold recorded queries; limit of a stage = the number of bins whose cumulative sum is below keep_ratio
    times the stage's total.  -> (limits int [num_stages], samples used)"""
    acc = np.zeros_like(np.asarray(hists[0]), dtype=np.int32)
    used = 0
    for h in hists:
        acc += h
        used += 1
        if np.min(np.sum(acc, axis=1)) > sample_threshold:
            break
    cum = np.cumsum(acc.T, axis=0)
    return np.sum(cum < (keep_ratio * cum[-1, :]), axis=0), used


def d2_f32(q, s, idx):
    """float32 d^2 of every (row, entry) of an index matrix in nanoflann's order of operations, ((0 + dx dx) + dy dy) + dz dz, numpy float32
    (no contraction); padding entries (index len(s)) -> inf"""
    s_pad = np.concatenate([np.asarray(s, np.float32), np.zeros((1, 3), np.float32)], 0)
    d = np.asarray(q, np.float32)[:, None, :] - s_pad[idx]
    out = np.zeros(idx.shape, np.float32)
    for k in range(3):
        out = out + d[:, :, k] * d[:, :, k]
    out[idx == len(s)] = np.inf
    return out


def origin_forms(mn, v):
    """the two float32 statements of a cloud's grid origin at its minimum mn [3] and voxel size v: vision3d's floor(min / v) * v
    (vision3d/csrc/cpu/grid_subsampling/grid_subsampling.cpp:32) and KPConv's floor(min * (1 / v)) * v"""
    mn, v = np.asarray(mn, np.float32), np.float32(v)
    return np.floor(mn / v) * v, np.floor(mn * (np.float32(1) / v)) * v


def occupied_voxels(points, origin, v):
    """number of distinct float32 voxel indices floor((p - origin) / v) of a cloud"""
    idx = np.floor((np.asarray(points, np.float32) - np.asarray(origin, np.float32)) / np.float32(v)).astype(np.int64)
    return len(np.unique(idx, axis=0))


def canonical_ties(q, s, idx):
    """the rows of an index matrix with every run of equal float32 d^2 (neighbouring entries of the row) put in ascending index order; nothing
    else moves: a row without such a run is returned as it is, whatever its order.  A barycentre of exactly two points is as far from the one as
    from the other, so the subsampling matrices hold such runs in every scene; the reference's std::sort leaves their order to the kd-tree's
    traversal, the device takes the lower index first."""
    if idx.shape[1] < 2:
        return idx
    d2 = d2_f32(q, s, idx)
    with np.errstate(invalid="ignore"):
        new_run = np.concatenate([np.ones((len(idx), 1), bool), d2[:, 1:] != d2[:, :-1]], 1)
    run = np.cumsum(new_run, 1)                       # ascending along the row by construction: sorting by (run, index) stays inside the runs
    o = np.lexsort((idx, run), axis=1)
    return np.take_along_axis(idx, o, axis=1)


def match_rows(a, b, tol=0.0):
    """perm with a[perm] == b row for row (within tol per coordinate), a and b [n, 3] holding the same points in another order; every row of a is
    used once.  Brute force in blocks (n is a few thousand)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    perm = np.empty(len(b), dtype=np.int64)
    for i0 in range(0, len(b), 512):
        d = np.abs(b[i0:i0 + 512, None, :] - a[None, :, :]).max(-1)
        perm[i0:i0 + 512] = d.argmin(1)
        assert (d.min(1) <= tol).all(), float(d.min(1).max())
    assert len(np.unique(perm)) == len(perm)
    return perm
