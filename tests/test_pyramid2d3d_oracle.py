"""CPU: the graph-pyramid fixture (tests/golden/pyramid2d3d.npz, recorded from the reference's collate-time C++) against the float64 pyramid
functions of tests/pcd_backbone2d3d_ref.py, and the calibration rule on its histograms.

The restatement works in float64 on the float32 coordinates, the reference in float32, so the two agree up to float32 rounding:
  * barycentres: the reference sums a voxel's n points in float32 in input order: n - 1 additions, each rounded by at most 2^-24 of a partial sum
    <= n M (M = the largest coordinate), then one product: |bary32 - bary64| <= (n + 2) 2^-24 M, with n the fullest voxel of the stage.  Points
    are matched by nearest row (the reference emits hash-map order, the restatement key order).
  * neighbour rows: d^2 of a kept pair is below r^2 <= 2^-2 and carries at most 4 roundings of 2^-24 of a value <= r^2: TAU = 4 2^-24 r^2.  A row
    that is not identical to the restatement's must be explained by that: its float64 d^2 ascend within TAU, every member lies below r^2 + TAU, and
    it holds as many entries as the cut allows of the supports below r^2 - TAU."""
import numpy as np
import pytest

from tests import pcd_backbone2d3d_ref as B
from tests import pyramid2d3d_ref as R

_G = {}


def _golden():
    if not _G:
        _G["g"] = R.load()
    return _G["g"]


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)])


@pytest.mark.parametrize("name", R.SCENES)
def test_stage_points_agree_with_float64_subsample(name):
    g = _golden()[0][name]
    assert np.array_equal(R.scene(name, g["seed"])[0], g["points"][0]) and np.array_equal(R.scene(name, g["seed"])[1], g["lengths"][0])
    for i in range(1, R.NUM_STAGES):
        voxel = R.VOXEL * 2 ** i
        fo, co = _offsets(g["lengths"][i - 1]), _offsets(g["lengths"][i])
        assert co[-1] == len(g["points"][i])
        for b in range(len(g["lengths"][0])):
            fine, coarse = g["points"][i - 1][fo[b]:fo[b + 1]], g["points"][i][co[b]:co[b + 1]]
            if len(fine) == 0:
                assert len(coarse) == 0
                continue
            ref = B.grid_subsample(fine, voxel)
            n = int(np.unique(np.floor(fine.astype(np.float64) / voxel).astype(np.int64), axis=0, return_counts=True)[1].max())
            tol = (n + 2) * 2.0 ** -24 * float(np.abs(fine).max())
            assert len(ref) == len(coarse), (i, b, len(ref), len(coarse))
            R.match_rows(ref, coarse, tol)


def _check_row(q, s, row, r, limit):
    """a golden row (cloud-local indices, -1 = padding) that differs from the restatement's"""
    tau = 4 * 2.0 ** -24 * r * r
    d2 = ((s.astype(np.float64) - q.astype(np.float64)) ** 2).sum(1)
    kept = row[row >= 0]
    assert len(np.unique(kept)) == len(kept)
    dk = d2[kept]
    assert (dk < r * r + tau).all() and (np.diff(dk) >= -tau).all()
    lo, hi = min(int((d2 < r * r - tau).sum()), limit), min(int((d2 < r * r + tau).sum()), limit)
    assert lo <= len(kept) <= hi
    if len(kept) == limit and len(d2) > limit:                 # cut: nothing dropped is nearer than the last kept one by more than tau
        assert dk[-1] <= np.partition(d2, limit - 1)[limit - 1] + tau


def _compare(g, qs, ss, r, limit, got):
    q_all, s_all = g["points"][qs], g["points"][ss]
    qo, so = _offsets(g["lengths"][qs]), _offsets(g["lengths"][ss])
    width, differing = 0, 0
    for b in range(len(g["lengths"][0])):
        q, s = q_all[qo[b]:qo[b + 1]], s_all[so[b]:so[b + 1]]
        rows = got[qo[b]:qo[b + 1]]
        if len(q) == 0:
            continue
        if len(s) == 0:
            assert (rows == len(s_all)).all()
            continue
        ref = B.radius_search(q, s, r, limit)
        width = max(width, ref.shape[1] if (ref != len(s)).any() else 0)
        local = np.where(rows == len(s_all), -1, rows - so[b])                     # no leakage: every index inside the query's own cloud
        assert ((local >= -1) & (local < len(s))).all()
        refl = np.full_like(local, -1)
        w = min(ref.shape[1], local.shape[1])
        refl[:, :w] = np.where(ref[:, :w] == len(s), -1, ref[:, :w])
        assert (ref[:, w:] == len(s)).all()
        for j in np.nonzero((local != refl).any(1))[0]:
            differing += 1
            _check_row(q[j], s, local[j], r, limit)
    assert got.shape[1] == width
    return differing


@pytest.mark.parametrize("name", R.SCENES)
def test_index_matrices_agree_with_float64_radius_search(name):
    g = _golden()[0][name]
    differing = 0
    for i in range(R.NUM_STAGES):
        r = R.RADIUS * 2 ** i
        differing += _compare(g, i, i, r, R.LIMITS[i], g["neighbors"][i])
        if i == 0:
            differing += _compare(g, 0, 0, r, g["narrow_limit"], g["neighbors0_narrow"])
        if i < R.NUM_STAGES - 1:
            differing += _compare(g, i + 1, i, r, R.LIMITS[i], g["subsampling"][i])
            differing += _compare(g, i, i + 1, 2 * r, R.LIMITS[i + 1], g["upsampling"][i])
    print("scene %s: %d rows differ from the float64 restatement within float32 rounding" % (name, differing))


def test_origin_scene_separates_the_two_grid_origins():
    """scene "origin": at every stage the cloud's minimum is a float at which vision3d's origin floor(min / v) * v and KPConv's
    floor(min * (1 / v)) * v differ, the golden's number of voxels is the one vision3d's origin gives on the golden's previous stage, and KPConv's
    origin gives another number at stages 1 and 2 -- so a device subsample that took KPConv's origin cannot reproduce this scene.  No other scene has such a minimum
    (asserted too: the day one does, this scene is no longer the only guard)."""
    scenes = _golden()[0]
    g = scenes["origin"]
    for i in range(1, R.NUM_STAGES):
        v, prev = R.VOXEL * 2 ** i, g["points"][i - 1]
        o_v3d, o_kp = R.origin_forms(prev.min(0), v)
        assert (o_v3d != o_kp).all(), (i, o_v3d, o_kp)
        assert R.occupied_voxels(prev, o_v3d, v) == len(g["points"][i])
        if i < R.NUM_STAGES - 1:                               # stage 3: the origins lie a whole voxel apart and no point sits on a face
            assert R.occupied_voxels(prev, o_kp, v) != len(g["points"][i])
    for name in R.SCENES[:-1]:
        h = scenes[name]
        for i in range(1, R.NUM_STAGES):
            fo = _offsets(h["lengths"][i - 1])
            for b in range(len(fo) - 1):
                if fo[b + 1] > fo[b]:
                    o_v3d, o_kp = R.origin_forms(h["points"][i - 1][fo[b]:fo[b + 1]].min(0), R.VOXEL * 2 ** i)
                    assert (o_v3d == o_kp).all(), (name, i, b)


def test_canonical_ties_moves_nothing_outside_runs():
    q = np.zeros((1, 3), np.float32)
    s = np.array([[0.3, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0.2, 0, 0]], np.float32)
    row = np.array([[2, 1, 0, 3, 4]])                          # d^2: .01 .01 .09 .04 inf -- one run (2, 1), and a mis-ordered pair (0, 3)
    assert np.array_equal(R.canonical_ties(q, s, row), [[1, 2, 0, 3, 4]])


def test_histograms_and_calibrated_limits():
    scenes, limits = _golden()
    assert R.HIST_N == 180
    for name in R.SCENES:
        g = scenes[name]
        for i in range(R.NUM_STAGES):
            assert g["hist"].dtype == np.int32 and g["hist"].shape == (R.NUM_STAGES, R.HIST_N)
            assert np.array_equal(g["hist"][i], np.bincount(g["counts"][i], minlength=R.HIST_N)[:R.HIST_N])
            # below the limit the calibration's counts are the row counts of the neighbour matrix
            row = (g["neighbors"][i] != len(g["points"][i])).sum(1)
            assert np.array_equal(np.minimum(g["counts"][i], R.LIMITS[i]), row)
    for thr in R.THRESHOLDS:
        got, used = R.calibrate_from_hists([scenes[s]["hist"] for s in R.SCENES], R.KEEP_RATIO, thr)
        assert np.array_equal(got, limits[thr][0]) and used == limits[thr][1]
    assert limits[R.THRESHOLDS[0]][1] == len(R.SCENES) and limits[R.THRESHOLDS[1]][1] < len(R.SCENES)


def test_pyramidless_pack_mode_hands_points_and_lengths_through():
    from diffreg_hip import pyramid2d3d as P
    points, lengths = np.zeros((5, 3), np.float32), np.array([5])
    out = P.pyramidless_pack_mode(points, lengths, 4, 0.025, 0.0625, [40, 36, 36, 36])
    assert set(out) == {"points", "lengths"} and out["points"] is points and out["lengths"] is lengths
