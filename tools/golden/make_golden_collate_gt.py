"""Mint the fixture of the 3D / 4D ground-truth collate by RUNNING THE REFERENCE's own functions (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_collate_gt.py REFERENCE_ROOT      # the directory holding Diff-Reg-3dmatch/
    -> tests/golden/collate_gt.npz

Matches and flow: Diff-Reg-3dmatch/datasets/utils.py is imported as it lies (pure numpy) and its blend_scene_flow and multual_nn_correspondence
are called on the scenes of tests/collate_gt_ref.py; the warp in front of the matches is the line of dataloader.py:255 (3D: torch.matmul in
float32) or :517-518 (4D: c_src + c_flow, np.matmul), written out here.  Recorded per scene: the clouds, rot / trn, the flow, the radius, the
reference's outputs, the seed, and for the blend the reference's float32 deviation from the float64 statement of the same formula
(tests/collate_gt_ref.blend_flow_knn3(dtype=float64)): the bar of the device test is a multiple of THAT.

Screening, asserted here on the inputs in float64 (a scene that fails is drawn again with the next seed, and the seed is recorded): for every
point the relative gap between its nearest and second-nearest d^2 exceeds 1e-4 (for the blend: among neighbours 1 to 4), and no nearest distance
lies within 1e-4 radius of the radius.  Under these conditions the result depends neither on the rounding of the reference's BLAS nor on the
unspecified order np.argpartition leaves equal distances in, so the reference alone carries every exact-equality claim of the tests.

Calibration: the body of calibrate_neighbors (dataloader.py:566-588: bincount of the counts below hist_n, the stop rule after every sample, the
percentile) run over neighbour matrices produced by the REFERENCE'S C++ -- cpp_subsampling / cpp_neighbors compiled into
oracle/_ref/libref_collate.so by oracle/Makefile (build()), called through oracle/collate_oracle.ref_subsample_batch / ref_batch_query -- along
the level loop of collate_fn_3dmatch (dataloader.py:120-211) with neighborhood_limits = [hist_n] * 5, on the hash-drawn datasets of
tests/collate_gt_ref.CALIB_DATASETS.  Asserted here: the first dataset stops before its last sample, the second runs to its end.

The hand-made tie scene is NOT minted from the reference: it is pinned to the stated rule by the float64 statement (tests/collate_gt_ref.py).
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "diff-reg_amd")):
    sys.path.insert(0, p)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from tests import collate_gt_ref as cg          # noqa: E402
from diffreg_hip import synth                   # noqa: E402
from diffreg_hip.collate import encoder_levels  # noqa: E402


def reference_utils(ref_root):
    spec = importlib.util.spec_from_file_location("ref_datasets_utils", os.path.join(ref_root, "Diff-Reg-3dmatch", "datasets", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_warp(sc):
    import torch
    if sc["flow"] is None:                  # dataloader.py:255
        return (torch.matmul(torch.from_numpy(sc["rot"]), torch.from_numpy(sc["src"]).T) + torch.from_numpy(sc["trn"].reshape(3, 1))).T.numpy()
    deformed = sc["src"] + sc["flow"]       # dataloader.py:517-518
    return (np.matmul(sc["rot"], deformed.T) + sc["trn"].reshape(3, 1)).T


def calibration(ref_counts_of, k):
    _, _, _, threshold = cg.CALIB_DATASETS[k]
    cfg = cg.CALIB_CFG
    hist_n = cg.hist_bins(cfg["deform_radius"])
    data = cg.calib_dataset(k)
    hists = np.zeros((cfg["num_layers"], hist_n), dtype=np.int32)
    used = 0
    for src, tgt in data:                   # dataloader.py:570-583
        counts = ref_counts_of(src, tgt, hist_n)
        hists += np.vstack([np.bincount(c, minlength=hist_n)[:hist_n] for c in counts]).astype(np.int32)
        used += 1
        if np.min(np.sum(hists, axis=1)) > threshold:
            break
    cumsum = np.cumsum(hists.T, axis=0)     # dataloader.py:585-586
    limits = np.sum(cumsum < (0.8 * cumsum[hist_n - 1, :]), axis=0)
    return hists, limits, used, len(data)


def main(ref_root):
    from oracle import collate_oracle as co
    ru = reference_utils(ref_root)
    out = {}
    for k, (ns, nt, kind) in enumerate(cg.MATCH_SCENES):
        for seed in range(1000 + 50 * k, 1050 + 50 * k):
            sc = cg.match_scene(k, seed)
            if cg.screen_matches(sc["src"], sc["tgt"], sc["rot"], sc["trn"], cg.RADIUS, sc["flow"]):
                break
        else:
            raise SystemExit("match scene %d: no seed passes the screening" % k)
        m = ru.multual_nn_correspondence(reference_warp(sc), sc["tgt"], search_radius=cg.RADIUS)
        if kind == "none":
            assert m.shape[1] == 0
        if kind == "all":
            assert m.shape[1] == ns
        for name in ("src", "tgt", "rot", "trn"):
            out["m%d_%s" % (k, name)] = sc[name]
        if sc["flow"] is not None:
            out["m%d_flow" % k] = sc["flow"]
        out["m%d_matches" % k] = m.astype(np.int64)
        out["m%d_seed" % k] = np.array([seed])
        print("match scene %2d (%4d, %4d, %-7s) seed %d: %d matches" % (k, ns, nt, kind, seed, m.shape[1]))
    for k, (nq, nr, coincident) in enumerate(cg.BLEND_SCENES):
        for seed in range(2000 + 50 * k, 2050 + 50 * k):
            sc = cg.blend_scene(k, seed)
            if cg.screen_blend(sc["query"], sc["ref"]):
                break
        else:
            raise SystemExit("blend scene %d: no seed passes the screening" % k)
        flow = ru.blend_scene_flow(sc["query"], sc["ref"], sc["ref_flow"], knn=3)
        assert flow.dtype == np.float32
        dev = np.abs(flow.astype(np.float64) - cg.blend_flow_knn3(sc["query"], sc["ref"], sc["ref_flow"], np.float64)).max()
        for name in ("query", "ref", "ref_flow"):
            out["b%d_%s" % (k, name)] = sc[name]
        out["b%d_out" % k] = flow
        out["b%d_dev" % k] = np.array([dev])
        out["b%d_seed" % k] = np.array([seed])
        print("blend scene %d (%4d queries, %4d references) seed %d: float32 deviation of the reference %.3e" % (k, nq, nr, seed, dev))
    assert co.ref_lib() is not None, "oracle/_ref/libref_collate.so is missing: run `python __graft_entry__.py build` first"
    cfg = cg.CALIB_CFG
    levels = encoder_levels(synth.KPFCN_ARCH)

    def ref_counts_of(src, tgt, hist_n):
        pts, lens = np.concatenate([src, tgt]), np.array([len(src), len(tgt)], np.int32)
        r_normal, counts = cfg["first_subsampling_dl"] * cfg["conv_radius"], []
        for wide_conv, down, _ in levels:
            assert wide_conv is False                                      # KPFCN_ARCH: every level convolves at the normal radius
            mat = co.ref_batch_query(pts, pts, lens, lens, r_normal)[:, :hist_n]
            counts.append(np.sum(mat < mat.shape[0], axis=1))              # dataloader.py:574
            if down:
                pts, lens = co.ref_subsample_batch(pts, lens, 2 * r_normal / cfg["conv_radius"])
            r_normal *= 2
        return counts

    for k in range(len(cg.CALIB_DATASETS)):
        hists, limits, used, n = calibration(ref_counts_of, k)
        if k == 0:
            assert used < n, "dataset 0 must stop early"
        if k == 1:
            assert used == n and not np.min(np.sum(hists, axis=1)) > cg.CALIB_DATASETS[k][3], "dataset 1 must run to its end"
        nz = np.nonzero(hists.sum(0))[0]
        out["c%d_hists" % k] = hists[:, :int(nz.max()) + 1]               # the bins behind the last occupied one are zero
        out["c%d_limits" % k] = limits.astype(np.int64)
        out["c%d_used" % k] = np.array([used])
        print("calibration dataset %d: %d of %d samples, row sums %s, limits %s" % (k, used, n, hists.sum(1), limits))
    path = os.path.join(GOLDEN, "collate_gt.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
