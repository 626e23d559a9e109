"""Mint the fixture of the 3D / 4D dataset item by RUNNING THE REFERENCE's own two __getitem__ bodies (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_item3d.py REFERENCE_ROOT      # the directory holding Diff-Reg-3dmatch/
    -> tests/golden/item3d.npz

Diff-Reg-3dmatch/datasets/_3dmatch.py and _4dmatch.py are imported as they lie; modules this machine lacks (open3d, easydict, ...) are stubbed
the way the other mint tools stub them.  A dataset object is made without its __init__ (which reads the split lists of the real datasets) and
given the attributes __getitem__ reads; its files are the scenes of tests/item3d_ref.py written as .pth / .npz into a temporary directory.
np.random.permutation and np.random.rand are wrapped so that every draw of a call is recorded, in order; torch.load is called with
weights_only=False, which the torch of the reference's time defaulted to (the .pth files hold numpy arrays).

Open3D is NOT importable here, so KDTree_corr's search (benchmark_utils.py:174-185: one search_radius_vector_3d per source point) is replaced,
when minting, by a float64 brute-force statement of the same predicate, |tsfm src_i - tgt_j| < search_voxel_size, in ascending (i, j) order
(Open3D returns a row's partners by ascending distance).  Parity with Open3D itself is therefore not claimed: the fixture pins the predicate and
everything the reference's own numpy code does in front of it.

Screening, asserted here in float64 on the reference's own outputs: a 3DMatch scene is kept only when no pair distance lies within GAPR of the
radius (tests/item3d_ref.near_radius == 0), so no pair is left out of any comparison; a scene that fails, or whose coin fell on the other
branch than the case asks for, is drawn again with the next seed, and the seed is recorded.
"""
import importlib.util
import os
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

from tests import item3d_ref as R          # noqa: E402


def reference_datasets(ref_root):
    import torch
    tree = os.path.join(ref_root, "Diff-Reg-3dmatch")
    sys.path.insert(0, tree)
    for m in ("open3d", "easydict", "tqdm", "sklearn", "sklearn.neighbors"):
        try:
            __import__(m)
        except ModuleNotFoundError:
            sys.modules[m] = MagicMock()
    mods = []
    for name in ("_3dmatch", "_4dmatch"):
        while True:
            try:
                spec = importlib.util.spec_from_file_location("ref_" + name, os.path.join(tree, "datasets", name + ".py"))
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                break
            except ModuleNotFoundError as e:
                sys.modules[e.name] = MagicMock()
        mods.append(mod)

    def brute_force_correspondences(src_pcd, tgt_pcd, trans, search_voxel_size, K=None):     # benchmark_utils.py:166-185 without Open3D
        assert K is None
        return torch.from_numpy(R.radius_pairs(np.asarray(src_pcd), np.asarray(tgt_pcd), trans[:3, :3], trans[:3, 3], search_voxel_size))

    mods[0].get_correspondences = brute_force_correspondences
    mods[0].to_o3d_pcd = lambda xyz: np.asarray(xyz)
    load = torch.load
    torch.load = lambda *a, **k: load(*a, **dict(k, weights_only=False))
    return mods


class Recorder:
    """np.random.permutation / np.random.rand with every result kept, in call order"""

    def __init__(self):
        self.perm, self.rand = np.random.permutation, np.random.rand
        self.calls = []

    def __enter__(self):
        def permutation(n):
            out = self.perm(n)
            self.calls.append(("perm", out.copy()))
            return out

        def rand(*shape):
            out = self.rand(*shape)
            self.calls.append(("rand", out.copy()))
            return out

        np.random.permutation, np.random.rand = permutation, rand
        return self

    def __exit__(self, *exc):
        np.random.permutation, np.random.rand = self.perm, self.rand


def draws_of(calls, ns, nt, max_points, aug):
    """the recorded calls by the names tests/item3d_ref.prepare reads (the reference's order: _3dmatch.py:72, 75, 95, 97, 105, 106)"""
    calls, d = list(calls), {}
    if ns > max_points:
        d["src_perm"] = calls.pop(0)[1]
    if nt > max_points:
        d["tgt_perm"] = calls.pop(0)[1]
    if aug:
        d["euler"] = calls.pop(0)[1] * np.pi * 2 / 1.0
        d["coin"] = calls.pop(0)[1][0]
        d["src_jitter"], d["tgt_jitter"] = calls.pop(0)[1], calls.pop(0)[1]
    assert not calls
    return d


def run_case(kind, k, mod, tmp):
    import torch
    case = (R.CASES_3D if kind == "3dmatch" else R.CASES_4D)[k]
    ns, nt, max_points, aug, want_src = case[:5]
    noise = R.NOISE_3D if kind == "3dmatch" else R.NOISE_4D
    for seed in range(100 * k + (5000 if kind == "3dmatch" else 7000), 100 * k + (5100 if kind == "3dmatch" else 7100)):
        raw = R.scene(kind, k, seed)
        cfg = MagicMock()
        if kind == "3dmatch":
            D = mod._3DMatch.__new__(mod._3DMatch)
            torch.save(raw["src"], os.path.join(tmp, "src.pth"))
            torch.save(raw["tgt"], os.path.join(tmp, "tgt.pth"))
            D.infos = dict(rot=[raw["rot"]], trans=[raw["trans"]], src=["src.pth"], tgt=["tgt.pth"])
        else:
            D = mod._4DMatch.__new__(mod._4DMatch)
            entry = dict(rot=raw["rot"], trans=raw["trans"], s2t_flow=raw["flow"], s_pc=raw["src"], t_pc=raw["tgt"],
                         correspondences=raw["correspondences"])
            if "metric_index" in raw:
                entry["metric_index"] = raw["metric_index"]
            np.savez(os.path.join(tmp, "entry.npz"), **entry)
            D.entries, D.cache, D.cache_size = [os.path.join(tmp, "entry.npz")], {}, 0
        D.base_dir, D.data_augmentation, D.config, D.rot_factor, D.augment_noise = tmp, aug, cfg, 1.0, noise
        D.max_points, D.overlap_radius = max_points, R.OVERLAP_RADIUS
        np.random.seed(seed)
        with Recorder() as rec:
            item = D.__getitem__(0)
        draws = draws_of(rec.calls, ns, nt, max_points, aug)
        if aug and (draws["coin"] > 0.5) != want_src:
            continue
        src, tgt, rot, trans = item[0], item[1], item[5], item[6]
        if kind == "3dmatch" and R.near_radius(np.asarray(src, np.float64), np.asarray(tgt, np.float64), rot, trans, R.OVERLAP_RADIUS):
            continue
        out = {"seed": np.array([seed]), "in_src": raw["src"], "in_tgt": raw["tgt"], "in_rot": raw["rot"], "in_trans": raw["trans"],
               "out_src": np.asarray(src), "out_tgt": np.asarray(tgt), "out_src_feats": item[2], "out_tgt_feats": item[3],
               "out_corr": np.asarray(item[4]).astype(np.int64).reshape(-1, 2), "out_rot": rot, "out_trans": trans}
        assert rot.dtype == np.float32 and trans.dtype == np.float32 and trans.shape == (3, 1)
        if kind == "4dmatch":
            out["in_flow"], out["in_corr"], out["out_flow"] = raw["flow"], raw["correspondences"], np.asarray(item[7])
            if item[8] is not None:
                out["in_metric_index"], out["out_metric_index"] = raw["metric_index"], np.asarray(item[8])
        else:
            assert item[7] is None
        for name, v in draws.items():
            out["draw_" + name] = np.asarray(v)
        print("%s case %d seed %d: src %s %s, tgt %s %s, %d correspondences" % (kind, k, seed, out["out_src"].shape, out["out_src"].dtype,
                                                                               out["out_tgt"].shape, out["out_tgt"].dtype, len(out["out_corr"])))
        return out
    raise SystemExit("%s case %d: no seed passes the screening" % (kind, k))


def main(ref_root):
    m3, m4 = reference_datasets(ref_root)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for kind, mod, cases in (("3dmatch", m3, R.CASES_3D), ("4dmatch", m4, R.CASES_4D)):
            for k in range(len(cases)):
                for name, v in run_case(kind, k, mod, tmp).items():
                    out["%s_%d_%s" % (kind, k, name)] = v
    path = os.path.join(GOLDEN, "item3d.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
