"""Time the 3D / 4D dataset item on one GPU:

    python tools/item3d_time.py [--out FILE.jsonl] [--host-runs K] [--points N]

Method of tools/item2d3d_time.py: 5 warm-up runs, then 30 runs alternating the sides, each between two device synchronisations; median [p10-p90]
in milliseconds, the one host read of a batch included.  The scene is a room of three planes sampled on a jittered 0.025 m grid (what the 3DMatch
files hold after their voxel downsampling), 30 000 points a side, the target the moved source plus 5 mm of noise; overlap_radius 0.0375
(_3dmatch.py:38; the train yaml has no such key), augment_noise 0.005, batch_size 2 (configs/train/3dmatch.yaml).  Rows:

    pairs_one        the pair list of ONE pair: `ragged` = dr_radius_pairs_ragged_f32 (count call, host read, write call: the grid sweep),
                     `all_pairs` = dr_radius_pairs_f32 (every source row against every target, room for the counted list), and `ragged_one_call`
                     = the ragged entry's write call alone with the room known (what a caller with a capacity bound pays)
    item_3dmatch     prepare_batch of one raw item (clouds already on the device), draws from a device generator
    batch_3dmatch    prepare_batch of two
    item_4dmatch     prepare_batch(kind="4dmatch") of one raw item with a flow
    host             the reference's procedure on this machine's CPU: numpy for the augmentation and one KD-tree radius query per source point in
                     a Python loop, as KDTree_corr does -- with scipy's cKDTree in Open3D's place when scipy is importable (neither Open3D nor its
                     timing is claimed); fewer runs (--host-runs, default 2)

The three device pair lists are compared entry for entry before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
RADIUS, NOISE, SPACING = 0.0375, 0.005, 0.025


def measure(sides, warm=5, runs=30):
    out = {k: [] for k in sides}
    for i in range(warm + runs):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warm:
                out[k].append((time.perf_counter() - t0) * 1e3)
    return {k: dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), runs=len(v))
            for k, v in out.items()}


def make_scene(n, seed):
    """-> (src, tgt float32 [n, 3], rot [3, 3], trans [3] float64, flow float32 [n, 3])"""
    from tests.item3d_ref import euler_zyx
    rng = np.random.RandomState(seed)
    side = int(np.ceil(np.sqrt(n / 3.0)))
    u, v = np.meshgrid(np.arange(side), np.arange(side))
    uv = np.stack([u.ravel(), v.ravel()], 1) * SPACING
    planes = [np.stack([uv[:, 0], uv[:, 1], np.zeros(len(uv))], 1), np.stack([uv[:, 0], np.zeros(len(uv)), uv[:, 1] + SPACING], 1),
              np.stack([np.zeros(len(uv)), uv[:, 0] + SPACING, uv[:, 1] + SPACING], 1)]
    room = np.concatenate(planes)[rng.permutation(3 * side * side)[:n]] + rng.uniform(-0.3, 0.3, size=(n, 3)) * SPACING
    rot, trans = euler_zyx(rng.rand(3) * 2 * np.pi), rng.randn(3) * 0.5
    flow = (rng.randn(n, 3) * 0.01).astype(np.float32)
    tgt = room[rng.permutation(n)] + rng.randn(n, 3) * 0.005
    src = (room - trans) @ rot                                   # rot src + trans = room
    return src.astype(np.float32), tgt.astype(np.float32), rot, trans, flow


def host_item(src, tgt, rot, trans, rng):
    """_3dmatch.py:93-110 in numpy, the pair list by one radius query per source point (KDTree_corr's loop)"""
    from scipy.spatial import cKDTree
    from tests.item3d_ref import euler_zyx
    rot_ab = euler_zyx(rng.rand(3) * np.pi * 2)
    if rng.rand(1)[0] > 0.5:
        src = np.matmul(rot_ab, src.T).T
        rot = np.matmul(rot, rot_ab.T)
    else:
        tgt = np.matmul(rot_ab, tgt.T).T
        rot = np.matmul(rot_ab, rot)
        trans = np.matmul(rot_ab, trans)
    src = src + (rng.rand(src.shape[0], 3) - 0.5) * NOISE
    tgt = tgt + (rng.rand(tgt.shape[0], 3) - 0.5) * NOISE
    moved = src @ rot.T + trans
    tree = cKDTree(tgt)
    corr = []
    for i, point in enumerate(moved):
        for j in tree.query_ball_point(point, RADIUS):
            corr.append([i, j])
    return np.array(corr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "item3d_time.jsonl"))
    ap.add_argument("--host-runs", type=int, default=2)
    ap.add_argument("--points", type=int, default=30000)
    a = ap.parse_args()
    from diffreg_hip import item3d, lib
    from diffreg_hip.partition2d3d import radius_pairs_raw
    n = a.points
    t = lambda x, dt=None: torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dt is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dt)
    scenes = [make_scene(n, 3), make_scene(n, 4)]
    src, tgt, rot, trans, flow = scenes[0]
    s_, t_ = t(src), t(tgt)
    T44 = np.eye(4)
    T44[:3, :3], T44[:3, 3] = rot, trans
    T44d = t(T44, torch.float32)
    so = torch.tensor([0, n], dtype=torch.int32, device=DEV)
    tsfm = T44d[:3].reshape(1, 3, 4).contiguous()

    def ragged():
        return item3d.get_correspondences(s_, t_, T44d, RADIUS)

    ref = ragged()
    found = ref.shape[0]
    c_off = torch.tensor([0, found], dtype=torch.int64, device=DEV)

    def ragged_one_call():
        return lib.radius_pairs_ragged(s_, so, t_, so, tsfm, RADIUS, c_off, found)

    def all_pairs():
        i, j, counts = radius_pairs_raw(s_, t_, T44d, RADIUS, capacity=found)
        counts.tolist()
        return i, j

    i, j = all_pairs()
    o_src, o_tgt, _, _ = ragged_one_call()
    same = bool(torch.equal(ref[:, 0], i[:found]) and torch.equal(ref[:, 1], j[:found]) and torch.equal(ref[:, 0], o_src) and torch.equal(ref[:, 1], o_tgt))
    print("%d x %d points, %d pairs (%.1f per source row); the three device lists are equal: %s" % (n, n, found, found / n, same), flush=True)
    rows = []
    res = measure({"ragged": ragged, "all_pairs": all_pairs, "ragged_one_call": ragged_one_call})
    rows.append(dict(row="pairs_one", points=n, pairs=found, lists_equal=same, **res))
    print(rows[-1], flush=True)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    opt = dict(max_points=30000, data_augmentation=True, rot_factor=1.0, augment_noise=NOISE, overlap_radius=RADIUS, generator=gen, device=DEV)
    raw3 = [dict(src_pcd=t(s[0]), tgt_pcd=t(s[1]), rot=s[2], trans=s[3]) for s in scenes]
    raw4 = [dict(s_pc=t(s[0]), t_pc=t(s[1]), rot=s[2], trans=s[3], s2t_flow=t(s[4]), correspondences=np.zeros((1, 2), np.int64)) for s in scenes]
    res = measure({"device": lambda: item3d.prepare_batch(raw3[:1], kind="3dmatch", **opt)})
    rows.append(dict(row="item_3dmatch", points=n, **res))
    print(rows[-1], flush=True)
    res = measure({"device": lambda: item3d.prepare_batch(raw3, kind="3dmatch", **opt)})
    rows.append(dict(row="batch_3dmatch", points=n, pairs_in_batch=2, **res))
    print(rows[-1], flush=True)
    res = measure({"device": lambda: item3d.prepare_batch(raw4[:1], kind="4dmatch", **dict(opt, augment_noise=0.002))})
    rows.append(dict(row="item_4dmatch", points=n, **res))
    print(rows[-1], flush=True)
    try:
        import scipy.spatial  # noqa: F401
        rng = np.random.RandomState(9)
        res = measure({"host": lambda: host_item(src, tgt, rot, trans, rng)}, warm=0, runs=a.host_runs)
        rows.append(dict(row="host", points=n, kd_tree="scipy cKDTree, one query per source point", **res))
    except ImportError:
        rows.append(dict(row="host", note="scipy is not importable here: not measured"))
    print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
