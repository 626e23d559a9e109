"""Time the device geodesic deformation graph (dr_geo_graph_f32) against host statements of the same procedure.

    python tools/geo_graph_time.py [--runs 30] [--host-runs 1] [--out profiles/geo_graph_time.jsonl]

Cases: one cloud of 9 000 points -> 512 nodes, Kn = 8, Ka = 6, and 8 such clouds in one call.  The clouds are gently curved sheets of side 1
(point spacing about 0.0105), max_distance = 0.03 (about 25 neighbours per point), node_coverage = 0.06; the nodes come from the device's
furthest-point sampling (num_samples = 512) and are not timed.
  (a) device: nonrigid.geo_graph into preallocated buffers (all four launches; nothing is read back);
  (b) host:   tests/geo_graph_ref.geo_graph(form="heap"), the numpy / heapq statement of the reference's loop, --host-runs runs of ONE cloud;
  (c) scipy:  when scipy is importable, scipy.sparse.csgraph.dijkstra(indices=nodes, limit=2 c) over the same edges: the path lengths only, in
              float64, without the two selections -- a lower bound of a compiled host Dijkstra, not the reference's program (its own C++ is not
              on the GPU machine, so its time is not claimed).
Median of --runs device runs with p10-p90 on a device-synchronised host clock.  device_equals_host compares the index tables of the first
cloud (the scenes are not screened for ties, so it is reported, not asserted).  Reads nothing outside the repository."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
from diffreg_hip import nonrigid as nr  # noqa: E402
from tests import geo_graph_ref as R  # noqa: E402

DEV = "cuda:0"
CASES = ((1, 9000, 512), (8, 9000, 512))
KN, KA, MAXD, COV = 8, 6, 0.03, 0.06


def cloud(n, seed):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(0, 1.0, (n, 2))
    return np.stack([uv[:, 0], uv[:, 1], 0.05 * np.sin(uv[:, 0] * 9) * np.cos(uv[:, 1] * 7)], 1).astype(np.float32)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return dict(median=float(np.median(xs)), p10=float(np.percentile(xs, 10)), p90=float(np.percentile(xs, 90)))


def scipy_reach(pts, nodes):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    src, dst, length = R.edges(pts, np.float32(MAXD))
    t0 = time.perf_counter()
    g = csr_matrix((length.astype(np.float64), (src, dst)), shape=(len(pts), len(pts)))
    dijkstra(g, directed=True, indices=nodes, limit=2.0 * float(np.float32(COV)))
    return (time.perf_counter() - t0) * 1e3


def measure(P, n, m, runs, host_runs):
    host = [cloud(n, 700 + p) for p in range(P)]
    pts = torch.cat([torch.from_numpy(h).to(DEV) for h in host])
    f = nr.fps_nodes(pts, num_samples=m, lengths=[n] * P)
    assert f["counts"].tolist() == [m] * P
    idx = f["indices"].reshape(-1).contiguous()
    buf = nr.geo_graph(pts, idx, KN, KA, MAXD, COV, point_lengths=[n] * P, node_lengths=[m] * P)
    device = lambda: nr.geo_graph(pts, idx, KN, KA, MAXD, COV, point_lengths=[n] * P, node_lengths=[m] * P, out=buf)
    device()
    t_dev = [clock(device)[0] for _ in range(runs)]
    out = device()
    status = out["status"].tolist()
    nodes0 = idx[:m].cpu().numpy()
    t_host, t_scipy, same = [], [], None
    for _ in range(host_runs):
        t0 = time.perf_counter()
        want = R.geo_graph(host[0], nodes0, KN, KA, np.float32(MAXD), np.float32(COV), form="heap")
        t_host.append((time.perf_counter() - t0) * 1e3)
        same = bool(np.array_equal(out["anchor_indices"][:n].cpu().numpy(), want["anchor_indices"]) and
                    np.array_equal(out["neighbor_indices"][:m].cpu().numpy(), want["neighbor_indices"]) and
                    np.array_equal(out["anchor_distances"][:n].cpu().numpy(), want["anchor_distances"]))
        try:
            t_scipy.append(scipy_reach(host[0], nodes0))
        except ImportError:
            pass
    reached = float((out["anchor_indices"][:, 0] >= 0).float().mean())
    return dict(clouds=P, points=n, nodes=m, num_neighbors=KN, num_anchors=KA, max_distance=MAXD, node_coverage=COV, runs=runs,
                form="on-chip" if n <= nr.geo_graph_onchip_capacity() else "streamed", status=status, points_reached=reached,
                device_ms=stats(t_dev), host_one_cloud_ms=stats(t_host) if t_host else None,
                scipy_dijkstra_one_cloud_ms=stats(t_scipy) if t_scipy else None, device_equals_host=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host-runs", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geo_graph_time.jsonl"))
    a = ap.parse_args()
    with open(a.out, "w") as f:
        for k, (P, n, m) in enumerate(CASES):
            rec = dict(tool="geo_graph_time", device=torch.cuda.get_device_name(0), **measure(P, n, m, a.runs, a.host_runs if k == 0 else 0))
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")
            f.flush()


if __name__ == "__main__":
    main()
