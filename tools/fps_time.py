"""Time the device furthest-point sampling (dr_fps_nodes_f32) against the same loop in plain PyTorch-ROCm float32 on the same GPU and against
the reference's host procedure.

    python tools/fps_time.py [--runs 30] [--host-runs 3] [--out profiles/fps_time.jsonl]

Cases: 9 000 points -> 512 nodes (the on-chip form), 30 000 points -> 800 nodes (above dr_fps_onchip_capacity(): the streaming form), and 8
clouds of 9 000 points in one call.  The clouds are 4DMatch-like sheets (tests/fps_ref.scene_points); only num_samples stops the loop, so every
path does the same number of iterations.
  (a) device:  nonrigid.fps_nodes into preallocated buffers;
  (b) torch:   ONE loop over all the clouds of the call, batched [P, n, 3]: per iteration one index (a gather by a [P, 1] DEVICE index
               tensor), one distance + min, one argmax over dim 1.  The index stays a 1-column tensor throughout: indexing by a 0-dim
               tensor would read it back to the host each iteration.  Nothing is read back inside the loop.  For P > 1 the P single-cloud
               loops run one after the other are timed as well (torch_sequential_ms);
  (c) host:    the numpy statement of the reference's loop (tests/fps_ref.nodes), --host-runs runs only.
Median of --runs alternated runs with p10-p90 on a device-synchronised host clock, and microseconds per iteration of (a) and (b).

Then the device entry alone at 1 024 s points -> 512 nodes for s = 1, 2, 4, 9, 12 slots per lane (every compiled slot count of the on-chip
form): the least-squares line through (s, microseconds per iteration) gives the per-slot cost of the distance update (slope) and what an
iteration costs beside it -- the wave reduction, the LDS exchange and the barrier (intercept): the floor of this design.  Reads nothing
outside the repository."""
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
from tests import fps_ref as F  # noqa: E402

DEV = "cuda:0"
CASES = ((1, 9000, 512), (1, 30000, 800), (8, 9000, 512))
SWEEP_SLOTS, SWEEP_NODES = (1, 2, 4, 9, 12), 512


def torch_fps(pts, m):
    """pts [B, N, 3] -> indices [B, m]; no host read inside the loop"""
    B, N = pts.shape[0], pts.shape[1]
    d = torch.full((B, N), float("inf"), device=pts.device)
    out = torch.zeros(B, m, dtype=torch.int64, device=pts.device)
    last = out[:, :1]
    for k in range(1, m):
        cur = torch.gather(pts, 1, last[:, :, None].expand(B, 1, 3))
        d = torch.minimum(d, (pts - cur).pow(2).sum(2).sqrt())
        last = torch.argmax(d, dim=1, keepdim=True)
        out[:, k:k + 1] = last
    return out


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return dict(median=float(np.median(xs)), p10=float(np.percentile(xs, 10)), p90=float(np.percentile(xs, 90)))


def measure(P, n, m, runs, host_runs):
    host = [F.scene_points(n, "surface", 900 + p) for p in range(P)]
    clouds = [torch.from_numpy(h).to(DEV) for h in host]
    pts = torch.cat(clouds)
    stacked = torch.stack(clouds)
    buf = nr.fps_nodes(pts, num_samples=m, lengths=[n] * P)
    device = lambda: nr.fps_nodes(pts, num_samples=m, lengths=[n] * P, out=buf)["indices"]
    plain = lambda: torch_fps(stacked, m)
    sequential = lambda: torch.cat([torch_fps(c[None], m) for c in clouds])
    device(); torch_fps(stacked, 4)
    t_dev, t_tor, t_seq = [], [], []
    for _ in range(runs):
        ms, i_dev = clock(device); t_dev.append(ms)
        ms, i_tor = clock(plain); t_tor.append(ms)
        if P > 1:
            ms, i_seq = clock(sequential); t_seq.append(ms)
    t_host = []
    for _ in range(host_runs):
        t0 = time.perf_counter()
        i_host = [F.nodes(h, None, m)[0] for h in host]
        t_host.append((time.perf_counter() - t0) * 1e3)
    iters = m - 1
    return dict(clouds=P, points=n, nodes=m, form="on-chip" if n <= nr.fps_onchip_capacity() else "streaming", runs=runs, device_ms=stats(t_dev),
                torch_ms=stats(t_tor), torch_loop="one batched loop over the %d cloud%s, no host read" % (P, "s" if P > 1 else ""),
                torch_sequential_ms=stats(t_seq) if t_seq else None, host_ms=stats(t_host) if t_host else None,
                device_us_per_iteration=float(np.median(t_dev)) * 1e3 / iters, torch_us_per_iteration=float(np.median(t_tor)) * 1e3 / iters,
                speedup_median=float(np.median(t_tor) / np.median(t_dev)),
                device_equals_host=bool(host_runs and all(np.array_equal(i_dev[p].cpu().numpy(), i_host[p]) for p in range(P))),
                device_equals_torch=bool(torch.equal(i_dev, i_tor)))


def sweep(runs):
    """the device entry alone over the slot counts of the on-chip form -> per-slot cost and the rest of an iteration"""
    us = []
    for s in SWEEP_SLOTS:
        n = s * F.BLOCK
        pts = torch.from_numpy(F.scene_points(n, "surface", 950 + s)).to(DEV)
        buf = nr.fps_nodes(pts, num_samples=SWEEP_NODES)
        device = lambda: nr.fps_nodes(pts, num_samples=SWEEP_NODES, out=buf)["indices"]
        device()
        us.append(float(np.median([clock(device)[0] for _ in range(runs)])) * 1e3 / (SWEEP_NODES - 1))
    slope, intercept = np.polyfit(np.asarray(SWEEP_SLOTS, np.float64), np.asarray(us), 1)
    return dict(sweep="slots per lane", nodes=SWEEP_NODES, runs=runs, slots=list(SWEEP_SLOTS), points=[s * F.BLOCK for s in SWEEP_SLOTS],
                device_us_per_iteration=us, us_per_slot=float(slope), us_per_iteration_beside_the_slots=float(intercept))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps_time.jsonl"))
    a = ap.parse_args()
    with open(a.out, "w") as f:
        for P, n, m in CASES:
            rec = dict(tool="fps_time", device=torch.cuda.get_device_name(0), **measure(P, n, m, a.runs, a.host_runs))
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")
            f.flush()
        rec = dict(tool="fps_time", device=torch.cuda.get_device_name(0), **sweep(a.runs))
        print(json.dumps(rec))
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
