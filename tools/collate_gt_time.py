"""Time the ground-truth entries of the 3D / 4D training collate on one GPU against their numpy statement on the host.

    python tools/collate_gt_time.py [--runs 30] [--warmup 3] [--out FILE.json]

Two single pairs (P = 1, the latency case), hash-drawn:
  3dmatch   coarse clouds of 700 x 650 points: dr_coarse_gt_matches_f32                                   vs  tests/collate_gt_ref.coarse_gt_matches
  4dmatch   600 x 640 coarse points, a raw source cloud of 9 000 points with its flow: dr_blend_flow_knn3_f32, then dr_coarse_gt_matches_f32 on
            the moved sources                                                                            vs  blend_flow_knn3 + coarse_gt_matches
The device path is timed from the library calls to the end of the one host read of (counts, status) that the collate makes; its inputs already
lie on the device, the host path's on the host.  The two paths are alternated, 30 runs after warm-up, device-synchronised host clock; median and
p10 - p90.  The host statement is numpy in float32 (what the reference's utils.py does, without its [M, N, 3] repeat copies), single process.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffreg_hip import lib, synth  # noqa: E402
from tests import collate_gt_ref as cg  # noqa: E402


def scene(seed, ns, nt, n_raw):
    R = synth._rodrigues(np.array([0.2, 0.1, 1.0]), 0.3).astype(np.float32)
    t = np.array([0.1, -0.05, 0.02], np.float32)
    src = synth.hash_uniform(seed, 1, (ns, 3), 0.0, 2.0).astype(np.float32)
    flow = (0.03 * synth.hash_normal(seed, 2, (ns, 3))).astype(np.float32)
    tgt = np.concatenate([cg.warp(src[:nt // 2], R, t, flow[:nt // 2] if n_raw else None, np.float64) + 0.01 * synth.hash_normal(seed, 3, (nt // 2, 3)),
                          synth.hash_uniform(seed, 4, (nt - nt // 2, 3), 0.0, 2.0)]).astype(np.float32)
    raw = raw_flow = None
    if n_raw:
        raw = np.concatenate([src, synth.hash_uniform(seed, 5, (n_raw - ns, 3), 0.0, 2.0).astype(np.float32)])
        raw_flow = (0.03 * synth.hash_normal(seed, 6, (n_raw, 3))).astype(np.float32)
    return dict(src=src, tgt=tgt, rot=R, trn=t, raw=raw, raw_flow=raw_flow)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("collate_gt_time: needs a GPU (a CPU run says nothing about the device)")
    dev = "cuda:0"
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    off = lambda n: torch.tensor([0, n], dtype=torch.int32, device=dev)
    radius = 0.1
    res = {"tool": "collate_gt_time", "runs": a.runs, "radius": radius}
    for name, (ns, nt, n_raw) in (("3dmatch", (700, 650, 0)), ("4dmatch", (600, 640, 9000))):
        sc = scene(17, ns, nt, n_raw)
        d = {k: T(v) for k, v in sc.items() if v is not None}
        so, to, ro = off(ns), off(nt), off(n_raw)
        rot, trn = d["rot"][None].contiguous(), d["trn"][None].contiguous()

        def run_device():
            flow = None
            words = []
            if n_raw:
                flow, bst = lib.blend_flow_knn3(d["src"], so, d["raw"], d["raw_flow"], ro)
                words.append(bst)
            o_s, o_t, cnt, st = lib.coarse_gt_matches(d["src"], so, d["tgt"], to, rot, trn, radius, src_flow=flow)
            host = torch.cat([cnt, st] + words).cpu()
            return o_s, o_t, int(host[0]), flow

        def run_host():
            flow = cg.blend_flow_knn3(sc["src"], sc["raw"], sc["raw_flow"]) if n_raw else None
            return cg.coarse_gt_matches(sc["src"], sc["tgt"], sc["rot"], sc["trn"], radius, flow), flow

        paths = (("host_numpy", run_host), ("device", run_device))
        for _ in range(a.warmup):
            for _, fn in paths:
                fn()
        torch.cuda.synchronize()
        t = {p: [] for p, _ in paths}
        for _ in range(a.runs):
            for p, fn in paths:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[p].append((time.perf_counter() - t0) * 1e3)
        o_s, o_t, c, flow = run_device()
        want, hflow = run_host()
        entry = {"n_src": ns, "n_tgt": nt, "n_raw": n_raw, "matches": c,
                 "matches_equal_host": bool(np.array_equal(torch.stack([o_s[:c], o_t[:c]]).cpu().numpy(), want))}
        if n_raw:
            entry["flow_max_abs_diff_vs_host"] = float(np.abs(flow.cpu().numpy() - hflow).max())
        for p, v in t.items():
            v = np.array(v)
            entry[p + "_ms"] = {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90))}
        res[name] = entry
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
