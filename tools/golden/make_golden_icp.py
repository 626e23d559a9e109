"""Writes tests/golden/icp.npz, the fixture of the point-to-point ICP tests.

The reference function (multi_scale_icp, vision3d/utils/open3d.py:378-396) calls Open3D only, and Open3D is installed on no machine of this
project.  So the fixture does NOT hold outputs of the reference: it holds the outputs of the float64 statement of the published loop
(tests/icp_ref.py) and, per tensor, the deviation of the float32 statement from them.  Parity with Open3D itself is not claimed.

Every scene is screened on the CPU and reseeded until it passes (tests/icp_ref.py: screens): over every evaluation of the float64 run the gap
between a row's nearest and second-nearest d2 is an exact tie or at least 1e-5 relative, no nearest d2 lies within 1e-5 of the threshold, in the
convergence scenes every |delta rmse| and |delta fitness| is below 1e-7 or above 1e-5, and in the two-scale scene no coordinate lies within
1e-5 voxels of a voxel wall.  The float32 statement must then give the float64 statement's correspondences and iteration counts.

    python tools/golden/make_golden_icp.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import icp_ref as R  # noqa: E402


def stack(traces, key, dtype):
    """[evaluation, pair, ...] of a fixed-iteration scene"""
    return np.array([[np.asarray(tr[k][key], dtype) for tr in traces] for k in range(len(traces[0]))])


def build(spec, first_seed):
    seed = first_seed
    while True:
        sc = R.make_scene(spec, seed)
        m, res64, tr64 = R.screens(sc)
        tr32 = []
        res32 = R.run(sc, np.float32, tr32)
        same = m["ok"]
        if same and sc["kind"] == "scales":
            same = all(np.array_equal(a["evals"][k]["corr"], b["evals"][k]["corr"]) and len(a["src"]) == len(b["src"])
                       for x, y in zip(tr64, tr32) for a, b in zip(x, y) for k in range(len(a["evals"])))
        elif same:
            same = all(len(x) == len(y) and all(np.array_equal(a["corr"], b["corr"]) for a, b in zip(x, y)) for x, y in zip(tr64, tr32))
            same = same and all(a["status"] == b["status"] == 0 for a, b in zip(res64, res32))
        if same:
            break
        seed += 1000
    name = sc["name"]
    out = {name + "/in_" + k: sc[k] for k in ("src", "tgt", "s_off", "t_off", "init", "gt")}
    out[name + "/seed"] = seed
    out[name + "/screens"] = np.array([m["gap"], m["edge"], m["wall"]])
    dev = lambda a, b: float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
    if sc["kind"] == "fixed":
        for key, k2 in (("T", "transform"), ("fitness", "fitness"), ("rmse", "rmse")):
            a, b = stack(tr64, key, np.float64), stack(tr32, key, np.float64)
            out["%s/%s" % (name, k2)] = a
            out["%s/dev_%s" % (name, k2)] = dev(a, b)
        out[name + "/corr"] = np.array([np.concatenate([tr[k]["corr"] for tr in tr64]) for k in range(len(tr64[0]))]).astype(np.int16)
    elif sc["kind"] == "converge":
        for key in ("transform", "fitness", "rmse"):
            a, b = np.array([r[key] for r in res64], np.float64), np.array([r[key] for r in res32], np.float64)
            out["%s/%s" % (name, key)] = a
            out["%s/dev_%s" % (name, key)] = dev(a, b)
        out[name + "/iterations"] = np.array([r["iterations"] for r in res64], np.int32)
        out[name + "/corr"] = np.concatenate([r["corr"] for r in res64]).astype(np.int16)
    else:
        a, b = np.array([s["T"] for s in tr64[0]]), np.array([s["T"] for s in tr32[0]], np.float64)
        out[name + "/transform"] = a                          # after every scale
        out[name + "/dev_transform"] = dev(a, b)
        for i, s in enumerate(tr64[0]):
            out["%s/scale%d_src" % (name, i)] = s["src"]
            out["%s/scale%d_tgt" % (name, i)] = s["tgt"]
            out["%s/dev_scale%d" % (name, i)] = max(dev(s["src"], tr32[0][i]["src"]), dev(s["tgt"], tr32[0][i]["tgt"]))
    print("%-16s seed %6d  gap %.2e  edge %.2e  wall %.2e" % (name, seed, m["gap"], m["edge"], m["wall"]), flush=True)
    return out


def main():
    data = {"provenance": np.array("float64 statement of the published point-to-point ICP loop (tests/icp_ref.py); dev_* = the float32 "
                                   "statement's largest deviation from it; no Open3D output: parity with Open3D itself is not claimed")}
    for i, spec in enumerate(R.SCENES):
        data.update(build(spec, 100 + i))
    path = os.path.join(ROOT, "tests", "golden", "icp.npz")
    np.savez_compressed(path, **data)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
