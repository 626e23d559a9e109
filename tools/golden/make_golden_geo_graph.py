"""Mint the fixture of the geodesic deformation graph by RUNNING THE REFERENCE (needs the Diff-Reg checkout, pybind11 and a C++ compiler; CPU only):

    python tools/golden/make_golden_geo_graph.py REFERENCE_ROOT     # the directory holding Diff-Reg-2d3d/; writes tests/golden/geo_graph.npz

build_deformation_graph_from_point_cloud (vision3d/csrc/cpu/deformation_graph/deformation_graph.cpp:13-265) and voxel.cpp are compiled from
where they lie into a temporary directory, with -ffp-contract=off, behind two stand-in helper headers and a three-line module definition
written here; the directory is removed afterwards.  Nothing compiled from the reference is kept.

Screen (on the CPU, with tests/geo_graph_ref.py, whose two forms must equal the reference's arrays as well): no pair distance within a relative
1e-5 of max_distance, no path length within 1e-5 of 2 node_coverage, no two consecutive entries of a sorted reach list through position K + 1
within 1e-5 of each other (the node's own 0 excepted) -- so no tie rule and no rounding at a bound can change a list.  One stated difference:
the reference writes the r-th REACHED point's anchors into row r (point_rows below); the fixture holds each list in its own point's row.  A scene that fails is
reseeded (seed + 1) until it passes.  Stored per scene: the inputs, the six arrays, the three margins, and the largest deviation of the
reference's float32 weights from the same formula evaluated in float64 on the reference's distances (neighbours, anchors): the GPU tests'
weight bar is 4 x that, or one float32 ulp."""
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

BINDING = """
#include "deformation_graph.cpp"
#include "../voxel/voxel.cpp"
PYBIND11_MODULE(ref_deformation_graph, m) {
  m.def("build_deformation_graph_from_point_cloud", &vision3d::build_deformation_graph_from_point_cloud);
}
"""
HELPER = "#pragma once\n#include <pybind11/numpy.h>\n#include <pybind11/pybind11.h>\n#include <pybind11/stl.h>\nnamespace py = pybind11;\n"


def build_cpp(base):
    import pybind11
    tmp = tempfile.mkdtemp(prefix="ref_geo_")
    try:
        for name in ("numpy_helper.h", "torch_helper.h"):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(HELPER)
        with open(os.path.join(tmp, "binding.cpp"), "w") as f:
            f.write(BINDING)
        so = os.path.join(tmp, "ref_deformation_graph" + sysconfig.get_config_var("EXT_SUFFIX"))
        src = os.path.join(base, "vision3d", "csrc", "cpu", "deformation_graph")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I", tmp, "-I", src,
                               "-I", pybind11.get_include(), "-I", sysconfig.get_paths()["include"], os.path.join(tmp, "binding.cpp"),
                               "-o", so])
        sys.path.insert(0, tmp)
        import ref_deformation_graph
        return ref_deformation_graph, tmp
    except Exception:
        shutil.rmtree(tmp, ignore_errors=True)
        raise


def point_rows(ref, reached, name):
    """The reference advances its anchor row only behind a point that HAS anchors (.cpp:149, :178): the r-th reached point's list lands in row r,
    whatever the point's index, and the rows behind the last reached point stay padding.  The lists are the reference's; here they are moved to
    the rows of the points they belong to (`reached`: the points some node reaches, by the statement), which is what the device returns."""
    r = int(reached.sum())
    assert np.all(ref["anchor_indices"][:r, 0] >= 0) and np.all(ref["anchor_indices"][r:] == -1), (name, "reached sets differ")
    for key in ("anchor_indices", "anchor_distances", "anchor_weights"):
        full = np.full_like(ref[key], -1 if "indices" in key else 0)
        full[reached] = ref[key][:r]
        ref[key] = full
    return ref


def weight_deviation(R, ref, c):
    """largest |reference float32 weight - float64 formula on the reference's distances|: (neighbours, anchors)"""
    nw = np.where(ref["neighbor_indices"] >= 0, R.weight_f64(ref["neighbor_distances"], c), 0.0)
    aw = np.where(ref["anchor_indices"] >= 0, R.weight_f64(ref["anchor_distances"], c), 0.0)
    s = aw.sum(1, keepdims=True)
    aw = np.divide(aw, s, out=np.zeros_like(aw), where=s > 0)
    return np.asarray([np.abs(ref["neighbor_weights"].astype(np.float64) - nw).max(initial=0.0),
                       np.abs(ref["anchor_weights"].astype(np.float64) - aw).max(initial=0.0)], np.float64)


def main(ref_root):
    from tests import geo_graph_ref as R
    cpp, tmp = build_cpp(os.path.join(ref_root, "Diff-Reg-2d3d"))
    out = {}
    try:
        for k, s in enumerate(R.SCENES):
            name, seed = s[0], 500 + 10 * k
            while True:
                pts, nodes, Kn, Ka, maxd, c = R.scene(name, seed)
                pair, bound, lst, G = R.screen(pts, nodes, Kn, Ka, maxd, c)
                if pair > 1e-5 and bound > 1e-5 and lst > 1e-5:
                    break
                print("%s: seed %d fails the screen (pair %.2e, bound %.2e, list %.2e), reseeding" % (name, seed, pair, bound, lst))
                seed += 1
            got = cpp.build_deformation_graph_from_point_cloud(pts, nodes, Kn, Ka, float(maxd), float(c))
            ref = {key: np.ascontiguousarray(a, np.int64 if "indices" in key else np.float32) for key, a in zip(R.KEYS, got)}
            ref = point_rows(ref, np.isfinite(G).any(0), name)
            for form in ("heap", "fixed_point"):
                mine = R.geo_graph(pts, nodes, Kn, Ka, maxd, c, form=form)
                for key in R.KEYS:
                    if "weights" in key:
                        assert np.abs(mine[key].astype(np.float64) - ref[key]).max(initial=0.0) <= 2.0 ** -23, (name, form, key)
                    else:
                        assert np.array_equal(mine[key], ref[key]), (name, form, key, "the statement differs from the reference")
            out[name + "/points"], out[name + "/node_indices"] = pts, nodes
            out[name + "/params"] = np.asarray([Kn, Ka, maxd, c], np.float64)
            for key in R.KEYS:
                out[name + "/" + key] = ref[key]
            out[name + "/margins"] = np.asarray([pair, bound, lst], np.float64)
            out[name + "/weight_dev"] = weight_deviation(R, ref, c)
            out[name + "/seed"] = np.asarray(seed)
            print("%-9s n %5d  nodes %4d  margins pair %.2e bound %.2e list %.2e  weight dev %.2e %.2e  seed %d"
                  % (name, len(pts), len(nodes), pair, bound, lst, *out[name + "/weight_dev"], seed))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(GOLDEN, "geo_graph.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1])
