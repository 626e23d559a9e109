"""Mint the fixture of the furthest-point sampling entries by RUNNING THE REFERENCE (needs the Diff-Reg checkout; CPU only):

    python tools/golden/make_golden_fps.py REFERENCE_ROOT     # the directory holding Diff-Reg-2d3d/; writes tests/golden/fps.npz

Two reference programs produce the index lists:
  * native_furthest_point_sample (vision3d/array_ops/furthest_point_sample.py:22-66), imported with vision3d.ext replaced by a MagicMock as the
    other minting scripts do (load_ext would build the extension).  It compares `distance < min_distance`, so "no min_distance" is passed as
    -1.0, which is what the module's own wrapper passes to the extension (:14-15).
  * sample_nodes_with_fps itself (vision3d/csrc/cpu/node_sampling/node_sampling.cpp:10-78), when pybind11 and a C++ compiler are present: the
    file is compiled from where it lies into a temporary directory, behind two stand-in helper headers and a three-line module definition
    written here, and the directory is removed afterwards.  Nothing compiled from the reference is kept.
Where both run their lists must agree, scene by scene; `programs` in the npz says which ran.

Screen (on the CPU, with tests/fps_ref.nodes, whose lists must equal the reference's as well): at every selection the winner's distance exceeds
the runner-up's by a relative 1e-5, and no iteration's best distance lies within a relative 1e-5 of min_distance -- so neither the order of the
float32 operations inside a norm nor a tie rule can change a list.  A scene that fails is reseeded (seed + 1) until it passes; points, lists
and the smallest margins found are stored."""
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile
from unittest.mock import MagicMock

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "diff-reg_amd"))

BINDING = """
#include "node_sampling.cpp"
PYBIND11_MODULE(ref_node_sampling, m) { m.def("sample_nodes_with_fps", &vision3d::sample_nodes_with_fps); }
"""
HELPER = "#pragma once\n#include <pybind11/numpy.h>\n#include <pybind11/pybind11.h>\nnamespace py = pybind11;\n"


def build_cpp(base):
    """-> (module, tmpdir) or (None, None) when it does not build here"""
    try:
        import pybind11
    except ImportError:
        return None, None
    tmp = tempfile.mkdtemp(prefix="ref_fps_")
    try:
        for name in ("numpy_helper.h", "torch_helper.h"):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(HELPER)
        with open(os.path.join(tmp, "binding.cpp"), "w") as f:
            f.write(BINDING)
        so = os.path.join(tmp, "ref_node_sampling" + sysconfig.get_config_var("EXT_SUFFIX"))
        src = os.path.join(base, "vision3d", "csrc", "cpu", "node_sampling")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I", tmp, "-I", src,
                               "-I", pybind11.get_include(), "-I", sysconfig.get_paths()["include"], os.path.join(tmp, "binding.cpp"),
                               "-o", so])
        sys.path.insert(0, tmp)
        import ref_node_sampling
        return ref_node_sampling, tmp
    except Exception as e:          # no compiler, no headers: the numpy program alone mints
        print("sample_nodes_with_fps did not build here (%s): minting from native_furthest_point_sample alone" % e)
        shutil.rmtree(tmp, ignore_errors=True)
        return None, None


def main(ref_root):
    for m in ("vision3d.ext", "ipdb", "open3d", "cv2", "easydict", "pykeops", "pykeops.torch", "pytorch3d", "pytorch3d.ops"):
        sys.modules[m] = MagicMock()
    base = os.path.join(ref_root, "Diff-Reg-2d3d")
    sys.path.insert(0, base)
    import importlib.util
    misc = MagicMock()
    sys.modules.setdefault("vision3d", MagicMock())
    sys.modules.setdefault("vision3d.utils", MagicMock())
    sys.modules["vision3d.utils.misc"] = misc                 # load_ext -> a MagicMock extension; only the numpy function is used
    spec = importlib.util.spec_from_file_location("ref_array_fps", os.path.join(base, "vision3d", "array_ops", "furthest_point_sample.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    cpp, tmp = build_cpp(base)
    from tests import fps_ref as F

    out, programs = {}, ["native_furthest_point_sample"] + (["sample_nodes_with_fps"] if cpp is not None else [])
    try:
        for name, n, kind, md, ns in F.SCENES:
            seed = 100 + 10 * len(out)
            while True:
                pts = F.scene_points(n, kind, seed)
                margins = []
                idx, dist, status = F.nodes(pts, md, ns, margins=margins)
                assert status == 0
                if name == F.STOPPED_BY_MIN_DISTANCE_WITH_BOTH_RULES:       # one scene with both rules where min_distance is the one that stops
                    assert md is not None and ns is not None and 1 < len(idx) < ns, (name, len(idx), ns)
                win = min((b / max(r, 1e-30) - 1.0 for b, r in margins if r > 0 and (md is None or b >= md)), default=np.inf)
                stop = min((abs(b / md - 1.0) for b, _ in margins), default=np.inf) if md is not None else np.inf
                if win > 1e-5 and stop > 1e-5:
                    break
                print("%s: seed %d fails the screen (winner margin %.2e, stop margin %.2e), reseeding" % (name, seed, win, stop))
                seed += 1
            native = np.asarray(ref.native_furthest_point_sample(pts, -1.0 if md is None else md, ns), dtype=np.int64)
            assert np.array_equal(native, idx), (name, "the statement differs from native_furthest_point_sample")
            if cpp is not None:
                got = np.asarray(cpp.sample_nodes_with_fps(pts, -1.0 if md is None else md, -1 if ns is None else ns), dtype=np.int64)
                assert np.array_equal(got, native), (name, "sample_nodes_with_fps and native_furthest_point_sample disagree")
            out[name + "/points"], out[name + "/indices"], out[name + "/distances"] = pts, native, dist
            out[name + "/margins"] = np.asarray([win, stop], np.float64)
            out[name + "/seed"] = np.asarray(seed)
            print("%-12s n %5d  nodes %4d  winner margin %.2e  stop margin %.2e  seed %d" % (name, n, len(native), win, stop, seed))
    finally:
        if tmp is not None:
            shutil.rmtree(tmp, ignore_errors=True)
    out["programs"] = np.asarray(programs)
    path = os.path.join(GOLDEN, "fps.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes); minted by %s" % (path, os.path.getsize(path), " and ".join(programs)))


if __name__ == "__main__":
    main(sys.argv[1])
