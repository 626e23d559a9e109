"""CPU check of the size queries whose layouts moved to one carve per workspace (csrc/carve.h): over the argument table of
tools/golden/make_golden_workspace_sizes.py every query answers what tests/golden/workspace_sizes.json records from the build before the move.
Three layouts did not start every array on a 256-byte boundary before; the Carver does, so their answer may grow by less than 256 bytes per
array and may never shrink."""
import importlib.util
import json
import os

import pytest

from tests.conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_golden_workspace_sizes",
                                               os.path.join(ROOT, "tools", "golden", "make_golden_workspace_sizes.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

# arrays of the layouts that were not 256-byte aligned throughout
GROWS = {"dr_ransac_workspace_bytes": 2, "dr_pnp_ransac_workspace_bytes": 2, "dr_mutual_topk_workspace_bytes": 2}


@pytest.fixture(scope="module")
def sizes():
    assert os.path.exists(gen.DEFAULT_LIB), "build first: python __graft_entry__.py build"
    return gen.query_all(gen.DEFAULT_LIB)


@pytest.fixture(scope="module")
def golden():
    with open(gen.OUT) as f:
        return json.load(f)


def test_table_is_the_recorded_one(golden):
    assert sorted(golden) == sorted(gen.TABLE)
    for name, (_, rows) in gen.TABLE.items():
        assert [r[0] for r in golden[name]] == [list(r) for r in rows], name


@pytest.mark.parametrize("name", sorted(gen.TABLE))
def test_size_query_matches_parent(name, sizes, golden):
    assert len(sizes[name]) == len(golden[name]) > 0
    for (args, new), (gargs, parent) in zip(sizes[name], golden[name]):
        assert args == gargs
        if name in GROWS:
            assert parent <= new < parent + 256 * GROWS[name], (name, args, parent, new)
            assert (parent == 0) == (new == 0), (name, args, parent, new)
        else:
            assert new == parent, (name, args, parent, new)


def test_carve_walk_ends_clean_under_sanitizers(tmp_path):
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for tools/carve_check.cpp"
    exe = str(tmp_path / "carve_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "diff-reg_amd", "csrc"), os.path.join(ROOT, "tools", "carve_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "regions ok" in r.stdout, r.stdout + r.stderr
