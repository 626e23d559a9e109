"""tests/conv_plan.py against csrc/conv2d.hip, and the case table of tests/test_conv_forms_gpu.py against the (entry, form, arm) matrix.  No device.

 * the two dispatch constants are read out of the source's text: a retune fails here instead of silently moving every case of the table onto
   another kernel; the two comparisons of the dispatcher are held as text as well (<= for the depth, >= for the tile count);
 * every case of the table lands on the form it names;
 * every reachable cell of {Fwd/plain, Fwd/ACT, Bwd, Trans} x {S, M, L} x {vec, scalar} and Fwd/PROJECT x {S, M} x {vec, scalar} is reached by
   the table or by an earlier test named by file; the claims about earlier tests are held to the shape tables they are parametrised by;
 * both thresholds are straddled by a pair of cases that differ in one extent only.
The coverage table is printed (run with -s) and is the assertion message when a cell is empty."""
import os
import re

from tests import conv_plan as P
from tests.conftest import ROOT

SRC = os.path.join(ROOT, "diff-reg_amd", "csrc", "conv2d.hip")


def source():
    with open(SRC) as f:
        return f.read()


def table(cov):
    lines = []
    for cell in P.reachable_cells():
        who = cov[cell]
        before = [w for w in who if not w.startswith("test_conv_forms_gpu.py")]
        lines.append("%-12s %s %-6s %s %s" % (cell[0], cell[1], cell[2], "          " if before else "[new here]", ", ".join(who) or "NOBODY"))
    return "\n".join(lines)


def test_constants_are_the_sources():
    src = source()
    short_k = re.findall(r"constexpr\s+int\s+CV_SHORT_K\s*=\s*(\d+)\s*;", src)
    large = re.findall(r"constexpr\s+long\s+long\s+CV_LARGE_TILES\s*=\s*(\d+)\s*;", src)
    assert len(short_k) == 1 and len(large) == 1, (short_k, large)
    assert int(short_k[0]) == P.CV_SHORT_K, "CV_SHORT_K was retuned: move conv_plan.py and the cases at the threshold with it"
    assert int(large[0]) == P.CV_LARGE_TILES, "CV_LARGE_TILES was retuned: move conv_plan.py and the cases at the threshold with it"
    # the comparisons themselves: depth <= CV_SHORT_K takes S (both dispatchers), large >= CV_LARGE_TILES takes L, tiles are 128 x 128
    assert len(re.findall(r"depth\(A\.g\)\s*<=\s*CV_SHORT_K", src)) == 2
    assert len(re.findall(r"large\s*>=\s*CV_LARGE_TILES", src)) == 1
    assert re.search(r"large\s*=\s*\(long long\)\(\(MAP::rows\(A\.g\)\s*\+\s*127\)\s*/\s*128\)\s*\*\s*\(\(MAP::cols\(A\.g\)\s*\+\s*127\)\s*/\s*128\)", src)
    # the alignment test of the five entries: the two operand bases and the A leading dimension, nothing else
    assert len(re.findall(r"const bool vec = \(\(\(\(uintptr_t\)\w+\) \| \(\(uintptr_t\)\w+\)\) & 15u\) == 0 && ld\w+ % 4 == 0;", src)) == 5


def test_plan_at_its_edges():
    assert P.plan("Fwd", 1, 1, 1024) == "S" and P.plan("Fwd", 1 << 20, 1 << 10, 1024) == "S" and P.plan("Fwd", 1, 1, 1025) == "M"
    assert P.plan("Bwd", 128 * 511, 128, 1025) == "M" and P.plan("Bwd", 128 * 511 + 1, 128, 1025) == "L"
    assert P.plan("Trans", 128, 128 * 511 + 1, 2000) == "L"
    assert P.plan_project(1024) == "S" and P.plan_project(1028) == "M"
    assert P.arm((0x1000, 0x2000), 120) == "vec" and P.arm((0x1004, 0x2000), 120) == "scalar"
    assert P.arm((0x1000, 0x2004), 120) == "scalar" and P.arm((0x1000, 0x2000), 119) == "scalar"
    assert P.extents("Fwd", 21, 27, 16, 32, k=3, s=2, p=1) == (11 * 14, 32, 144)
    assert P.extents("Bwd", 21, 27, 16, 32, k=3, s=2, p=1) == (567, 16, 288)
    assert P.extents("Trans", 29, 31, 1028, 516, s=4) == (899, 8256, 1028)


def test_every_case_lands_on_its_form():
    assert len(P.BY_ID) == len(P.CASES)
    for c in P.CASES:
        rows, cols, depth = P.case_extents(c)
        assert P.case_plan(c) == c["form"], (c["id"], rows, cols, depth, P.large_tiles(rows, cols), P.case_plan(c))
        if c["pair"]:
            a, b = c["geom"], P.BY_ID[c["pair"]]["geom"]
            assert c["entry"] == P.BY_ID[c["pair"]]["entry"] and a["H"] < b["H"] and {k: v for k, v in a.items() if k != "H"} == \
                {k: v for k, v in b.items() if k != "H"}, "a pair shares everything but the number of image rows"


def test_claims_about_earlier_tests_hold():
    from tests import image_backbone2d3d_ref as R
    for c in P.EXISTING:
        path = os.path.join(ROOT, "tests", c["file"])
        with open(path) as f:
            assert re.search(r"^def %s\(" % re.escape(c["test"]), f.read(), re.M), (c["file"], c["test"])
        if c["name"]:
            k, s, p, d, cin, cout, H, W = R.CONV_CASES[c["name"]]
            assert d == 1 and dict(H=H, W=W, cin=cin, cout=cout, k=k, s=s, p=p) == c["geom"], (c["name"], R.CONV_CASES[c["name"]], c["geom"])
        if c["entry"] in ("Fwd/plain", "Fwd/ACT", "Fwd/PROJECT", "Trans"):
            assert c["geom"]["cin"] % 4 == 0                  # the MFMA kernel, not the direct one
        else:
            assert c["geom"]["cout"] % 4 == 0


def test_the_table_covers_every_reachable_cell():
    cov = P.coverage()
    text = table(cov)
    print("\n" + text)
    assert len(cov) == 4 * 3 * 2 + 2 * 2 and set(cov) == set(P.reachable_cells())
    empty = [cell for cell, who in cov.items() if not who]
    assert not empty, "cells nobody reaches: %s\n%s" % (empty, text)
    # the forms this table is about are reached by the table itself, on both arms
    for e, f in [(e, f) for e in ("Fwd/plain", "Fwd/ACT", "Bwd", "Trans") for f in ("M", "L")] + [("Fwd/PROJECT", "M")]:
        for a in P.ARMS:
            assert any(w.startswith("test_conv_forms_gpu.py") for w in cov[(e, f, a)]), "the table itself runs %s %s %s\n%s" % (e, f, a, text)


def differ_in_one_extent(a, b):
    ra, rb = P.case_extents(a), P.case_extents(b)
    return a["entry"] == b["entry"] and sum(x != y for x, y in zip(ra, rb)) == 1


def test_both_thresholds_are_straddled():
    depth_pairs, tile_pairs = [], []
    for a in P.CASES:
        for b in P.CASES:
            if not differ_in_one_extent(a, b):
                continue
            (ra, ca, da), (rb, cb, db) = P.case_extents(a), P.case_extents(b)
            if da <= P.CV_SHORT_K < db and (ra, ca) == (rb, cb) and (P.case_plan(a), P.case_plan(b)) == ("S", "M"):
                depth_pairs.append((a["id"], da, b["id"], db))
            ta, tb = P.large_tiles(ra, ca), P.large_tiles(rb, cb)
            if da == db > P.CV_SHORT_K and ta < P.CV_LARGE_TILES <= tb and (P.case_plan(a), P.case_plan(b)) == ("M", "L"):
                tile_pairs.append((a["id"], ta, b["id"], tb))
    print("\ndepth threshold %d straddled by %s\ntile threshold %d straddled by %s" % (P.CV_SHORT_K, depth_pairs, P.CV_LARGE_TILES, tile_pairs))
    assert depth_pairs, "no pair of cases on the two sides of CV_SHORT_K that differs in the depth alone"
    assert {p[0].split("_")[0] for p in tile_pairs} >= {"fwd", "bwd"}, "CV_LARGE_TILES is straddled for the forward and the data gradient"
    # the sides are as tight as ragged edges allow: the depth pair is 1 024 | 1 028 (the next multiple of 4), the L side is 512 tiles exactly
    assert any(p[1] == P.CV_SHORT_K and p[3] == P.CV_SHORT_K + 4 for p in depth_pairs)
    assert all(p[3] == P.CV_LARGE_TILES for p in tile_pairs)
